"""What the training forward (inerf_encode_mlp_train) should leave in every slot of its activation buffer, and how to read the
buffer back half by half.

``reference_slots`` evaluates the package's own torch module on the CPU - fp64 for the expected values, fp32 for the yardstick
(how far the reference's own arithmetic lands from fp64 on the same inputs) - on the encoding of the fp32 positions the kernels
form, and returns the slots of csrc/layout.h SaveSlot from forward hooks on the module's ``nn.Linear`` layers.  The positions
are the kernels' to the bit: x = fl32(o + fl32(d z)), for the scene-level network divided once more in fp32; everything after
that is the precision under test.

``run_train_forward`` launches the kernel through the C ABI on a buffer pre-filled with a word that is a NaN as fp32 and in
both of its f16 halves, so that an unwritten word shows; ``slot_planes`` / ``slot_values`` decode a FRAGMENT slot (include/inerf.h)
into its hi and lo planes over the slot's WHOLE tiles - the padding rows of the last tile belong to the slot."""
import copy
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from intrinsicnerf_amd import _capi, kernels

SENTINEL = 0x7FC07FC0            # int32 word: quiet NaN as fp32, and 0x7FC0 (quiet NaN) in both f16 halves
SENTINEL_HALF = 0x7FC0
SLOT_NAMES = {kernels.SAVE_ENC: "enc", kernels.SAVE_DIR: "dir", kernels.SAVE_AS1H: "as1h", kernels.SAVE_FEAT: "feat",
              kernels.SAVE_VH: "vh", kernels.SAVE_SEMH: "semh"}
SLOT_NAMES.update({kernels.SAVE_H0 + i: f"h{i}" for i in range(8)})
ACTIVATION_SLOTS = tuple(sorted(SLOT_NAMES))


# ---------------------------------------------------------------------------------------------------------------------
# CPU reference
# ---------------------------------------------------------------------------------------------------------------------
def positions(rays, z, xyz_div):
    """fp32 [n * s, 3] sample positions as the kernels form them: one fp32 product, one fp32 sum (never a fused multiply-add),
    then - xyz_div != 1 - one fp32 true division (by a tensor: no reciprocal shortcut)."""
    rays, z = rays.detach().cpu().float(), z.detach().cpu().float()
    prod = rays[:, None, 3:6] * z[:, :, None]
    x = (rays[:, None, 0:3] + prod).reshape(-1, 3)
    if xyz_div != 1.0:
        x = x / torch.full_like(x, float(xyz_div))
    return x


def directions(rays, n_samples):
    rays = rays.detach().cpu().float()
    return rays[:, None, 8:11].expand(rays.shape[0], n_samples, 3).reshape(-1, 3)


def encode(x, n_freqs, dtype):
    """[x, sin(x 2^f), cos(x 2^f) ...] of fp32 ``x`` evaluated in ``dtype`` (x 2^f is exact in either)."""
    x = x.to(dtype)
    parts = [x]
    for f in range(n_freqs):
        parts += [torch.sin(x * float(2 ** f)), torch.cos(x * float(2 ** f))]
    return torch.cat(parts, -1)


def _pad(m, width):
    return torch.cat([m, m.new_zeros(m.shape[0], width - m.shape[1])], -1)


def reference_slots(module, rays, z, xyz_div, endpoint, dtype=torch.float64):
    """{slot: [n_points, width]} of ``module`` (object_level.NeRF / ssr.Semantic_NeRF; a copy is evaluated, on the CPU in ``dtype``)
    on ``rays`` [n, 11] and depths ``z`` [n, s]; under "raw" the module's output and under "emb" its input.  fp32: the
    reference's arithmetic - fp32 sin / cos of the fp32 argument, fp32 layers - on the same fp32 positions."""
    net = copy.deepcopy(module).cpu().to(dtype)
    l_xyz, l_dir = (net.input_ch - 3) // 6, (net.input_ch_views - 3) // 6
    enc = encode(positions(rays, z, xyz_div), l_xyz, dtype)
    dirs = encode(directions(rays, z.shape[1]), l_dir, dtype)
    emb = torch.cat([enc, dirs], -1)
    kept = {}
    hooks = [m.register_forward_hook(lambda mod, args, out, name=name: kept.__setitem__(name, out.detach()))
             for name, m in net.named_modules() if isinstance(m, torch.nn.Linear)]
    try:
        with torch.no_grad():
            raw = net(emb, True) if (endpoint and hasattr(net, "enable_semantic")) else net(emb)
    finally:
        for h in hooks:
            h.remove()
    shading1 = "shading_linear1" if "shading_linear1" in kept else "test_linear1"       # (object-level: test_linear1 is the shading head)
    slots = {kernels.SAVE_ENC: _pad(enc, 64), kernels.SAVE_DIR: _pad(dirs, 32)}
    for layer in range(8):
        slots[kernels.SAVE_H0 + layer] = F.relu(kept[f"pts_linears.{layer}"])
    slots[kernels.SAVE_AS1H] = torch.cat([F.relu(kept["albedo_linear1"]), F.relu(kept[shading1])], -1)
    slots[kernels.SAVE_FEAT] = kept["feature_linear"]
    slots[kernels.SAVE_VH] = F.relu(kept["views_linears.0"])
    sem = kept.get("semantic_linear.0.0")
    slots[kernels.SAVE_SEMH] = F.relu(sem) if sem is not None else enc.new_zeros(enc.shape[0], 0)
    slots["raw"], slots["emb"] = raw, emb
    return slots


def heads_from_slots(module, slots, endpoint):
    """The module's output continued from the LAST slots (h7, the two hidden layers of the heads, the views and semantic hidden
    layers) through its output heads, in the slots' dtype: equal to the module's own output only if the slots are what the
    module computed where the mapping says."""
    net = copy.deepcopy(module).cpu().to(slots[kernels.SAVE_H0 + 7].dtype)
    ssr = hasattr(net, "enable_semantic")
    h7, as1h, vh, semh = (slots[s] for s in (kernels.SAVE_H0 + 7, kernels.SAVE_AS1H, kernels.SAVE_VH, kernels.SAVE_SEMH))
    with torch.no_grad():
        sigma = net.alpha_linear(h7)
        albedo = torch.sigmoid(net.albedo_linear2(as1h[:, :128].contiguous()))
        shading = torch.sigmoid((net.shading_linear2 if ssr else net.test_linear2)(as1h[:, 128:].contiguous()))
        residual = torch.sigmoid((net.residual_linear if ssr else net.shading_linear)(vh))
        parts = [albedo * shading + residual, sigma, albedo, shading, residual]
        if semh.shape[1]:
            parts.append(net.semantic_linear[1](semh))
        if endpoint and ssr:
            parts.append(vh)
    return torch.cat(parts, -1)


def chain_from_slots(module, slots):
    """{slot: value} of every slot that has a predecessor, recomputed from the PREVIOUS slots (h_l from h_(l-1) and, at the
    skip layer, enc; the heads' hidden layers and feat from h7; vh from feat and dir): the slot mapping link by link."""
    net = copy.deepcopy(module).cpu().to(slots[kernels.SAVE_H0].dtype)
    enc, dirs = slots[kernels.SAVE_ENC][:, :net.input_ch], slots[kernels.SAVE_DIR][:, :net.input_ch_views]
    out = {}
    with torch.no_grad():
        out[kernels.SAVE_H0] = F.relu(net.pts_linears[0](enc))
        for layer in range(1, 8):
            h = slots[kernels.SAVE_H0 + layer - 1]
            out[kernels.SAVE_H0 + layer] = F.relu(net.pts_linears[layer](torch.cat([enc, h], -1) if layer - 1 in net.skips else h))
        h7 = slots[kernels.SAVE_H0 + 7]
        sh1 = net.shading_linear1 if hasattr(net, "shading_linear1") else net.test_linear1
        out[kernels.SAVE_AS1H] = torch.cat([F.relu(net.albedo_linear1(h7)), F.relu(sh1(h7))], -1)
        out[kernels.SAVE_FEAT] = net.feature_linear(h7)
        out[kernels.SAVE_VH] = F.relu(net.views_linears[0](torch.cat([slots[kernels.SAVE_FEAT], dirs], -1)))
        if slots[kernels.SAVE_SEMH].shape[1]:
            out[kernels.SAVE_SEMH] = net.semantic_linear[0](h7)
    return out


def make_module(variant, classes, state_dict=None, l_xyz=10, l_dir=4):
    from intrinsicnerf_amd import object_level, ssr
    kw = dict(D=8, W=256, input_ch=3 + 6 * l_xyz, output_ch=5, skips=[4], input_ch_views=3 + 6 * l_dir, use_viewdirs=True)
    net = ssr.Semantic_NeRF(classes > 0, classes, **kw) if variant == "ssr" else object_level.NeRF(**kw)
    if state_dict is not None:
        net.load_state_dict(state_dict)
    return net


def rays_and_depths(n, s, seed=0, origin_scale=1.0):
    """The camera of test_train_masks_gpu._rays (one origin, directions scattered about the view of the world's origin, depths
    sorted in [2, 6]) on the CPU; ``origin_scale`` moves the ray origins out (columns 0:3 only)."""
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([[2.5, 1.5, 2.0]]).expand(n, 3)
    d = -o / o.norm(dim=-1, keepdim=True) + 0.2 * torch.randn(n, 3, generator=g)
    rays = torch.cat([o * origin_scale, d, 2 * torch.ones(n, 1), 6 * torch.ones(n, 1), d / d.norm(dim=-1, keepdim=True)], -1)
    z = torch.sort(torch.rand(n, s, generator=g) * 4 + 2, -1)[0]
    return rays.contiguous(), z.contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the encoder sweep's arguments
# ---------------------------------------------------------------------------------------------------------------------
def _neighbours(v):
    """fp32 ``v`` with its two fp32 neighbours on each side."""
    v = np.float32(v)
    out, lo, hi = [v], v, v
    for _ in range(2):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return out


def sweep_arguments(direction):
    """The encoder sweep's argument list as a float32 tensor: random arguments, the fp32 neighbourhoods of the quadrant edges
    m pi / 4 / 2^f of every band (the ends of the polynomials' interval; |x| < 64 for positions, < 4096 for directions), zeros,
    subnormals, +-1 and the switch to the large-argument path at |x 2^f| = 2^15 (``direction``: also around 2^3 v = 2^15)."""
    g = torch.Generator().manual_seed(2024)
    vals = [np.float32(v) for v in ((torch.rand(1000, generator=g, dtype=torch.float64) * 12 - 6).float().tolist()
                                    + (torch.rand(500, generator=g, dtype=torch.float64) * 2 - 1).float().tolist())]
    limit = 4096.0 if direction else 64.0
    for f in range(10):
        for m in (1, 2, 3, 7, 100, 1001, 20860):
            for sign in (1, -1):
                vals += [v for v in _neighbours(sign * m * math.pi / 4 / 2 ** f) if abs(float(v)) < limit]
    vals += [np.float32(v) for v in (0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 1e-40, -1e-40, 1.0, -1.0)]
    vals += [np.float32(v) for v in (63.99999, 64.0, -64.0, 64.00001, 100.0, 1000.0)]
    if direction:
        vals += [np.float32(v) for v in (4095.9, 4096.0, -4096.0, 5000.0)]
    out = torch.from_numpy(np.array(vals, dtype=np.float32))
    assert bool(torch.isfinite(out).all())
    return out


MOVED_ROWS = 64                  # rows of the sweep whose position is o + d z with d != 0


def sweep_rays(n):
    """[n, 11] rays whose columns 0:3 / 8:11 carry the position / direction argument lists, each component in an order of its
    own (repeated to ``n`` rows), and the depths [n, 1].  d = 0 and z = 1 (x = o exactly) - except in MOVED_ROWS rows of one
    of the repeats (the last whole tile, before the ragged one), where d is random in [-1, 1] and z in [2, 6]: there the
    position is the kernels' fl32(o + fl32(d z)), which a fused multiply-add misses by an ulp in many of them."""
    rays = torch.zeros(n, 11)
    for base, direction in ((0, False), (8, True)):
        args = sweep_arguments(direction)
        assert args.numel() + MOVED_ROWS + 64 <= n
        for c in range(3):
            order = torch.randperm(args.numel(), generator=torch.Generator().manual_seed(10 * base + c))
            rays[:, base + c] = args[order.repeat(-(-n // args.numel()))[:n]]
    rays[:, 6], rays[:, 7] = 2.0, 6.0
    z = torch.ones(n, 1)
    g = torch.Generator().manual_seed(77)
    rows = moved_rows(n)
    rays[rows, 3:6] = torch.rand(MOVED_ROWS, 3, generator=g) * 2 - 1
    z[rows, 0] = torch.rand(MOVED_ROWS, generator=g) * 4 + 2
    return rays.contiguous(), z


def moved_rows(n):
    """The rows of ``sweep_rays(n)`` with d != 0: the last whole tile."""
    first = (n // 64 - 1) * 64
    return slice(first, first + MOVED_ROWS)


def fused_positions(rays, z):
    """What ONE rounding would make of the positions: fl32(o + d z) with the product exact (fp64 holds it; the sum's second
    rounding, to fp64 first, moves the result only at ties of 2^-29 of the cases) - the defect the moved rows are there for."""
    rays, z = rays.detach().cpu().double(), z.detach().cpu().double()
    return (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3).float()


# ---------------------------------------------------------------------------------------------------------------------
# the kernel and its buffer
# ---------------------------------------------------------------------------------------------------------------------
def run_train_forward(desc, packed, rays, z, endpoint=False, raw=None):
    """inerf_encode_mlp_train through the C ABI on a sentinel-filled buffer: (raw [n, s, ch], the buffer as int32 words,
    act_max as a float, status as an int), synchronised.  ``raw``: a caller-owned contiguous fp32 view of n * s * ch floats to write
    the rows into (returned as it is) instead of a fresh tensor."""
    lib = _capi.lib()
    dev = rays.device
    n, s = z.shape
    flags = kernels.FLAG_ENDPOINT if endpoint else 0
    if raw is None:
        raw = torch.zeros(n, s, lib.inerf_raw_channels(desc, flags, 1), device=dev)
    assert raw.is_contiguous() and raw.dtype == torch.float32 and raw.numel() == n * s * lib.inerf_raw_channels(desc, flags, 1)
    save = torch.full((lib.inerf_mlp_save_floats(desc, n * s),), SENTINEL, dtype=torch.int32, device=dev)
    act_max = torch.zeros(1, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        rc = lib.inerf_encode_mlp_train(desc, p(packed), p(rays), p(z), n, s, flags, p(raw), p(save), p(act_max), p(status),
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _capi.check(rc, "inerf_encode_mlp_train")
    torch.cuda.synchronize(dev)
    return raw, save, float(act_max), int(status)


def slot_words(desc, save, n_points, slot):
    """(the int32 words of ``slot`` over its whole tiles, width) of an activation buffer given as int32 words."""
    off, width = C.c_int64(), C.c_int()
    _capi.check(_capi.lib().inerf_mlp_save_slot(desc, slot, n_points, C.byref(off), C.byref(width)), "inerf_mlp_save_slot")
    padded = (n_points + 63) // 64 * 64
    return save[off.value: off.value + padded * width.value], width.value


def frag_planes(words, width):
    """A FRAGMENT slot's int32 words (whole tiles) -> its f16 halves as a [2 (hi, lo), points, width] float16 tensor (include/inerf.h;
    the index arithmetic of kernels.frag_decode with the planes kept apart and the padding rows kept)."""
    h = words.view(torch.float16)
    cbs = width // 32
    tiles = h.numel() // (64 * width * 2)
    v = h.view(tiles, 2, 2, cbs, 2, 2, 32, 2, 4)                   # [tile, pb, q, cb, plane, h, c, i_hi, i_lo]
    return v.permute(4, 0, 1, 2, 7, 5, 8, 3, 6).reshape(2, tiles * 64, width)      # [plane, (tile, pb, q, i_hi, h, i_lo), (cb, c)]


def halves_bits(planes):
    return planes.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def planes_value(planes):
    """(hi + lo) / 8 in fp64: exact (the fp32 sum of two halves can round)."""
    return (planes[0].double() + planes[1].double()) / kernels.ACT_SCALE
