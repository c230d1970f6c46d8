"""Every slot of the training forward's activation buffer (inerf_encode_mlp_train, include/inerf.h) against fp64, point for point,
in all five saving kernels - and, through the two encoding slots, the fused kernels' own position / direction encoder
(csrc/mlp_f16_dev.h fast_sincosf, the positions x = o + d z in two fp32 roundings) against fp64 sin / cos of the fp32 argument.

The networks of the other tests damp band f of the encoding by 2^-f, so an encoder error of 1e-4 in a high band reaches no
output they look at; the encoding slots show it undamped.  The buffer is pre-filled with a NaN word, so an unwritten half shows
(the weight-gradient kernels DMA whole tiles: the padding rows of the last tile count).

Worst figures on an MI355X (profiles/forward_slots.txt has every line the module prints):
  sweep    sin / cos columns 1.45e-7 (band 0, cos of -3.9002) against the bound of 3.5e-7, the worst of every form and band between
           1.1e-7 and 1.5e-7; identity columns 2.0e-10 inside their bound at the closest
  slots    err / D: 13.31 in enc (32 955 points; its D is the fp32 sine's 3.6e-8, its error the split of an identity column at
           |x| = 5.6: it passes through the bound's second term, err / bound 0.17), at most 3.98 in every other slot (dir; 2.81 in a
           layer slot); err / (4 D + 2^-21 max) at most 0.42 (h6 at one point): the factor 4 stands
  act_max  1.8143 for a largest decoded value of 1.8127 (SSR, 703 points): an upper bound (csrc/mlp_f16_dev.h split_upper_bound),
           where the largest hi half alone is 1.8125
  lo opposed to hi: 0.4 to 0.5 of the values in enc / dir (hi to nearest), none in the layer slots (hi towards zero) - include/inerf.h
"""
import functools

import pytest
import torch

import _forward_slots as fs
import _raw_rows as rr
import oracle
from intrinsicnerf_amd import _capi, kernels, packing

pytestmark = pytest.mark.gpu

FORMS = {"default": {}, "single": {"INERF_F16_KERNEL": "single"}, "t128": {"INERF_TRAIN_FWD": "t128"}}
TAG = "forward_slots |"          # every figure this module prints starts with it


def _select_form(monkeypatch, form):
    for name in ("INERF_F16_KERNEL", "INERF_TRAIN_FWD"):
        monkeypatch.delenv(name, raising=False)
    for name, value in FORMS[form].items():
        monkeypatch.setenv(name, value)


def _desc(variant, classes, l_xyz=10, l_dir=4):
    ssr = variant == "ssr"
    return _capi.net_desc(_capi.VARIANT_SSR if ssr else _capi.VARIANT_OBJECT, classes, l_xyz, l_dir, 10.0 if ssr else 1.0, _capi.PREC_F16X3)


def _fragment_slot(desc, save, n, slot):
    """(planes [2, padded, width] on the CPU, their halves as bit patterns) of a FRAGMENT slot over its whole tiles."""
    words, width = fs.slot_words(desc, save, n, slot)
    planes = fs.frag_planes(words, width).cpu()
    return planes, fs.halves_bits(planes)


def _opposed_share(planes):
    """Share of the values whose lo half has the other sign than hi: none when hi is rounded towards zero, about half of them when
    it is rounded to nearest (include/inerf.h says which slot does which)."""
    hi, lo = planes[0].float(), planes[1].float()
    return float(((hi * lo) < 0).float().mean())


def _check_padding(name, bits, n, problems):
    """No half of the slot's whole-tile range still holds the sentinel; the padding rows are the last point's, bit for bit."""
    left = int((bits == fs.SENTINEL_HALF).sum())
    if left:
        rows = (bits == fs.SENTINEL_HALF).any(0).any(-1).nonzero().flatten()
        problems.append(f"{name}: {left} halves never written, rows {rows[:4].tolist()} .. {int(rows[-1])} of {bits.shape[1]} (n = {n})")
    if bits.shape[1] > n and not torch.equal(bits[:, n:], bits[:, n - 1:n].expand_as(bits[:, n:])):
        bad = (bits[:, n:] != bits[:, n - 1:n]).any(0).any(-1).nonzero().flatten() + n
        problems.append(f"{name}: padding rows {bad[:8].tolist()} are not a copy of row {n - 1}")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the encoder, through the enc / dir slots
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_RAYS = 4099                # 65 tiles, three points in the last one
SINCOS_BOUND = 3.5e-7            # 9.3e-8 (fast_sincosf against fp64, |a| < 2^15; ocml beyond is tighter) + 2^-22 (hi / lo split of 8 v, |v| <= 1)


@functools.lru_cache(maxsize=None)
def _sweep(xyz_div):
    """(rays, z, fp32 positions, fp32 directions, fp64 position encoding [n, 63], fp64 direction encoding [n, 27]) - shared and left alone."""
    rays, z = fs.sweep_rays(SWEEP_RAYS)
    x, v = fs.positions(rays, z, xyz_div), fs.directions(rays, 1)
    return rays, z, x, v, fs.encode(x, 10, torch.float64), fs.encode(v, 4, torch.float64)


def _zero_weights(variant, classes, l_xyz, l_dir):
    return {k: torch.zeros(shape) for k, shape in oracle.state_dict_spec(variant, classes, l_xyz, l_dir)}


def _run_sweep(variant, classes, endpoint, l_xyz, l_dir):
    dev = torch.device("cuda:0")
    desc = _desc(variant, classes, l_xyz, l_dir)
    packed = packing.pack_state_dict(desc, _zero_weights(variant, classes, l_xyz, l_dir)).to(dev)
    rays, z = _sweep(desc.xyz_div)[:2]
    return (desc,) + fs.run_train_forward(desc, packed, rays.to(dev), z.to(dev), endpoint)


@pytest.mark.parametrize("variant,classes,endpoint,form,l_xyz,l_dir", [
    pytest.param("object", 0, False, "default", 10, 4, id="object-default"),
    pytest.param("object", 0, False, "single", 10, 4, id="object-single"),
    pytest.param("object", 0, False, "t128", 10, 4, id="object-t128"),
    pytest.param("ssr", 28, False, "default", 10, 4, id="ssr28-default"),
    pytest.param("ssr", 5, True, "default", 10, 4, id="ssr5-endpoint"),             # the endpoint feature takes the one-workgroup kernel
    pytest.param("object", 0, False, "default", 3, 0, id="object-default-L3-0")])   # a reduced encoder: other pad columns
def test_encoder_sweep_through_the_encoding_slots(variant, classes, endpoint, form, l_xyz, l_dir, monkeypatch, request):
    """All-zero weights (nothing but the encodings can be anything), d = 0 and z = 1 (x = o exactly; 64 rows of a repeat of the list have
    d != 0 and z in [2, 6] instead, so that a position formed in one rounding shows here too): columns 0:3 / 8:11 of 4 099 rays
    carry the arguments - random ones, the fp32 neighbourhoods of the quadrant edges m pi / 4 / 2^f of every band, zeros and
    subnormals, and both sides of |x 2^f| = 2^15 where fast_sincosf hands over to ocml (positions at 64, directions at 4096).
    sin / cos columns: |got - fp64 sin / cos of the fp32 argument| <= 3.5e-7 = 9.3e-8 (the encoder's own error) + 2^-22 (the
    hi / lo split of 8 v at |v| <= 1).  A position formed by one fused multiply-add is 2.4e-4 in band 9, a dropped reduction
    constant 1e-4.  Identity columns: the split's 22 bits.  Pad columns: zero in both planes.  Padding rows of the 65th tile: the
    last point's halves.  t128: the words of the default form."""
    case = request.node.callspec.id
    print()                                        # (under -s the figures start on a line of their own)
    _select_form(monkeypatch, form)
    desc, raw, save, act_max, status = _run_sweep(variant, classes, endpoint, l_xyz, l_dir)
    n = SWEEP_RAYS
    _, _, x, v, enc64, dir64 = _sweep(desc.xyz_div)
    problems = []
    for slot, arg, want, bands in ((kernels.SAVE_ENC, x, enc64, l_xyz), (kernels.SAVE_DIR, v, dir64, l_dir)):
        name = fs.SLOT_NAMES[slot]
        planes, bits = _fragment_slot(desc, save, n, slot)
        _check_padding(name, bits, n, problems)
        got = fs.planes_value(planes)[:n]
        cols = 3 + 6 * bands
        # identity columns: hi + lo carry 22 bits of 8 x, down to f16's smallest subnormal
        ident = (got[:, :3] - arg.double()).abs()
        over = ident - (2.0 ** -21 * arg.double().abs() + 2.0 ** -28)
        print(f"{TAG} sweep {case} {name} identity: worst |err| {float(ident.max()):.3e}, worst (err - bound) {float(over.max()):.3e}, "
              f"lo opposed to hi {_opposed_share(planes):.3f}")
        if not float(over.max()) <= 0:
            r, c = divmod(int(over.argmax()), 3)
            problems.append(f"{name} identity column {c}: {float(got[r, c])!r} for {float(arg[r, c])!r}")
        # sin / cos columns, band by band
        for f in range(bands):
            err = (got[:, 3 + 6 * f: 9 + 6 * f] - want[:, 3 + 6 * f: 9 + 6 * f]).abs()
            worst = float(err.max())
            r, c = divmod(int(err.argmax()), 6)
            print(f"{TAG} sweep {case} {name} band {f}: worst |err| {worst:.3e} ({'sin' if c < 3 else 'cos'} of {float(arg[r, c % 3]) * 2 ** f!r})")
            if not worst <= SINCOS_BOUND:
                problems.append(f"{name} band {f}: |err| {worst:.3e} > {SINCOS_BOUND} ({'sin' if c < 3 else 'cos'} of {float(arg[r, c % 3]) * 2 ** f!r}, "
                                f"{int((err > SINCOS_BOUND).sum())} values over)")
        if not bool(torch.isfinite(got[:, :cols]).all()):
            problems.append(f"{name}: non-finite values")
        # pad columns: both halves zero, in the padding rows too
        nonzero = int((planes[:, :, cols:] != 0).sum())
        if nonzero:
            problems.append(f"{name}: {nonzero} non-zero halves in the pad columns {cols}..")
    print(f"{TAG} sweep {case}: act_max {act_max!r}, status {status}")
    if form == "t128":
        _select_form(monkeypatch, "default")
        ref = _run_sweep(variant, classes, endpoint, l_xyz, l_dir)[2]
        for slot in (kernels.SAVE_ENC, kernels.SAVE_DIR):
            if not torch.equal(fs.slot_words(desc, save, n, slot)[0], fs.slot_words(desc, ref, n, slot)[0]):
                problems.append(f"{fs.SLOT_NAMES[slot]}: the 128-point tile's words differ from the default form's")
    assert status == 0
    assert bool(torch.isfinite(raw).all())
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# 2. every slot, point for point
# ---------------------------------------------------------------------------------------------------------------------
WEIGHT_SEED = 11
# 4 = 2^(24 - 22): the kernels' operands (f16 hi + lo) carry 22 bits where the fp32 reference's carry 24
YARDSTICK_FACTOR = 4.0


def _tile_loop_points():
    """64 (2 CUs + 3) - 5: three tiles more than the two-workgroup grid holds, the last one ragged and in a second-round workgroup."""
    return 64 * (2 * torch.cuda.get_device_properties(0).multi_processor_count + 3) - 5


def _split(p):
    """(rays, samples per ray) with rays * samples = p: the largest sample count up to 24 that divides p."""
    s = max(k for k in range(1, 25) if p % k == 0)
    return p // s, s


@functools.lru_cache(maxsize=None)
def _reference(variant, classes, endpoint, p):
    """(rays, z, fp64 slots, fp32 slots) of one case on the CPU - computed once, shared by the forms, left alone."""
    ssr = variant == "ssr"
    n, s = _split(p)
    rays, z = fs.rays_and_depths(n, s, seed=p % 1000, origin_scale=3.0 if ssr else 1.0)
    net = fs.make_module(variant, classes, oracle.make_state_dict(variant, classes, seed=WEIGHT_SEED))
    div = 10.0 if ssr else 1.0
    return rays, z, fs.reference_slots(net, rays, z, div, endpoint), fs.reference_slots(net, rays, z, div, endpoint, dtype=torch.float32)


@pytest.mark.parametrize("variant,classes,endpoint,form,points", [
    pytest.param("object", 0, False, "default", 1, id="object-default-1"),
    pytest.param("object", 0, False, "default", 63, id="object-default-63"),
    pytest.param("object", 0, False, "default", 64, id="object-default-64"),
    pytest.param("object", 0, False, "default", 65, id="object-default-65"),
    pytest.param("object", 0, False, "default", 703, id="object-default-703"),           # eleven tiles, ragged
    pytest.param("object", 0, False, "default", None, id="object-default-tile-loop"),
    pytest.param("object", 0, False, "single", 65, id="object-single-65"),
    pytest.param("object", 0, False, "single", 703, id="object-single-703"),
    pytest.param("ssr", 28, False, "default", 703, id="ssr28-default-703"),
    pytest.param("ssr", 28, False, "single", 703, id="ssr28-single-703"),
    pytest.param("ssr", 28, False, "default", None, id="ssr28-default-tile-loop"),
    pytest.param("ssr", 5, True, "default", 147, id="ssr5-endpoint-147"),
    pytest.param("ssr", 0, False, "default", 65, id="ssr0-default-65")])                 # no semantic head: semh has width 0
def test_every_slot_point_for_point_against_fp64(variant, classes, endpoint, form, points, monkeypatch, request):
    """Default-init weights, the camera of test_train_masks_gpu (SSR: origins moved out by 3).  For every slot of non-zero width:
    max |got - fp64| <= 4 D + 2^-21 max |fp64|, D = how far the reference's own fp32 arithmetic lands from fp64 on the same slot
    (computed here) and 4 = 2^(24 - 22), the kernels' operands carrying 22 bits where fp32's carry 24 (enc goes beyond 4 D - its D is the
    fp32 sine's error, which knows nothing of the identity columns' |x| - and passes through the second term, the split's own 2^-22 |x|);
    fragment slots: the padding
    rows of the last tile hold the last point's halves and no half of the whole-tile range is unwritten; the row-format slot
    (semh): every row of a point written.  act_max is not below the largest value any slot decodes to; status stays 0.  The raw rows
    of the same launch: every channel group at the same yardstick (tests/_raw_rows.py judge; figures in tests/test_raw_rows_gpu.py)."""
    case = request.node.callspec.id
    print()                                        # (under -s the figures start on a line of their own)
    dev = torch.device("cuda:0")
    p = _tile_loop_points() if points is None else points
    _select_form(monkeypatch, form)
    desc = _desc(variant, classes)
    rays, z, want64, want32 = _reference(variant, classes, endpoint, p)
    sd = {k: t.to(dev) for k, t in oracle.make_state_dict(variant, classes, seed=WEIGHT_SEED).items()}
    packed = packing.device_packer(desc, False, dev)(sd)
    raw, save, act_max, status = fs.run_train_forward(desc, packed, rays.to(dev), z.to(dev), endpoint)
    lib = _capi.lib()
    problems = []
    largest = 0.0
    for slot in fs.ACTIVATION_SLOTS:
        name = fs.SLOT_NAMES[slot]
        words, width = fs.slot_words(desc, save, p, slot)
        assert width == want64[slot].shape[1], name
        if width == 0:
            continue
        if lib.inerf_mlp_save_slot_is_fragment(slot, 0) == 1:
            planes, bits = _fragment_slot(desc, save, p, slot)
            _check_padding(name, bits, p, problems)
            got = fs.planes_value(planes)[:p]
            opposed = f", lo opposed to hi {_opposed_share(planes):.3f}"
        else:
            rows = words[:p * width].cpu()
            left = int((rows == fs.SENTINEL).sum())
            if left:
                problems.append(f"{name}: {left} words of the points' rows never written")
            got = rows.view(torch.float32).view(p, width).double()
            opposed = ""
        want = want64[slot]
        err = (got - want).abs()
        worst = float(err.max())
        d = float((want32[slot].double() - want).abs().max())
        bound = YARDSTICK_FACTOR * d + 2.0 ** -21 * float(want.abs().max())
        largest = max(largest, float(got.abs().max()))
        print(f"{TAG} slots {case} {name}: err {worst:.3e}, D {d:.3e}, err / D {worst / d:.2f}, err / bound {worst / bound:.2f}, max |value| {float(want.abs().max()):.3f}{opposed}")
        if not worst <= bound:
            over = err > bound
            problems.append(f"{name}: |err| {worst:.3e} > {bound:.3e} = 4 x {d:.3e} + 2^-21 x {float(want.abs().max()):.3f}; {int(over.sum())} values over, in "
                            f"{int(over.any(1).sum())} of {p} points, {len(set((over.any(1).nonzero().flatten() // 64).tolist()))} tiles")
    print(f"{TAG} slots {case}: act_max {act_max!r}, largest decoded |value| {largest!r}, status {status}")
    if not act_max >= largest:
        problems.append(f"act_max {act_max!r} is below the largest decoded |value| {largest!r}")
    # the same launch's raw rows, one layer behind the last slots: per channel group at the same yardstick (tests/_raw_rows.py)
    rr.judge(raw.reshape(p, -1), want64["raw"], want32["raw"], rr.groups(variant, classes, endpoint), f"slots {case}", problems)
    assert status == 0
    assert bool(torch.isfinite(raw).all())
    assert not problems, "; ".join(problems)
