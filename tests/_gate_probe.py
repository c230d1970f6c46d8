"""Shared by tests/test_gate_probe_cpu.py and tests/test_gate_probe_gpu.py: the density gate's probe restated in
torch, the fp64 trunk it is judged against, and the networks and sample points both tests use."""
import glob
import os

import numpy as np
import torch

from conftest import REPO

KAPPA = 2.0 ** -6          # csrc/mlp_f16_t128.hip kProbeKappa
ACT_SCALE = 8.0            # csrc/layout.h kActScale
F16_SAFE = 6.0e4           # csrc/mlp_f16_dev.h kF16Safe: the range flag is raised when a scaled activation passes it
MODEL_TO_KERNEL = 1.5e-4   # the largest |s_model - s_kernel| / S recorded on whole frames (profiles/gate_probe_margin.txt "model vs kernel":
                           # 1.43e-4), rounded up; tests/test_gate_probe_gpu.py holds the kernel's own distance (up to 4.6e-4 there) to kappa / 8
MIN_SHARE = 0.02           # a case is fair when at least this share of its points has sigma > 0, and at least this share is culled
SKIP = 4                   # pts_linears[5] takes cat([encoding, h4])
L_XYZ = 10


def f16(t):
    """To f16, to nearest, and back (the probe's one conversion per activation)."""
    return t.to(torch.float16).to(t.dtype)


def weight_hi(w):
    """What the probe sees of a packed GEMM (csrc/pack.cpp): W' = W 2^kw with max |W'| in [2^13, 2^14), hi = f16(W') - as (hi, 2^-kw)."""
    m = float(w.abs().max())
    e = int(np.frexp(np.float32(m))[1]) if m > 0 else 14
    scale = 2.0 ** (14 - e)
    return f16(w.float() * scale).double(), 1.0 / scale


def encode(x, dtype):
    """NeRF's positional encoding of fp32 positions (run_nerf_helpers.py: x, sin(2^f x), cos(2^f x), f = 0..9), evaluated in ``dtype``."""
    x = x.to(dtype)
    out = [x]
    for f in range(L_XYZ):
        out += [torch.sin(x * 2.0 ** f), torch.cos(x * 2.0 ** f)]
    return torch.cat(out, -1)


def positions(rays, z):
    """The kernels' fp32 sample positions o + d z, [N * S, 3]."""
    return (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3).float()


def sigma_fp64(sd, x):
    """The trunk and the density head in fp64 on the fp32 weights."""
    enc = encode(x, torch.float64)
    h = enc
    for i in range(8):
        h = torch.relu(h @ sd[f"pts_linears.{i}.weight"].double().T + sd[f"pts_linears.{i}.bias"].double())
        if i == SKIP:
            h = torch.cat([enc, h], -1)
    return (h @ sd["alpha_linear.weight"].double().T + sd["alpha_linear.bias"].double())[:, 0]


def probe_model(sd, x, amax=None):
    """(s, S) of the probe kernel: hi weights, activations as f16(8 h) to nearest, one product per MAC.  The kernel accumulates in
    fp32 on the matrix core; here the sums are fp64 - they differ by ~1e-7 of the sum of magnitudes, three orders below the margin.
    ``amax``: a list that receives the largest scaled activation, the quantity the kernel's f16 range flag looks at."""
    enc = f16(encode(x, torch.float32) * ACT_SCALE).double()
    h = enc
    top = float(enc.abs().max())
    for i in range(8):
        wh, inv = weight_hi(sd[f"pts_linears.{i}.weight"])
        t = (h @ wh.T) * inv + ACT_SCALE * sd[f"pts_linears.{i}.bias"].double()
        top = max(top, float(torch.relu(t).max()))
        h = f16(torch.relu(t).float()).double()
        if i == SKIP:
            h = torch.cat([enc, h], -1)
    wh, inv = weight_hi(sd["alpha_linear.weight"])
    b = sd["alpha_linear.bias"].double()[0]
    s = (h @ wh[0]) * (inv / ACT_SCALE) + b
    big_s = (h @ wh[0].abs()) * (inv / ACT_SCALE) + b.abs()
    if amax is not None:
        amax.append(top)
    return s, big_s


def bench_rays():
    """bench.py's strided 4096-ray sample of the 800 x 800 chair frame, on the CPU."""
    import bench
    from intrinsicnerf_amd import object_level as ol
    ro, rd = ol.get_rays(bench.H, bench.W, bench.chair_intrinsics(), bench.chair_pose())
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    n = bench.H * bench.W
    sel = torch.arange(0, n, n // bench.PARITY_RAYS + 1)[:bench.PARITY_RAYS]
    vd = rd[sel] / rd[sel].norm(dim=-1, keepdim=True)
    one = torch.ones_like(vd[:, :1])
    return torch.cat([ro[sel], rd[sel], bench.NEAR * one, bench.FAR * one, vd], -1).contiguous()


_nets = {}
_holdout = {}

TRUNK_KEYS = tuple(f"pts_linears.{i}.{p}" for i in range(8) for p in ("weight", "bias")) + ("alpha_linear.weight", "alpha_linear.bias")
HOLDOUT_SEED = {"long": 0, "sharp": 1}         # the network seeds of the two fits: the seeds of the filled-in heads too
PART_BYTES = 900 * 1024                        # a fixture is written in parts of at most this many bytes of tensors


def holdout_fixture(which):
    """tests/golden/probe_holdout_<which>.npz and its further parts probe_holdout_<which>.<n>.npz as one dict (a committed file stays
    below 1 MiB; tests/golden/make_golden_probe_holdout.py writes them): ``w_coarse/<key>`` and ``w_fine/<key>`` for TRUNK_KEYS,
    ``rays`` [256, 11], ``z_fine`` [256, 192]."""
    if which not in _holdout:
        stem = os.path.join(REPO, "tests", "golden", f"probe_holdout_{which}")
        paths = [stem + ".npz"] + sorted(glob.glob(stem + ".[0-9]*.npz"))
        fx = {}
        for path in paths:
            with np.load(path) as d:
                fx.update({k: np.array(d[k]) for k in d.files})
        assert len(paths) == int(fx["n_parts"]), (paths, int(fx["n_parts"]))
        _holdout[which] = fx
    return _holdout[which]


def write_holdout_fixture(which, fx):
    """The inverse of ``holdout_fixture``: the entries in their order, greedily into parts of at most PART_BYTES."""
    stem = os.path.join(REPO, "tests", "golden", f"probe_holdout_{which}")
    parts, size = [{}], 0
    for k, v in fx.items():
        v = np.ascontiguousarray(v)
        if parts[-1] and size + v.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    for old in [stem + ".npz"] + glob.glob(stem + ".[0-9]*.npz"):
        if os.path.exists(old):
            os.remove(old)
    paths = []
    for i, part in enumerate(parts):
        paths.append(stem + (".npz" if i == 0 else f".{i}.npz"))
        np.savez_compressed(paths[-1], **part, **({"n_parts": np.int64(len(parts))} if i == 0 else {}))
    return paths


def with_heads(trunk, seed):
    """A full object-level state dict: ``trunk`` (TRUNK_KEYS) with the colour heads of ``oracle.make_state_dict("object", 0, seed)``.
    The heads enter neither s, S nor sigma."""
    import oracle
    sd = oracle.make_state_dict("object", 0, seed=seed)
    assert set(TRUNK_KEYS) <= set(sd)
    sd.update({k: trunk[k] for k in TRUNK_KEYS})
    return sd


def network(name):
    """(state dict, rays [4096, 11]) of ``bench_coarse`` / ``bench_fine`` (the bench frame's calibrated default-init networks, seeds
    0 / 1), ``trained_coarse`` / ``trained_fine`` (tests/golden/trained_object_chair.npz) or ``default_init_<seed>`` (calibrated the
    same way); (state dict, rays [256, 11]) of ``holdout_{long,sharp}_{coarse,fine}`` (tests/golden/probe_holdout_*.npz: networks the
    margin was not fitted to, their colour heads filled in by ``with_heads``).  Built once per name and left unchanged."""
    if name not in _nets:
        from oracle import calibration as cal
        if name.startswith("holdout_"):
            _, which, lvl = name.split("_")
            fx = holdout_fixture(which)
            trunk = {k: torch.from_numpy(fx[f"w_{lvl}/{k}"]).float() for k in TRUNK_KEYS}
            _nets[name] = (with_heads(trunk, HOLDOUT_SEED[which] + (lvl == "fine")), torch.from_numpy(fx["rays"]).float())
        elif name.startswith("trained_"):
            d = np.load(os.path.join(REPO, "tests", "golden", "trained_object_chair.npz"))
            sd = {k.split("/", 1)[1]: torch.from_numpy(d[k]).float() for k in d.files if k.startswith(f"w_{name[8:]}/")}
            _nets[name] = (sd, torch.from_numpy(d["rays"]).float())
        else:
            if "rays" not in _nets:
                _nets["rays"] = bench_rays()
            seed = {"bench_coarse": 0, "bench_fine": 1}.get(name)
            seed = int(name.rsplit("_", 1)[1]) if seed is None else seed
            _nets[name] = (cal.calibrated_default_init("object", 0, seed, _nets["rays"]), _nets["rays"])
    return _nets[name]


NETWORKS = ("bench_coarse", "bench_fine", "trained_coarse", "trained_fine", "default_init_2", "default_init_3", "default_init_4")
HOLDOUT_FAMILIES = ("trained", "holdout_long", "holdout_sharp")      # <family>_coarse / <family>_fine: every network that was trained
N_RAYS = 256               # the CPU cases' strided subset of a network's rays


def sample_depths(rays, n_samples, seed):
    """Sorted uniform depths between each ray's near and far."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(rays.shape[0], n_samples, generator=g).sort(-1).values
    return (rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * u).contiguous()


_fine = {}


def family_rays(family):
    """The 256 rays the cases of ``family`` (HOLDOUT_FAMILIES) run on: a strided subset of the trained fixture's 4096, all of a
    hold-out fixture's."""
    rays = network(family + "_fine")[1]
    return rays[:: rays.shape[0] // N_RAYS][:N_RAYS].contiguous()


def fine_depths(family):
    """z_fine [256, 192] of ``family_rays``: the fine pass's own depths - 64 linspace depths and the 128 the coarse network's weights
    resample, which crowd where sigma changes sign.  Stored in a hold-out fixture; for the trained fixture computed once from the
    oracle and kept."""
    if family not in _fine:
        if family.startswith("holdout_"):
            _fine[family] = torch.from_numpy(holdout_fixture(family[8:])["z_fine"]).float()
        else:
            _fine[family] = oracle_fine_depths(network(family + "_coarse")[0], network(family + "_fine")[0], family_rays(family))
    return _fine[family]


def oracle_fine_depths(sd_c, sd_f, rays):
    import oracle
    cfg = oracle.RenderConfig(variant="object", n_samples=64, n_importance=128, white_bkgd=True)
    with torch.no_grad():
        return oracle.render_rays(rays, sd_c, sd_f, cfg, stages=True)["z_fine"].contiguous()


def depth_sets(name):
    """{set name: depths [256, S]} of network ``name`` on ``family_rays``: sorted uniform depths (64 for a coarse network, 192 for a
    fine one), and for a fine network the fine pass's own ``z_fine`` (a coarse network only ever sees its 64 stratified depths)."""
    family, lvl = name.rsplit("_", 1)
    rays = family_rays(family)
    sets = {"uniform": sample_depths(rays, 64 if lvl == "coarse" else 192, seed=7)}
    if lvl == "fine":
        sets["z_fine"] = fine_depths(family)
    return sets


def case_figures(sd, x):
    """What a margin case is judged by, the probe model against the fp64 trunk on points ``x``: r = max |s - sigma| / S, the shares of
    points with sigma > 0 and of culled points, the number of culled points with sigma > 0, the largest scaled activation, and
    whether every value is finite."""
    amax = []
    with torch.no_grad():
        sigma = sigma_fp64(sd, x)
        s, big_s = probe_model(sd, x, amax)
    culled = s < -KAPPA * big_s
    return dict(points=x.shape[0], r=float(((s - sigma).abs() / big_s).max()), positive=float((sigma > 0).double().mean()),
                culled=float(culled.double().mean()), culled_positive=int((culled & (sigma > 0)).sum()), amax=amax[0],
                finite=bool(torch.isfinite(sigma).all() and torch.isfinite(s).all() and torch.isfinite(big_s).all()))


def format_figures(tag, f):
    return (f"{tag}: {f['points']} points, sigma > 0 on {f['positive']:.4f}, culled {f['culled']:.4f}, culled with sigma > 0: {f['culled_positive']}, "
            f"r = {f['r']:.3e}, kappa / r = {KAPPA / f['r']:.2f}, largest scaled activation {f['amax']:.4g}")
