"""Shared by tests/test_gate_probe_cpu.py and tests/test_gate_probe_gpu.py: the density gate's probe restated in
torch, the fp64 trunk it is judged against, and the networks and sample points both tests use."""
import os

import numpy as np
import torch

from conftest import REPO

KAPPA = 2.0 ** -6          # csrc/mlp_f16_t128.hip kProbeKappa
ACT_SCALE = 8.0            # csrc/layout.h kActScale
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


def probe_model(sd, x):
    """(s, S) of the probe kernel: hi weights, activations as f16(8 h) to nearest, one product per MAC.  The kernel accumulates in
    fp32 on the matrix core; here the sums are fp64 - they differ by ~1e-7 of the sum of magnitudes, three orders below the margin."""
    enc = f16(encode(x, torch.float32) * ACT_SCALE).double()
    h = enc
    for i in range(8):
        wh, inv = weight_hi(sd[f"pts_linears.{i}.weight"])
        t = (h @ wh.T) * inv + ACT_SCALE * sd[f"pts_linears.{i}.bias"].double()
        h = f16(torch.relu(t).float()).double()
        if i == SKIP:
            h = torch.cat([enc, h], -1)
    wh, inv = weight_hi(sd["alpha_linear.weight"])
    b = sd["alpha_linear.bias"].double()[0]
    s = (h @ wh[0]) * (inv / ACT_SCALE) + b
    big_s = (h @ wh[0].abs()) * (inv / ACT_SCALE) + b.abs()
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


def network(name):
    """(state dict, rays [4096, 11]) of ``bench_coarse`` / ``bench_fine`` (the bench frame's calibrated default-init networks, seeds
    0 / 1), ``trained_coarse`` / ``trained_fine`` (tests/golden/trained_object_chair.npz) or ``default_init_<seed>`` (calibrated the
    same way).  Built once per name and left unchanged."""
    if name not in _nets:
        from oracle import calibration as cal
        if name.startswith("trained_"):
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


def sample_depths(rays, n_samples, seed):
    """Sorted uniform depths between each ray's near and far."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(rays.shape[0], n_samples, generator=g).sort(-1).values
    return (rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * u).contiguous()
