"""The per-ray stage kernels (csrc/ray_ops.hip: k_sample_coarse, k_composite, k_composite_bwd, k_sample_fine) at their size
limits: the cases, their fp64 references and the bounds, shared by test_ray_stage_limits_cpu.py (the cases are fair: the
reference's own fp32 arithmetic stays inside the bounds on every element) and test_ray_stage_limits_gpu.py (the kernels do).

Every input comes from a seeded ``torch.Generator`` on the CPU; the references are the oracle's dtype-generic functions on
``.double()`` inputs (``oracle.composite``, ``torch.autograd.grad`` through it, ``oracle.inverse_cdf_sample``,
``oracle.coarse_depths``), computed once per case and left alone.

Input recipe (test_backward_golden.test_composite_backward_randomized_shapes): raw ~ U[0, 1) with raw[..., 3] = 2 randn + 0.3,
z = sort(4 rand + 2), d = randn; sampling weights U[0.5, 1) or U[0, 1); bins sort(4 rand + 2).

Bounds (none of them taken from what the kernels give):
  maps, weights, depths   |got - want| <= 1e-5 + 1e-4 |want| (disp: 5e-4), NaNs at the same places     - test_gpu_parity.py
  d_raw                   |got - want| <= 2e-5 max |want| + 2e-4 |want|                                  - test_backward_golden.py
  z_merged, sample_coarse, to8b: bit for bit."""
import functools

import numpy as np
import torch

import oracle

RTOL, ATOL, RTOL_DISP = 1e-4, 1e-5, 5e-4
D_RAW_RTOL, D_RAW_ATOL_OF_MAX = 2e-4, 2e-5
SENTINEL = -12345.5                  # what the rejection tests fill every output with

MAP_KEYS = ("rgb", "disp", "acc", "depth", "albedo", "shading", "residual", "sem", "feat", "weights")


def rtol_of(key):
    return RTOL_DISP if key == "disp" else RTOL


def worst_ratio(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|) over the elements that are not NaN in ``want`` (0.0 when there is none)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = ~np.isnan(want) & ~np.isnan(got)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / (atol + rtol * np.abs(want[ok]))))


def d_raw_atol(want):
    return D_RAW_ATOL_OF_MAX * float(np.nanmax(np.abs(np.asarray(want, np.float64)))) + 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 1. compositing, forward and backward
# ---------------------------------------------------------------------------------------------------------------------
COMPOSITE_RAYS = 5                   # one whole workgroup of four waves, and one with a single live wave
COMPOSITE_SIZES = (1, 64, 65, 1023, 1024)
# name -> (semantic classes, unused channels between the logits and the feature block, feature width); channels = 11 + sum
LAYOUTS = {"object": (0, 0, 0), "c64": (64, 0, 0), "c65": (65, 0, 0), "c130-gap3-feat128": (130, 3, 128)}
DISP_ACC_FLOOR = 1e-3                # the disp cotangent is used where every ray's fp64 acc is above this
DEAD_RAY = 4                         # s = 1: the one ray with no positive density (acc = 0, disp = NaN)


def layout_channels(layout):
    c, gap, feat = LAYOUTS[layout]
    return 11 + c + gap + feat


def _seed(*parts):
    return int(sum((i + 1) * 1000003 * int(p) for i, p in enumerate(parts)) % (2 ** 31 - 1))


def composite_inputs(s, layout, with_noise, n=COMPOSITE_RAYS):
    """(raw [n, s, ch], z [n, s], d [n, 3], noise [n, s] or None), fp32 on the CPU.  s = 1: the density is forced positive (beyond
    what the noise can undo) on every ray but DEAD_RAY, and negative there."""
    ch = layout_channels(layout)
    g = torch.Generator().manual_seed(_seed(s, ch, 7))
    raw = torch.rand(n, s, ch, generator=g)
    raw[..., 3] = torch.randn(n, s, generator=g) * 2 + 0.3
    z = torch.sort(torch.rand(n, s, generator=g) * 4 + 2, -1)[0]
    d = torch.randn(n, 3, generator=g)
    noise = torch.randn(n, s, generator=g) * 0.3
    if s == 1:
        raw[..., 3] = raw[..., 3].abs() + 3.0
        raw[DEAD_RAY, :, 3] = -5.0
        noise = noise.clamp(-1.0, 1.0)
    return raw, z.contiguous(), d, (noise if with_noise else None)


def composite_config(layout, white_bkgd):
    c, _, feat = LAYOUTS[layout]
    assert feat in (0, oracle.intrinsic_render.ENDPOINT_DIM)
    return oracle.RenderConfig(variant="ssr" if c > 0 else "object", white_bkgd=white_bkgd, n_classes=c, endpoint_feat=feat > 0)


def composite_reference(raw, z, d, noise, layout, white_bkgd, dtype, cot=None):
    """(maps, cotangents, d_raw) of ``oracle.composite`` evaluated in ``dtype`` with autograd through it: the cotangents are drawn
    here (fp32 randn on every output, disp only where every ray's acc is above DISP_ACC_FLOOR) unless ``cot`` hands them in."""
    feat = LAYOUTS[layout][2] > 0
    r = raw.to(dtype).clone().requires_grad_(True)
    out = oracle.composite(r, z.to(dtype), d.to(dtype), composite_config(layout, white_bkgd), None if noise is None else noise.to(dtype), feat=feat)
    out = {k: out[k] for k in MAP_KEYS if out.get(k) is not None}
    if cot is None:
        g = torch.Generator().manual_seed(_seed(raw.shape[1], raw.shape[2], 11))
        cot = {k: torch.randn(out[k].shape, generator=g) for k in out}           # (drawn for every output: the same stream in every case)
        if not bool((out["acc"] > DISP_ACC_FLOOR).all()):
            del cot["disp"]
    (d_raw,) = torch.autograd.grad(sum((cot[k].to(dtype) * out[k]).sum() for k in cot), r)
    return {k: v.detach() for k, v in out.items()}, cot, d_raw


@functools.lru_cache(maxsize=None)
def composite_case(s, layout, white_bkgd, with_noise):
    """One case, computed once: dict with the fp32 inputs, the fp64 maps ``want``, the cotangents ``cot`` and the fp64 ``d_raw``."""
    raw, z, d, noise = composite_inputs(s, layout, with_noise)
    want, cot, d_raw = composite_reference(raw, z, d, noise, layout, white_bkgd, torch.float64)
    return {"raw": raw, "z": z, "d": d, "noise": noise, "want": want, "cot": cot, "d_raw": d_raw}


def gap_channels(layout):
    c, gap, feat = LAYOUTS[layout]
    return slice(11 + c, 11 + c + gap)


# 2. a NaN density in the second chunk of one ray
NAN_CASE = dict(s=130, layout="c65", white_bkgd=True, ray=1, sample=70)


@functools.lru_cache(maxsize=None)
def nan_case():
    raw, z, d, _ = composite_inputs(NAN_CASE["s"], NAN_CASE["layout"], False)
    raw = raw.clone()
    raw[NAN_CASE["ray"], NAN_CASE["sample"], 3] = float("nan")
    want, cot, d_raw = composite_reference(raw, z, d, None, NAN_CASE["layout"], NAN_CASE["white_bkgd"], torch.float64)
    return {"raw": raw, "z": z, "d": d, "want": want, "cot": cot, "d_raw": d_raw}


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. sample_pdf and sample_fine
# ---------------------------------------------------------------------------------------------------------------------
SAMPLING_RAYS = 7                    # one whole workgroup and one with three live waves
PDF_SHAPES = ((2, 1), (3, 7), (65, 64), (66, 65), (67, 63), (256, 512))              # (n_bins, n_samples): 1, 2, 64, 65, 66, 255 weights
FINE_SHAPES = ((3, 1), (66, 64), (67, 65), (68, 63), (256, 512))                     # (n_coarse, n_importance): 1, 64, 65, 66, 254 weights
WEIGHT_RANGES = {"w05": 0.5, "w01": 0.0}                                             # weights ~ U[lo, 1)
U_FORMS = ("shared", "per-ray", "random")
U_FORMS_FINE = U_FORMS + ("ties",)


def u_of(form, n, n_samples, g):
    """shared: linspace(0, 1, n) with both ends, [n_samples]; per-ray: the same handed in as [n, n_samples]; random: U[0, 1) per ray;
    ties: the shared linspace with a run of equal values (ascending: the merge path of k_sample_fine, with ties)."""
    lin = torch.linspace(0.0, 1.0, n_samples)
    if form == "shared":
        return lin
    if form == "per-ray":
        return lin.expand(n, n_samples).contiguous()
    if form == "random":
        return torch.rand(n, n_samples, generator=g)
    a, b = n_samples * 5 // 16, n_samples * 15 // 32
    lin = lin.clone()
    lin[a:b] = lin[a] if b > a else lin[a:b]
    return lin


def _expanded(u, n):
    return (u if u.dim() == 2 else u.expand(n, u.shape[0])).contiguous()


@functools.lru_cache(maxsize=None)
def pdf_case(n_bins, n_samples, weights, form, n=SAMPLING_RAYS):
    g = torch.Generator().manual_seed(_seed(n_bins, n_samples, 13))
    bins = torch.sort(torch.rand(n, n_bins, generator=g) * 4 + 2, -1)[0].contiguous()
    lo = WEIGHT_RANGES[weights]
    w = (torch.rand(n, n_bins - 1, generator=g) * (1.0 - lo) + lo).contiguous()
    u = u_of(form, n, n_samples, g)
    want = oracle.inverse_cdf_sample(bins.double(), w.double(), _expanded(u, n).double())
    return {"bins": bins, "w": w, "u": u, "want": want}


def pdf_fp32(case):
    return oracle.inverse_cdf_sample(case["bins"], case["w"], _expanded(case["u"], case["bins"].shape[0]))


@functools.lru_cache(maxsize=None)
def fine_case(n_coarse, n_importance, weights, form, n=SAMPLING_RAYS):
    g = torch.Generator().manual_seed(_seed(n_coarse, n_importance, 17))
    z = torch.sort(torch.rand(n, n_coarse, generator=g) * 4 + 2, -1)[0].contiguous()
    lo = WEIGHT_RANGES[weights]
    w = (torch.rand(n, n_coarse, generator=g) * (1.0 - lo) + lo).contiguous()           # the FULL coarse weights: the kernel drops both ends
    u = u_of(form, n, n_importance, g)
    zs = fine_samples(z, w, u, torch.float64)
    return {"z": z, "w": w, "u": u, "z_samples": zs, "z_std": torch.std(zs, -1, unbiased=False)}


def fine_samples(z, w, u, dtype):
    """z_mid + sample_pdf over weights[1:-1] (run_nerf.py:499-501) in ``dtype``."""
    z, w = z.to(dtype), w.to(dtype)
    mid = 0.5 * (z[:, 1:] + z[:, :-1])
    return oracle.inverse_cdf_sample(mid, w[:, 1:-1], _expanded(u, z.shape[0]).to(dtype))


# ---------------------------------------------------------------------------------------------------------------------
# 5. grid-stride caps
# ---------------------------------------------------------------------------------------------------------------------
COARSE_GRID_CAP, FRAME_GRID_CAP, BLOCK = 8192, 4096, 256
COARSE_STRIDE_RAYS, COARSE_STRIDE_SAMPLES = 2049, 1024          # 2049 x 1024 = 8192 x 256 + 1024 elements: a second trip for 1024 threads
FRAME_ELEMENTS = FRAME_GRID_CAP * BLOCK + 1                     # one element into the second trip


def coarse_rays(n, seed=1):
    """[n, 11] rays with near in [0.5, 1.5) and far 1 to 6 beyond it (test_gpu_parity.test_sample_coarse_bit_exact)."""
    g = torch.Generator().manual_seed(seed)
    rays = torch.randn(n, 11, generator=g)
    rays[:, 6] = torch.rand(n, generator=g) + 0.5
    rays[:, 7] = rays[:, 6] + torch.rand(n, generator=g) * 5 + 1
    return rays, g


def frame_values():
    """FRAME_ELEMENTS values in [-0.5, 1.5) - a quarter clipped on either side - the last one 1.0 (-> 255)."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(FRAME_ELEMENTS, generator=g) * 2 - 0.5
    x[-1] = 1.0
    return x
