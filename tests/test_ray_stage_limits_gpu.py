"""The per-ray stage kernels of csrc/ray_ops.hip at their size limits against fp64 (cases, references and bounds: tests/_ray_stage.py;
that the cases are fair: test_ray_stage_limits_cpu.py): compositing forward and backward over 1 .. 16 chunks of 64 samples and
over 64, 65 and 130 semantic classes with a channel gap before the feature block; a NaN density in the second chunk; the cdf scan of
k_sample_fine with 1 .. 255 weights, its merge and its rank sort at 768 elements; the second trip of the grid-stride loops of
k_sample_coarse and k_frame_to_u8; and one size beyond every limit, which must be turned away with nothing written.

Every figure the module prints starts with "ray_stage |": the worst err / bound per output and case, bound = the plain tolerances of
test_gpu_parity.py (1e-5 + 1e-4 |want|; disp 5e-4) and test_backward_golden.py (d_raw: 2e-5 max |want| + 2e-4 |want|).

Worst figures on an MI355X, err / bound (profiles/ray_stage_limits.txt has every line the module prints; 47 tests, 1.6 s):
  composite forward   0.021 (feat, s = 1023, 272 channels), 0.020 (sem, 65 classes), at most 0.0082 in every other output (weights)
  composite backward  d_raw 0.029 (s = 1024, 11 channels); unused channels exactly 0 in all 20 cases of that layout
  NaN density         the other rays: forward 0.0050 (sem), backward 0.0044; NaN positions the oracle's
  sample_pdf          0.016 (256 bins, 512 random u, weights in [0, 1))
  sample_fine         z_samples 0.010 (66 + 64, weights in [0, 1)), z_std 0.0020; z_merged bit for bit in all 42 checks
  sample_coarse       0 of 2 098 176 depths differ in each of the four forms; to8b: 0 of 1 048 577 values differ
No sampling case needed the CDF_NOISE x sample_pdf_sensitivity term of test_gpu_parity.py: the plain tolerance holds with a factor
of 60 to spare.
"""
import numpy as np
import pytest
import torch

import _ray_stage as rs
import oracle
from _cases import assert_maps_close

pytestmark = pytest.mark.gpu
TAG = "ray_stage |"
DEV = "cuda:0"


def _to(t):
    return None if t is None else t.to(DEV)


def _ratios(pairs):
    """'key ratio' for every (key, got, want, rtol, atol), worst err / bound over the elements that are numbers in both."""
    return ", ".join(f"{k} {rs.worst_ratio(g, w, rt, at):.3g}" for k, g, w, rt, at in pairs)


def _judge(pairs, tag, problems):
    for k, g, w, rt, at in pairs:
        try:
            assert_maps_close(g, w, rt, at, f"{tag}: {k}")
        except AssertionError as e:
            problems.append(str(e))


# ---------------------------------------------------------------------------------------------------------------------
# 1. compositing forward and backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(rs.LAYOUTS))
@pytest.mark.parametrize("s", rs.COMPOSITE_SIZES)
def test_composite_forward_and_backward_vs_fp64(s, layout):
    """5 rays (a whole workgroup and one with a single live wave) x s samples, white background and noise on and off: every output of
    the forward, ``weights`` included, and d_raw for cotangents on all outputs (disp where every ray's fp64 acc > 1e-3: every case with
    s >= 64) against fp64; the unused channels between the logits and the feature block get a d_raw of exactly 0; at s = 1 the one ray
    without positive density has disp = NaN, as the oracle's has."""
    from intrinsicnerf_amd import kernels
    print()
    c, gap, feat = rs.LAYOUTS[layout]
    problems = []
    for wb in (False, True):
        for with_noise in (False, True):
            case = rs.composite_case(s, layout, wb, with_noise)
            tag = f"composite s={s} {layout} wb={int(wb)} noise={int(with_noise)}"
            raw, z, d, noise = (_to(case[k]) for k in ("raw", "z", "d", "noise"))
            out = kernels.composite(raw, z, d, noise, wb, n_classes=c, feat_dim=feat)
            assert set(out) == set(case["want"]), tag
            pairs = [(k, out[k].cpu().numpy(), w.numpy(), rs.rtol_of(k), rs.ATOL) for k, w in case["want"].items()]
            print(f"{TAG} {tag} forward: {_ratios(pairs)}")
            _judge(pairs, tag, problems)
            if s == 1:
                assert bool(torch.isnan(out["disp"][rs.DEAD_RAY])) and float(out["acc"][rs.DEAD_RAY]) == 0.0, tag
            assert ("disp" in case["cot"]) == (s >= 64), tag
            got = kernels.composite_backward(raw, z, d, {k: _to(v) for k, v in case["cot"].items()}, noise, wb, c, feat).cpu().numpy()
            want = case["d_raw"].numpy()
            pairs = [("d_raw", got, want, rs.D_RAW_RTOL, rs.d_raw_atol(want))]
            print(f"{TAG} {tag} backward ({len(case['cot'])} cotangents): {_ratios(pairs)}")
            _judge(pairs, tag, problems)
            if gap and not float(np.abs(got[..., rs.gap_channels(layout)]).max()) == 0.0:
                problems.append(f"{tag}: d_raw of the unused channels is not exactly 0")
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# 2. a NaN density in the second chunk
# ---------------------------------------------------------------------------------------------------------------------
def test_nan_density_in_the_second_chunk_stays_in_its_ray():
    """s = 130, raw[1, 70, 3] = NaN: the NaN pattern of every output is the fp64 oracle's - weights finite before sample 70 and NaN from
    it on, through the carry into the third chunk - and the other four rays (three of them in the same workgroup, beside it in the
    shared LDS arrays) stay inside the plain tolerance, forward and backward."""
    from intrinsicnerf_amd import kernels
    print()
    case, cfg = rs.nan_case(), rs.NAN_CASE
    c, gap, feat = rs.LAYOUTS[cfg["layout"]]
    raw, z, d = (_to(case[k]) for k in ("raw", "z", "d"))
    out = kernels.composite(raw, z, d, None, cfg["white_bkgd"], n_classes=c, feat_dim=feat)
    pairs = [(k, out[k].cpu().numpy(), w.numpy(), rs.rtol_of(k), rs.ATOL) for k, w in case["want"].items()]
    print(f"{TAG} nan-density forward: {_ratios(pairs)}")
    problems = []
    _judge(pairs, "nan-density", problems)                     # (NaN positions must be equal: assert_maps_close)
    w = out["weights"][cfg["ray"]].cpu()
    assert bool(torch.isfinite(w[:cfg["sample"]]).all()) and bool(torch.isnan(w[cfg["sample"]:]).all())
    others = [r for r in range(rs.COMPOSITE_RAYS) if r != cfg["ray"]]
    got = kernels.composite_backward(raw, z, d, {k: _to(v) for k, v in case["cot"].items()}, None, cfg["white_bkgd"], c, feat).cpu().numpy()
    want = case["d_raw"].numpy()
    pairs = [("d_raw of the other rays", got[others], want[others], rs.D_RAW_RTOL, rs.d_raw_atol(want[others]))]
    print(f"{TAG} nan-density backward: {_ratios(pairs)}")
    _judge(pairs, "nan-density", problems)
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# 3. sample_pdf   4. sample_fine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", list(rs.WEIGHT_RANGES))
@pytest.mark.parametrize("n_bins,n_samples", rs.PDF_SHAPES)
def test_sample_pdf_vs_fp64(n_bins, n_samples, weights):
    """The stand-alone sampler (k_sample_fine<true>) with 1, 2, 64, 65, 66 and 255 weights - the cdf scan's carry is used from 65 on -
    for u = linspace with both ends (shared and per ray) and random u, 7 rays: plain tolerance, no sensitivity term."""
    from intrinsicnerf_amd import kernels
    print()
    problems = []
    for form in rs.U_FORMS:
        case = rs.pdf_case(n_bins, n_samples, weights, form)
        tag = f"sample_pdf bins={n_bins} n={n_samples} {weights} u={form}"
        got = kernels.sample_pdf(_to(case["bins"]), _to(case["w"]), _to(case["u"]), n_samples).cpu().numpy()
        pairs = [("samples", got, case["want"].numpy(), rs.RTOL, rs.ATOL)]
        print(f"{TAG} {tag}: {_ratios(pairs)}")
        _judge(pairs, tag, problems)
    assert not problems, "; ".join(problems)


def _check_fine(case, tag, problems, n_importance):
    from intrinsicnerf_amd import kernels
    z = _to(case["z"])
    zs, zm, zstd = kernels.sample_fine(z, _to(case["w"]), _to(case["u"]), n_importance)
    zs, zm, zstd = zs.cpu(), zm.cpu(), zstd.cpu()
    pairs = [("z_samples", zs.numpy(), case["z_samples"].numpy(), rs.RTOL, rs.ATOL), ("z_std", zstd.numpy(), case["z_std"].numpy(), rs.RTOL, rs.ATOL)]
    merged = torch.sort(torch.cat([case["z"], zs], -1), -1)[0]
    same = torch.equal(torch.nan_to_num(zm, nan=-1.0), torch.nan_to_num(merged, nan=-1.0)) and torch.equal(torch.isnan(zm), torch.isnan(merged))
    print(f"{TAG} {tag}: {_ratios(pairs)}, z_merged {'bit-exact' if same else 'DIFFERS'}")
    _judge(pairs, tag, problems)
    if not same:
        problems.append(f"{tag}: z_merged is not sort(cat(z_coarse, z_samples)) bit for bit ({int((zm != merged).sum())} of {zm.numel()} differ)")
    return zs, zm, zstd


@pytest.mark.parametrize("weights", list(rs.WEIGHT_RANGES))
@pytest.mark.parametrize("n_coarse,n_importance", rs.FINE_SHAPES)
def test_sample_fine_vs_fp64(n_coarse, n_importance, weights):
    """k_sample_fine<false> with 1, 64, 65, 66 and 254 pdf weights: z_samples against the fp64 inverse cdf over the mid-points and
    weights[1:-1], z_std against the fp64 population std (exactly 0 for one sample), z_merged bit for bit the sort of its own inputs -
    by the merge for ascending u (shared, per ray, with a run of ties) and by the rank sort for random u, up to 256 + 512 elements."""
    print()
    problems = []
    for form in rs.U_FORMS_FINE:
        case = rs.fine_case(n_coarse, n_importance, weights, form)
        tag = f"sample_fine coarse={n_coarse} imp={n_importance} {weights} u={form}"
        zs, zm, zstd = _check_fine(case, tag, problems, n_importance)
        if n_importance == 1 and not float(zstd.abs().max()) == 0.0:
            problems.append(f"{tag}: z_std of a single sample is {float(zstd.abs().max())!r}, not 0")
    assert not problems, "; ".join(problems)


def test_sample_fine_nan_depth_at_the_largest_size():
    """A NaN among the 256 coarse depths of one ray (with 512 new samples: the rank sort over 768 elements, NaNs last): the merged row
    is still the sort of its own inputs, the other six rays stay inside the plain tolerance."""
    from intrinsicnerf_amd import kernels
    print()
    case = dict(rs.fine_case(256, 512, "w05", "shared"))
    ray = 5
    case["z"] = case["z"].clone()
    case["z"][ray, 7] = float("nan")
    zs64 = rs.fine_samples(case["z"], case["w"], case["u"], torch.float64)
    others = [r for r in range(rs.SAMPLING_RAYS) if r != ray]
    assert torch.equal(zs64[others], case["z_samples"][others]) and bool(torch.isnan(zs64[ray]).any())
    z = _to(case["z"])
    zs, zm, zstd = (t.cpu() for t in kernels.sample_fine(z, _to(case["w"]), _to(case["u"]), 512))
    merged = torch.sort(torch.cat([case["z"], zs], -1), -1)[0]
    assert torch.equal(torch.isnan(zm), torch.isnan(merged)) and int(torch.isnan(zm[ray]).sum()) >= 1
    assert torch.equal(torch.nan_to_num(zm, nan=-1.0), torch.nan_to_num(merged, nan=-1.0))
    assert torch.equal(torch.isnan(zs), torch.isnan(zs64))
    pairs = [("z_samples of the other rays", zs[others].numpy(), zs64[others].numpy(), rs.RTOL, rs.ATOL),
             ("z_std of the other rays", zstd[others].numpy(), case["z_std"][others].numpy(), rs.RTOL, rs.ATOL)]
    print(f"{TAG} sample_fine coarse=256 imp=512 NaN depth: {_ratios(pairs)}, z_merged bit-exact")
    problems = []
    _judge(pairs, "NaN depth", problems)
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# 5. grid-stride caps
# ---------------------------------------------------------------------------------------------------------------------
def test_sample_coarse_beyond_the_grid_cap_is_bit_exact():
    """2049 rays x 1024 samples = 8192 x 256 + 1024 elements: the last 1024 are the second trip of the stride loop.  Bit for bit the
    fp32 oracle, with and without jitter and lindisp.  And 1 and 2 samples per ray with jitter: a lone sample has lower = upper = z."""
    from intrinsicnerf_amd import kernels
    print()
    n, s = rs.COARSE_STRIDE_RAYS, rs.COARSE_STRIDE_SAMPLES
    rays, g = rs.coarse_rays(n)
    t = torch.linspace(0., 1., s)
    tr = torch.rand(n, s, generator=g)
    rays_dev, t_dev, tr_dev = _to(rays), _to(t), _to(tr)
    for lindisp in (False, True):
        for t_rand, t_rand_dev in ((None, None), (tr, tr_dev)):
            want = oracle.coarse_depths(rays[:, 6:7], rays[:, 7:8], t, lindisp, t_rand)
            got = kernels.sample_coarse(rays_dev, t_dev, t_rand_dev, lindisp).cpu()
            differ = int((got != want).sum())
            first = rs.COARSE_GRID_CAP * rs.BLOCK
            second_trip = int((got.flatten()[first:] != want.flatten()[first:]).sum())
            print(f"{TAG} sample_coarse {n}x{s} lindisp={int(lindisp)} jitter={int(t_rand is not None)}: {differ} of {got.numel()} differ, "
                  f"{second_trip} of {got.numel() - first} in the second trip")
            assert torch.equal(got, want), f"lindisp={lindisp} jitter={t_rand is not None}: {differ} differ ({second_trip} in the second trip)"
    rays5, g = rs.coarse_rays(5, seed=2)
    for s in (1, 2):
        t, tr = torch.linspace(0., 1., s), torch.rand(5, s, generator=g)
        for lindisp in (False, True):
            want = oracle.coarse_depths(rays5[:, 6:7], rays5[:, 7:8], t, lindisp, tr)
            got = kernels.sample_coarse(_to(rays5), _to(t), _to(tr), lindisp).cpu()
            assert torch.equal(got, want), f"s={s} lindisp={lindisp}"
            if s == 1:
                assert torch.equal(got, kernels.sample_coarse(_to(rays5), _to(t), None, lindisp).cpu())
    print(f"{TAG} sample_coarse 5x1 and 5x2 with jitter: bit-exact")


def test_to8b_beyond_the_grid_cap():
    """4096 x 256 + 1 values: the last one is the second trip of k_frame_to_u8's stride loop."""
    from intrinsicnerf_amd import frames
    print()
    x = rs.frame_values()
    want = (255 * np.clip(x.numpy(), 0, 1)).astype(np.uint8)
    got = frames.to8b(_to(x)).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    print(f"{TAG} to8b {x.numel()} values: {int((got != want).sum())} differ, last {int(got[-1])}")
    assert np.array_equal(got, want) and int(got[-1]) == 255


# ---------------------------------------------------------------------------------------------------------------------
# 6. one beyond each limit, through the wrappers
# ---------------------------------------------------------------------------------------------------------------------
def _rejected(monkeypatch, call):
    """``call()`` must raise what _capi.check raises for E_UNSUPPORTED, and leave every output tensor the wrapper allocated - handed
    out pre-filled with a sentinel here - untouched."""
    from intrinsicnerf_amd import _capi, kernels
    handed = []

    def filled(like, *shape):
        t = torch.full(shape, rs.SENTINEL, dtype=torch.float32, device=like.device)
        handed.append(t)
        return t

    with monkeypatch.context() as m:
        m.setattr(kernels, "_new", filled)
        with pytest.raises(RuntimeError) as e:
            call()
    with pytest.raises(RuntimeError) as ref:
        _capi.check(_capi.E_UNSUPPORTED, "x")
    assert str(e.value).split(": ", 1)[1] == str(ref.value).split(": ", 1)[1], str(e.value)
    torch.cuda.synchronize()
    assert handed and all(bool((t == rs.SENTINEL).all()) for t in handed), "a rejected call wrote to its outputs"
    return len(handed)


def test_sizes_beyond_the_limits_are_rejected_through_the_wrappers(monkeypatch):
    from intrinsicnerf_amd import kernels
    print()
    g = torch.Generator().manual_seed(3)
    n = 5
    big = rs.composite_inputs(1025, "object", False)
    raw, z, d = (_to(t) for t in big[:3])
    assert raw.shape == (n, 1025, 11)
    counts = {}
    counts["composite s=1025"] = _rejected(monkeypatch, lambda: kernels.composite(raw, z, d))
    cot = {"rgb": torch.ones(n, 3, device=DEV), "weights": torch.ones(n, 1025, device=DEV)}
    counts["composite_backward s=1025"] = _rejected(monkeypatch, lambda: kernels.composite_backward(raw, z, d, cot))
    for sc, ni in ((2, 128), (257, 128), (64, 513)):
        zc = _to(torch.sort(torch.rand(n, sc, generator=g) * 4 + 2, -1)[0].contiguous())
        w, u = _to(torch.rand(n, sc, generator=g)), torch.linspace(0., 1., ni, device=DEV)
        counts[f"sample_fine coarse={sc} imp={ni}"] = _rejected(monkeypatch, lambda: kernels.sample_fine(zc, w, u, ni))
    for nb in (1, 257):
        bins = _to(torch.sort(torch.rand(n, nb, generator=g) * 4 + 2, -1)[0].contiguous())
        w, u = _to(torch.rand(n, nb - 1, generator=g)), torch.linspace(0., 1., 128, device=DEV)
        counts[f"sample_pdf bins={nb}"] = _rejected(monkeypatch, lambda: kernels.sample_pdf(bins, w, u, 128))
    print(f"{TAG} rejected, outputs untouched: " + ", ".join(f"{k} ({v} tensors)" for k, v in counts.items()))
    # ... and the calls that follow are served as if nothing had happened
    problems = []
    case = rs.composite_case(65, "object", False, False)
    raw, z, d = (_to(case[k]) for k in ("raw", "z", "d"))
    out = kernels.composite(raw, z, d)
    pairs = [(k, out[k].cpu().numpy(), w.numpy(), rs.rtol_of(k), rs.ATOL) for k, w in case["want"].items()]
    got = kernels.composite_backward(raw, z, d, {k: _to(v) for k, v in case["cot"].items()}).cpu().numpy()
    pairs.append(("d_raw", got, case["d_raw"].numpy(), rs.D_RAW_RTOL, rs.d_raw_atol(case["d_raw"].numpy())))
    _judge(pairs, "composite after the rejections", problems)
    _check_fine(rs.fine_case(66, 64, "w05", "shared"), "sample_fine after the rejections", problems, 64)
    case = rs.pdf_case(65, 64, "w05", "shared")
    got = kernels.sample_pdf(_to(case["bins"]), _to(case["w"]), _to(case["u"]), 64).cpu().numpy()
    _judge([("samples", got, case["want"].numpy(), rs.RTOL, rs.ATOL)], "sample_pdf after the rejections", problems)
    assert not problems, "; ".join(problems)
