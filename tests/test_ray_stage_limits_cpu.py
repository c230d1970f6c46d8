"""CPU: the cases of tests/_ray_stage.py are fair - the reference's own fp32 arithmetic (the fp32 oracle, fp32 autograd through it)
stays inside the very bounds the kernels are held to, on every element of every case, nothing left out - and the size limits of
the per-ray stages are enforced by the C ABI before anything is launched (no device is needed, and with one nothing reaches it:
every call below is either rejected or an empty batch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _ray_stage as rs
import oracle
from _cases import assert_maps_close
from conftest import REPO


# ---------------------------------------------------------------------------------------------------------------------
# the cases are fair
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(rs.LAYOUTS))
@pytest.mark.parametrize("s", rs.COMPOSITE_SIZES)
def test_composite_cases_are_fair(s, layout):
    """fp32 oracle and fp32 autograd against fp64, at the kernels' bounds, all rays and elements; the disp cotangent is in every
    case with s >= 64 (every ray's acc is far above the floor) and out at s = 1, where one ray is empty and its disp NaN."""
    for wb in (False, True):
        for with_noise in (False, True):
            case = rs.composite_case(s, layout, wb, with_noise)
            tag = f"s={s} {layout} wb={wb} noise={with_noise}"
            c, gap, feat = rs.LAYOUTS[layout]
            assert case["raw"].shape == (rs.COMPOSITE_RAYS, s, 11 + c + gap + feat)
            want = case["want"]
            assert set(want) == {"rgb", "disp", "acc", "depth", "albedo", "shading", "residual", "weights"} | ({"sem"} if c else set()) | ({"feat"} if feat else set())
            acc = want["acc"]
            if s >= 64:
                assert float(acc.min()) > 0.5, (tag, float(acc.min()))
                assert set(case["cot"]) == set(want), tag
            else:
                assert "disp" not in case["cot"] and set(case["cot"]) == set(want) - {"disp"}, tag
                nan = torch.isnan(want["disp"])
                assert nan.tolist() == [r == rs.DEAD_RAY for r in range(rs.COMPOSITE_RAYS)], tag
                assert float(acc[rs.DEAD_RAY]) == 0.0 and float(acc[~nan].min()) > 0.99, tag
            got, _, d_raw = rs.composite_reference(case["raw"], case["z"], case["d"], case["noise"], layout, wb, torch.float32, cot=case["cot"])
            for k, w in want.items():
                assert_maps_close(got[k].numpy(), w.numpy(), rs.rtol_of(k), rs.ATOL, f"{tag}: fp32 {k}")
            w = case["d_raw"].numpy()
            assert np.isfinite(w).all() and float(np.abs(w).max()) > 0, tag
            assert_maps_close(d_raw.numpy(), w, rs.D_RAW_RTOL, rs.d_raw_atol(w), f"{tag}: fp32 d_raw")
            if gap:
                assert float(np.abs(w[..., rs.gap_channels(layout)]).max()) == 0.0, tag
                # ... and the channels on either side of the gap are alive: the last logit and the first feature channel
                assert float(np.abs(w[..., 11 + c - 1]).max()) > 0 and float(np.abs(w[..., 11 + c + gap]).max()) > 0, tag


def test_nan_case_is_what_it_claims():
    case, cfg = rs.nan_case(), rs.NAN_CASE
    w = case["want"]["weights"]
    ray, smp = cfg["ray"], cfg["sample"]
    assert smp >= 64 and smp < 128 < cfg["s"]                                   # in the second chunk, with a third behind it
    assert bool(torch.isfinite(w[ray, :smp]).all()) and bool(torch.isnan(w[ray, smp:]).all())
    others = [r for r in range(rs.COMPOSITE_RAYS) if r != ray]
    for k, v in case["want"].items():
        assert bool(torch.isnan(v[ray]).all()) or k == "weights", k
        assert bool(torch.isfinite(v[others]).all()), k
    assert bool(torch.isfinite(case["d_raw"][others]).all())


@pytest.mark.parametrize("weights", list(rs.WEIGHT_RANGES))
@pytest.mark.parametrize("n_bins,n_samples", rs.PDF_SHAPES)
def test_sample_pdf_cases_are_fair(n_bins, n_samples, weights):
    for form in rs.U_FORMS:
        case = rs.pdf_case(n_bins, n_samples, weights, form)
        assert case["w"].shape == (rs.SAMPLING_RAYS, n_bins - 1) and case["want"].shape == (rs.SAMPLING_RAYS, n_samples)
        assert float(case["w"].min()) >= rs.WEIGHT_RANGES[weights] and bool(torch.isfinite(case["want"]).all())
        if form != "random":
            assert float(case["u"].flatten()[0]) == 0.0 and (n_samples == 1 or float(case["u"].flatten()[-1]) == 1.0)
        assert_maps_close(rs.pdf_fp32(case).numpy(), case["want"].numpy(), rs.RTOL, rs.ATOL, f"bins={n_bins} n={n_samples} {weights} {form}: fp32 samples")


@pytest.mark.parametrize("weights", list(rs.WEIGHT_RANGES))
@pytest.mark.parametrize("n_coarse,n_importance", rs.FINE_SHAPES)
def test_sample_fine_cases_are_fair(n_coarse, n_importance, weights):
    for form in rs.U_FORMS_FINE:
        case = rs.fine_case(n_coarse, n_importance, weights, form)
        tag = f"coarse={n_coarse} imp={n_importance} {weights} {form}"
        zs = case["z_samples"]
        assert zs.shape == (rs.SAMPLING_RAYS, n_importance) and bool(torch.isfinite(zs).all())
        got = rs.fine_samples(case["z"], case["w"], case["u"], torch.float32)
        assert_maps_close(got.numpy(), zs.numpy(), rs.RTOL, rs.ATOL, f"{tag}: fp32 z_samples")
        assert_maps_close(torch.std(got, -1, unbiased=False).numpy(), case["z_std"].numpy(), rs.RTOL, rs.ATOL, f"{tag}: fp32 z_std")
        if n_importance == 1:
            assert float(case["z_std"].abs().max()) == 0.0
        # which sort the kernel takes: ascending u gives ascending samples (the merge), random u does not (the rank sort)
        ascending = bool((got[:, 1:] >= got[:, :-1]).all())
        assert ascending == (form != "random" or n_importance == 1), tag
        if form == "ties" and n_importance > 2:
            assert int((got[:, 1:] == got[:, :-1]).sum()) >= rs.SAMPLING_RAYS * (n_importance // 8), tag


def test_grid_stride_cases_pass_the_caps():
    assert rs.COARSE_STRIDE_RAYS * rs.COARSE_STRIDE_SAMPLES > rs.COARSE_GRID_CAP * rs.BLOCK
    assert rs.FRAME_ELEMENTS == rs.FRAME_GRID_CAP * rs.BLOCK + 1
    src = open(os.path.join(REPO, "intrinsicnerf_amd", "csrc", "ray_ops.hip")).read()
    assert f"if (blocks > {rs.COARSE_GRID_CAP}) blocks = {rs.COARSE_GRID_CAP};" in src
    src = open(os.path.join(REPO, "intrinsicnerf_amd", "csrc", "frame_ops.hip")).read()
    assert f"if (blocks > {rs.FRAME_GRID_CAP}) blocks = {rs.FRAME_GRID_CAP};" in src
    x = rs.frame_values()
    assert int((x < 0).sum()) > 1000 and int((x > 1).sum()) > 1000 and float(x[-1]) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the limits, through the C ABI, with nothing launched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi


FAKE = 0x1000                        # a non-null pointer that is never dereferenced: every call it goes into is turned away


def test_limit_constants_come_from_the_header(capi):
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define INERF_(MAX_SAMPLES|MIN_COARSE|MAX_COARSE|MIN_BINS|MAX_IMPORTANCE)\s+(\d+)", text)}
    assert header == {"MAX_SAMPLES": 1024, "MIN_COARSE": 3, "MAX_COARSE": 256, "MIN_BINS": 2, "MAX_IMPORTANCE": 512}
    assert header == {k: getattr(capi, k) for k in header}
    # the kernels and the whole-path entry take them from there: no second statement of the numbers
    for name in ("ray_ops.hip", "api.cpp"):
        src = open(os.path.join(REPO, "intrinsicnerf_amd", "csrc", name)).read()
        assert "INERF_MAX_SAMPLES" in src and "INERF_MAX_COARSE" in src and "INERF_MAX_IMPORTANCE" in src
        code = re.sub(r"//.*", "", src)
        assert not re.search(r"\b(1024|1025|512|513|257)\b", code), name
    for fn in ("inerf_composite", "inerf_sample_fine", "inerf_sample_pdf", "inerf_render_rays"):           # ... and the header states them at each call
        decl = text.index(f"int {fn}(")
        assert "Limits" in text[max(0, decl - 2000):decl], fn


def test_stage_limits_are_rejected_before_a_launch(capi):
    """One beyond each limit: INERF_E_UNSUPPORTED with non-null pointers (never dereferenced) - and for an empty batch, where the
    last supported size is INERF_OK: it got past the checks, and an empty batch launches nothing."""
    lib, U, OK = capi.lib(), capi.E_UNSUPPORTED, capi.OK
    co = capi.CompositeOut(**{k: FAKE for k in ("rgb", "disp", "acc", "depth", "albedo", "shading", "residual", "weights")})
    p = C.c_void_p(FAKE)

    def composite(n, s):
        return lib.inerf_composite(p, p, p, 3, None, n, s, 11, 0, 0, 0, C.byref(co), None)

    def backward(n, s):
        return lib.inerf_composite_backward(p, p, p, 3, None, n, s, 11, 0, 0, 0, C.byref(co), p, None)

    def fine(n, sc, ni):
        return lib.inerf_sample_fine(p, p, p, n, sc, ni, 0, p, p, p, None)

    def pdf(n, nb, ns):
        return lib.inerf_sample_pdf(p, p, p, n, nb, ns, 0, p, None)

    for n in (4, 0):
        assert composite(n, capi.MAX_SAMPLES + 1) == U and backward(n, capi.MAX_SAMPLES + 1) == U
        assert fine(n, capi.MIN_COARSE - 1, 128) == U and fine(n, capi.MAX_COARSE + 1, 128) == U
        assert fine(n, 64, capi.MAX_IMPORTANCE + 1) == U and fine(n, 64, 0) == U
        assert pdf(n, capi.MIN_BINS - 1, 128) == U and pdf(n, capi.MAX_COARSE + 1, 128) == U
        assert pdf(n, 63, capi.MAX_IMPORTANCE + 1) == U and pdf(n, 63, 0) == U
    # the last supported sizes
    assert composite(0, capi.MAX_SAMPLES) == OK and backward(0, capi.MAX_SAMPLES) == OK and composite(0, 1) == OK
    assert fine(0, capi.MIN_COARSE, 1) == OK and fine(0, capi.MAX_COARSE, capi.MAX_IMPORTANCE) == OK
    assert pdf(0, capi.MIN_BINS, 1) == OK and pdf(0, capi.MAX_COARSE, capi.MAX_IMPORTANCE) == OK
    # the INERF_E_INVALID cases stay what they were (test_capi_cpu.test_argument_validation): a null pointer at a supported size
    I = capi.E_INVALID
    assert lib.inerf_sample_fine(None, None, None, 4, 64, 128, 0, None, None, None, None) == I
    assert lib.inerf_sample_pdf(None, None, None, 4, 63, 128, 0, None, None) == I
    assert lib.inerf_composite(None, None, None, 3, None, 4, 64, 11, 0, 0, 0, C.byref(capi.CompositeOut()), None) == I
    assert lib.inerf_composite_backward(None, None, None, 3, None, 4, 64, 11, 0, 0, 0, C.byref(capi.CompositeOut()), None, None) == I
    assert composite(4, 0) == I and backward(4, 0) == I
    assert lib.inerf_composite(p, p, p, 2, None, 4, 64, 11, 0, 0, 0, C.byref(co), None) == I                 # direction stride below 3
    assert lib.inerf_composite(p, p, p, 3, None, 4, 64, 11, 1, 0, 0, C.byref(co), None) == I                 # more channels asked for than raw has
    assert lib.inerf_composite(p, p, p, 3, None, 0, 64, 11, 0, 0, 0, None, None) == I                         # no output struct
    for rc in (lib.inerf_sample_pdf(None, None, None, 0, 63, 128, 0, None, None), lib.inerf_sample_fine(None, None, None, 0, 64, 128, 0, None, None, None, None)):
        assert rc == OK


def _render_args(capi, n_rays, n_samples, n_importance):
    a = capi.RenderArgs()
    a.net = capi.net_desc(capi.VARIANT_OBJECT, 0, 10, 4, 1.0)
    a.packed_coarse = a.rays = a.t_vals = a.u = FAKE
    a.n_rays, a.n_samples, a.n_importance = n_rays, n_samples, n_importance
    a.workspace, a.workspace_bytes = FAKE, 1 << 62
    return a


@pytest.mark.parametrize("n_samples,n_importance", [(1025, 0), (257, 128), (64, 513), (2, 128)])
def test_render_rays_validates_sizes_before_it_launches(capi, n_samples, n_importance):
    """A workspace that is large enough and non-null pointers everywhere: without the up-front check the coarse pass would be
    enqueued (and the call fail some other way where there is no device) before inerf_sample_fine / inerf_composite reports the size."""
    lib = capi.lib()
    for n_rays in (4, 0):
        assert lib.inerf_render_rays(C.byref(_render_args(capi, n_rays, n_samples, n_importance)), None) == capi.E_UNSUPPORTED
    # the checks before it keep their answers
    a = _render_args(capi, 4, n_samples, n_importance)
    a.rays = None
    assert lib.inerf_render_rays(C.byref(a), None) == capi.E_INVALID
    if n_importance > 0:
        a = _render_args(capi, 4, n_samples, n_importance)
        a.u = None
        assert lib.inerf_render_rays(C.byref(a), None) == capi.E_INVALID


def test_render_rays_accepts_the_last_supported_sizes(capi):
    lib = capi.lib()
    for n_samples, n_importance in ((1024, 0), (1, 0), (256, 512), (3, 1), (64, 128)):
        assert lib.inerf_render_rays(C.byref(_render_args(capi, 0, n_samples, n_importance)), None) == capi.OK
    # ... and a supported size with too small a workspace is still a workspace error, not a size error
    a = _render_args(capi, 4, 256, 512)
    a.workspace_bytes = 16
    assert lib.inerf_render_rays(C.byref(a), None) == capi.E_WORKSPACE
