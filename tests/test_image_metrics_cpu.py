"""Intrinsic-image metrics without a device: the yardstick itself (_image_metrics.py) against scipy and closed forms, the host
finishing of ``intrinsicnerf_amd.evaluation`` fed the yardstick's moments, the C entry points' argument checks through the built
library, and the fairness of the LMSE cases the GPU tests use (no window's sum of p^2 lies near the 1e-5 branch: the cap on windows
left out is zero)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _image_metrics as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi


def test_header_binding_and_names_agree(capi):
    with open(os.path.join(REPO, "include", "inerf.h")) as fh:
        text = fh.read()
    header = int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1))
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version() and header >= 40023
    for name in ("inerf_image_quality", "inerf_image_quality_workspace_bytes"):
        assert name in capi.SYMBOLS and re.search(r"\b%s\(" % name, text)
    assert capi.IMQ_SUM_NAMES == ("spp", "spg", "sgg", "sq_diff", "lmse_num", "lmse_den", "ssim_sum")
    assert capi.IMQ_COUNT_NAMES == ("n_valid", "n_windows", "n_ssim")
    assert (capi.IMQ_SUMS, capi.IMQ_COUNTS) == (len(capi.IMQ_SUM_NAMES), len(capi.IMQ_COUNT_NAMES))
    assert re.search(r"#define INERF_IMQ_SUMS\s+%d\b" % capi.IMQ_SUMS, text) and re.search(r"#define INERF_IMQ_COUNTS\s+%d\b" % capi.IMQ_COUNTS, text)
    for i, name in enumerate(capi.IMQ_SUM_NAMES + capi.IMQ_COUNT_NAMES):
        assert re.search(r"#define INERF_IMQ_%s\s+%d\b" % (name.upper(), i % capi.IMQ_SUMS), text), name
    # the ctypes mirror in header field order
    body = text[text.index("typedef struct inerf_imq_args"):text.index("} inerf_imq_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"([a-z_0-9]+)(?:\[11\])?\s*;", body) == [f[0] for f in capi.ImqArgs._fields_]
    assert C.sizeof(capi.ImqArgs) == 16 + 9 * 8 + 8 + 11 * 8 + 2 * 8 + 4 * 8


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
def test_helper_filter_equals_scipy_gaussian_filter():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    x = rng.random((48, 67))
    want = ndimage.gaussian_filter(x, sigma=1.5, truncate=3.5)[5:-5, 5:-5]
    t = M.taps()
    assert t.shape == (11,) and abs(t.sum() - 1.0) < 1e-15 and np.array_equal(t, t[::-1])
    got = sum(t[dy] * t[dx] * x[dy: dy + 38, dx: dx + 57] for dy in range(11) for dx in range(11))
    assert np.max(np.abs(got - want)) < 1e-14
    # ... and the map built from it: mu, sigma^2 by subtraction, on a pair of images
    y = rng.random((48, 67))
    f = lambda a: ndimage.gaussian_filter(a, sigma=1.5, truncate=3.5)[5:-5, 5:-5]
    mx, my = f(x), f(y)
    vx, vy, vxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    want = ((2 * mx * my + 1e-4) * (2 * vxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))
    assert np.max(np.abs(M.ssim_map(x, y)[..., 0] - want)) < 1e-10


def test_helper_closed_forms():
    pred, target, _ = M.make_case(45, 67, 3, seed=1)
    g = target.astype(np.float64)
    s, total, n = M.ssim(g, g)
    assert s == 1.0 and n == 35 * 57 and total == 3 * n
    assert M.si_mse(0.5 * g, g) <= 1e-15 and M.lmse(0.5 * g, g)[0] <= 1e-15
    assert M.si_mse(pred, target) < M.mse(pred, target)
    assert M.mse(np.full((12, 13, 3), 0.25), np.full((12, 13, 3), 0.75)) == 0.25
    assert M.mse(np.full((12, 13), 0.25), np.full((12, 13), 0.75), np.eye(12, 13)) == 0.25
    m = M.metrics(np.full((30, 30, 1), 0.25), np.full((30, 30, 1), 0.75))
    assert m["psnr"] == -10.0 * np.log10(0.25) and m["si_mse"] <= 1e-30 and (m["n_valid"], m["n_windows"], m["n_ssim"]) == (900, 4, 400)
    # no window, no position, no valid pixel: NaN
    assert np.isnan(M.lmse(g[:19, :40], g[:19, :40])[0]) and M.lmse(g[:19, :40], g[:19, :40])[3] == 0
    assert np.isnan(M.ssim(g[:10], g[:10])[0])
    assert all(np.isnan(M.metrics(pred, target, np.zeros((45, 67)))[k]) for k in M.KEYS)
    # a masked pixel may hold anything; a NaN mask value is invalid
    mask = np.ones((45, 67)); mask[3, 4] = 0; mask[7, 7] = np.nan
    dirty = pred.copy(); dirty[3, 4] = np.nan; dirty[7, 7] = 1e30
    a, b = M.metrics(dirty, target, mask), M.metrics(pred, target, mask)
    assert all(a[k] == b[k] for k in ("mse", "si_mse", "lmse")) and a["n_valid"] == 45 * 67 - 2
    # window origins: range(0, H-k+1, s)
    assert M.lmse(g[:45, :67], g[:45, :67])[3] == 3 * 5 and M.lmse(g, g, None, 24, 3)[3] == 8 * 15 and M.lmse(g, g, None, 16, 16)[3] == 2 * 4


@pytest.mark.parametrize("name", list(M.case_table()))
def test_no_lmse_case_sits_near_the_scale_threshold(name):
    """Every window's sum of m p^2 is exactly 0 or >= 1e-3, so that no rounding decides the 1e-5 branch; zero windows are exempt."""
    kw, k, s = M.case_table()[name]
    pred, _, mask = M.make_case(**kw)
    spp = M.window_spp(np.nan_to_num(pred, nan=1.0), mask, k, s)
    near = (spp != 0.0) & (spp < 1e-3)
    assert not near.any(), (name, spp[near][:5])
    if (k, s) == (20, 10) and kw.get("mask") in (None, "random") and not kw.get("black_window") and spp.size:
        assert spp.min() >= 70.0, (name, spp.min())
    if kw.get("mask") in ("zero", "window") or kw.get("black_window"):
        assert (spp == 0.0).any()                                    # the alpha = 0 branch is taken


# ---- the host finishing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["45x67x3", "45x67x1 mask random", "45x67x3 mask zero", "45x67x3 mask window", "45x67x3 black window",
                                  "45x67x3 nan pixel", "19x40x3", "11x11x1", "45x67x3 mask random lmse 24,3"])
def test_finish_image_quality_reproduces_the_helper(name):
    from intrinsicnerf_amd import evaluation
    kw, k, s = M.case_table()[name]
    pred, target, mask = M.make_case(**kw)
    sums, counts = M.sums_and_counts(pred, target, mask, k, s)
    got, want = evaluation.finish_image_quality(sums, counts, kw["channels"]), M.metrics(pred, target, mask, k, s)
    assert list(got) == list(evaluation.IMAGE_QUALITY_KEYS) == list(M.KEYS)
    for key in M.KEYS:
        assert np.isnan(got[key]) == np.isnan(want[key]), (key, got[key], want[key])
        if not np.isnan(want[key]):
            tol = 1e-9 if key == "psnr" else 1e-12           # psnr: d log10(mse) = 4.3 d mse / mse, mse >= 1e-2 here
            assert abs(got[key] - want[key]) <= tol, (key, got[key], want[key])
        assert isinstance(got[key], (float, np.float64))
    stack = evaluation.finish_image_quality_stack(np.stack([sums, sums]), np.stack([counts, counts]), kw["channels"])
    assert len(stack["frames"]) == 2 and all(np.array_equal(stack["mean"][k2], got[k2], equal_nan=True) for k2 in M.KEYS)


def test_ssim_taps_are_the_helpers():
    from intrinsicnerf_amd import evaluation
    assert np.array_equal(np.array(evaluation.ssim_taps()), M.taps())


# ---- the C entry points' argument checks (no launch) ------------------------------------------------------------------------------
def _args(capi, **over):
    a = capi.ImqArgs()
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p).value
    a.n_images, a.height, a.width, a.channels = 1, 30, 30, 3
    a.pred, a.pred_pixel_stride, a.trgt, a.trgt_pixel_stride = ptr, 3, ptr, 3
    a.mask, a.mask_pixel_stride = None, 1
    a.window_size, a.window_shift = 20, 10
    a.sums, a.counts, a.workspace, a.workspace_bytes = ptr, ptr, ptr, 1 << 40
    for k, v in over.items():
        setattr(a, k, v)
    a._keep = buf
    return a


def test_argument_validation_without_a_device(capi):
    lib = capi.lib()
    ws = lib.inerf_image_quality_workspace_bytes
    # 30 x 30, s = 10: 9 cells, one lane group of 64 per cell -> 3 workgroups of 5 slots, 27 cell slots, 1 window row, 20 x 20
    # positions in two 32 x 16 tiles
    assert ws(1, 30, 30, 3, 20, 10) == 8 * (3 * 5 + 9 * 3 + 2 + 2 * 2)
    assert ws(7, 30, 30, 1, 20, 10) == 7 * ws(1, 30, 30, 3, 20, 10)
    assert ws(1, 19, 40, 3, 20, 10) == 8 * (2 * 5 + 8 * 3 + 0 + 2)                     # no window; 9 x 30 positions: one tile
    assert ws(1, 10, 10, 3, 20, 10) == 8 * (1 * 5 + 1 * 3)                             # neither
    assert ws(0, 30, 30, 3, 20, 10) == 0 and ws(1, 0, 30, 3, 20, 10) == 0
    big = ws(1, 4000, 4000, 3, 20, 10)
    assert big == 8 * (256 * 5 + 400 * 400 * 3 + 256 * 2 + 256 * 2)                    # every grid at its cap
    assert ws(1, 30, 30, 2, 20, 10) == capi.E_INVALID and ws(-1, 30, 30, 3, 20, 10) == capi.E_INVALID and ws(1, -1, 30, 3, 20, 10) == capi.E_INVALID
    for k, s in ((20, 7), (20, 0), (10, 20), (18, 2), (0, 0), (20, -10)):
        assert ws(1, 30, 30, 3, k, s) == capi.E_UNSUPPORTED, (k, s)
    for k, s in ((20, 10), (16, 16), (24, 3), (8, 1), (2, 1), (1, 1)):
        assert ws(1, 30, 30, 3, k, s) > 0, (k, s)
    assert ws(65536, 30, 30, 3, 20, 10) == capi.E_UNSUPPORTED and ws(1, 65536, 65536, 3, 20, 10) == capi.E_UNSUPPORTED

    call = lambda **over: lib.inerf_image_quality(C.byref(_args(capi, **over)), None)
    assert lib.inerf_image_quality(None, None) == capi.E_INVALID
    for over in (dict(pred=None), dict(trgt=None), dict(sums=None), dict(counts=None), dict(n_images=-1), dict(height=-1), dict(width=-1),
                 dict(channels=2), dict(channels=0), dict(pred_pixel_stride=2), dict(trgt_pixel_stride=2), dict(pred_image_stride=-1),
                 dict(mask=_args(capi).pred, mask_pixel_stride=0), dict(pred=_args(capi).pred + 2), dict(mask=_args(capi).pred + 1),
                 dict(sums=_args(capi).pred + 4), dict(counts=_args(capi).pred + 4)):
        assert call(**over) == capi.E_INVALID, over
    for over in (dict(window_shift=7), dict(window_shift=0), dict(window_size=10, window_shift=20), dict(window_size=18, window_shift=2)):
        assert call(**over) == capi.E_UNSUPPORTED, over
    for over in (dict(workspace=None), dict(workspace_bytes=ws(1, 30, 30, 3, 20, 10) - 1), dict(workspace=_args(capi).pred + 4)):
        assert call(**over) == capi.E_WORKSPACE, over
    # nothing to do: accepted without a pointer
    for over in (dict(n_images=0, pred=None, trgt=None, sums=None, counts=None, workspace=None), dict(height=0, pred=None, workspace=None),
                 dict(width=0, sums=None)):
        assert call(**over) == capi.OK, over
    # channels = 1 accepts a pixel stride of 1; the argument errors come before the no-op
    assert call(n_images=0, channels=2) == capi.E_INVALID and call(n_images=0, window_shift=7) == capi.E_UNSUPPORTED
