"""The yardstick of the intrinsic-image metrics: a plain float64 numpy restatement of the definitions in include/inerf.h
(inerf_image_quality), in their DIRECT forms - sum((g - a p)^2) with the scale applied to the pixels, window sums as loops over the
k x k offsets of a window, the SSIM filter as a loop over its 11 x 11 taps - and seeded case builders.  It shares no code with
intrinsicnerf_amd/evaluation.py."""
import numpy as np

C1, C2 = 1e-4, 9e-4
THRESHOLD = 1e-5
KEYS = ("mse", "psnr", "si_mse", "lmse", "ssim", "dssim")


def taps():
    w = np.exp(-0.5 * (np.arange(-5, 6, dtype=np.float64) / 1.5) ** 2)
    return w / w.sum()


def _images(pred, target, mask):
    p, g = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    if p.ndim == 2:
        p, g = p[..., None], g[..., None]
    assert p.shape == g.shape and p.ndim == 3 and p.shape[2] in (1, 3)
    valid = np.ones(p.shape[:2], dtype=bool) if mask is None else np.asarray(mask) > 0          # NaN > 0 is False
    return p, g, valid


def _scale(spp, spg):
    return spg / spp if spp > THRESHOLD else 0.0


def moments(pred, target, mask=None):
    """(Spp, Spg, Sgg, S(g-p)^2, M) over the valid pixels and all channels."""
    p, g, valid = _images(pred, target, mask)
    pv, gv = p[valid], g[valid]
    return np.sum(pv * pv), np.sum(pv * gv), np.sum(gv * gv), np.sum((gv - pv) ** 2), int(valid.sum())


def mse(pred, target, mask=None):
    p, g, valid = _images(pred, target, mask)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(np.sum((g[valid] - p[valid]) ** 2)) / np.float64(p.shape[2] * int(valid.sum()))


def si_mse(pred, target, mask=None):
    p, g, valid = _images(pred, target, mask)
    pv, gv = p[valid], g[valid]
    a = _scale(np.sum(pv * pv), np.sum(pv * gv))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(np.sum((gv - a * pv) ** 2)) / np.float64(p.shape[2] * int(valid.sum()))


def _window_sums(values, valid, k, s):
    """[n_wy, n_wx]: for every window origin (i, j) in range(0, H-k+1, s) x range(0, W-k+1, s), the sum of `values` [H, W, C]
    over the window's valid pixels and all channels - one strided slice per offset inside the window."""
    h, w = valid.shape
    ny, nx = (h - k) // s + 1, (w - k) // s + 1
    out = np.zeros((ny, nx), dtype=np.float64)
    v = np.where(valid[..., None], values, 0.0).sum(axis=2)
    for dy in range(k):
        for dx in range(k):
            out += v[dy: dy + (ny - 1) * s + 1: s, dx: dx + (nx - 1) * s + 1: s]
    return out


def window_spp(pred, mask=None, window_size=20, window_shift=10):
    """Every window's sum of m p^2 (the quantity the 1e-5 branch looks at), flattened; empty when the image holds no window."""
    p, _, valid = _images(pred, pred, mask)
    if p.shape[0] < window_size or p.shape[1] < window_size:
        return np.zeros(0)
    return _window_sums(p * p, valid, window_size, window_shift).ravel()


def lmse(pred, target, mask=None, window_size=20, window_shift=10):
    """(lmse, numerator, denominator, number of windows)."""
    p, g, valid = _images(pred, target, mask)
    k, s = int(window_size), int(window_shift)
    h, w = valid.shape
    if h < k or w < k:
        return np.float64(np.nan), 0.0, 0.0, 0
    ny, nx = (h - k) // s + 1, (w - k) // s + 1
    spp, spg = _window_sums(p * p, valid, k, s), _window_sums(p * g, valid, k, s)
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = np.where(spp > THRESHOLD, spg / spp, 0.0)
    keep = valid[..., None]
    num_w, den_w = np.zeros((ny, nx)), np.zeros((ny, nx))
    with np.errstate(divide="ignore", invalid="ignore"):
        for dy in range(k):
            for dx in range(k):
                sl = (slice(dy, dy + (ny - 1) * s + 1, s), slice(dx, dx + (nx - 1) * s + 1, s))
                # invalid pixels contribute nothing, whatever they hold; a valid NaN stays a NaN (0 * NaN with alpha = 0 included)
                r = np.where(keep[sl], g[sl] - alpha[..., None] * p[sl], 0.0)
                t = np.where(keep[sl], g[sl], 0.0)
                num_w += (r * r).sum(axis=2)
                den_w += (t * t).sum(axis=2)
        num, den = np.sum(num_w), np.sum(den_w)
        return np.float64(num) / np.float64(den), num, den, ny * nx


def ssim_map(pred, target):
    """[H-10, W-10, C]: the SSIM map over the valid region, the 11 x 11 window applied tap by tap."""
    p, g, _ = _images(pred, target, None)
    h, w, _ = p.shape
    t = taps()
    oh, ow = h - 10, w - 10
    f = [np.zeros((oh, ow, p.shape[2])) for _ in range(5)]
    for dy in range(11):
        for dx in range(11):
            wt = t[dy] * t[dx]
            x, y = p[dy: dy + oh, dx: dx + ow], g[dy: dy + oh, dx: dx + ow]
            for acc, v in zip(f, (x, y, x * x, y * y, x * y)):
                acc += wt * v
    mx, my, exx, eyy, exy = f
    vx, vy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
    return ((2 * mx * my + C1) * (2 * vxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def ssim(pred, target, mask=None):
    """(ssim, sum of the map over channels and valid-centre positions, number of such positions)."""
    p, g, valid = _images(pred, target, mask)
    h, w, c = p.shape
    if h < 11 or w < 11:
        return np.float64(np.nan), 0.0, 0
    m = ssim_map(p, g)
    centre = valid[5: h - 5, 5: w - 5]
    total, n = np.sum(m[centre]), int(centre.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(total) / np.float64(c * n), total, n


def metrics(pred, target, mask=None, window_size=20, window_shift=10):
    """The six metrics plus the counts the device reports (n_valid, n_windows, n_ssim)."""
    p, g, valid = _images(pred, target, mask)
    e = mse(p, g, valid)
    l, _, _, n_windows = lmse(p, g, valid, window_size, window_shift)
    s, _, n_ssim = ssim(p, g, valid)
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"mse": e, "psnr": -10.0 * np.log10(e), "si_mse": si_mse(p, g, valid), "lmse": l, "ssim": s, "dssim": (1.0 - s) / 2.0,
                "n_valid": int(valid.sum()), "n_windows": n_windows, "n_ssim": n_ssim}


def sums_and_counts(pred, target, mask=None, window_size=20, window_shift=10):
    """The helper's own values of the device's rows: (Spp, Spg, Sgg, S(g-p)^2, lmse_num, lmse_den, ssim_sum), (M, n_windows, n_ssim)."""
    spp, spg, sgg, sd, m = moments(pred, target, mask)
    _, num, den, n_windows = lmse(pred, target, mask, window_size, window_shift)
    _, total, n_ssim = ssim(pred, target, mask)
    return np.array([spp, spg, sgg, sd, num, den, total], dtype=np.float64), np.array([m, n_windows, n_ssim], dtype=np.int64)


# ---- seeded cases ---------------------------------------------------------------------------------------------------------------
def make_case(height, width, channels, seed, mask=None, black_window=None, nan_pixel=None, window_size=20):
    """fp32 (pred, target, mask) in [0, 1].  pred = a smooth-ish function of target plus noise, kept in [0.25, 1] so that no window with
    a valid pixel has a sum of p^2 near the 1e-5 threshold.  ``mask``: None | "random" (70 % valid) | "zero" | "window" (the first
    window fully masked, needs height, width >= window_size).  ``black_window``: True makes pred exactly 0 on the first window.
    ``nan_pixel``: (y, x) gets a NaN in pred (all channels)."""
    rng = np.random.default_rng(seed)
    target = rng.random((height, width, channels), dtype=np.float32)
    noise = rng.random((height, width, channels), dtype=np.float32)
    pred = (np.float32(0.25) + np.float32(0.75) * (np.float32(0.7) * target + np.float32(0.3) * noise)).astype(np.float32)
    m = None
    if mask == "random":
        m = (rng.random((height, width)) < 0.7).astype(np.float32)
    elif mask == "zero":
        m = np.zeros((height, width), dtype=np.float32)
    elif mask == "window":
        m = np.ones((height, width), dtype=np.float32)
        m[:window_size, :window_size] = 0.0
    elif mask is not None:
        raise ValueError(mask)
    if black_window:
        pred[:window_size, :window_size] = 0.0
    if nan_pixel is not None:
        pred[nan_pixel[0], nan_pixel[1]] = np.nan
    return pred, target, m


SHAPES = ((11, 11), (11, 75), (12, 13), (20, 20), (19, 40), (29, 30), (30, 30), (45, 67),
          (25, 41), (27, 43),           # the SSIM tile (32 x 16 positions of the (H-10) x (W-10) valid region) straddled by -1 / +1
          (240, 320))
SECOND_TRIP_SHAPE = (267, 491)          # 17 x 16 = 272 SSIM tiles, 131 097 one-pixel cells, 130 340 windows at (2, 1): every capped grid loops


def case_table():
    """name -> (make_case keywords, window_size, window_shift): every device-against-helper case of the GPU suite."""
    cases = {}
    for i, (h, w) in enumerate(SHAPES):
        for c in (1, 3):
            cases[f"{h}x{w}x{c}"] = (dict(height=h, width=w, channels=c, seed=100 + 2 * i + c), 20, 10)
    for c in (1, 3):
        for kind in ("random", "zero", "window"):
            cases[f"45x67x{c} mask {kind}"] = (dict(height=45, width=67, channels=c, seed=200 + c, mask=kind), 20, 10)
        cases[f"45x67x{c} black window"] = (dict(height=45, width=67, channels=c, seed=210 + c, black_window=True), 20, 10)
        cases[f"45x67x{c} nan pixel"] = (dict(height=45, width=67, channels=c, seed=220 + c, nan_pixel=(22, 33)), 20, 10)
        for k, s in ((16, 16), (24, 3)):
            cases[f"45x67x{c} mask random lmse {k},{s}"] = (dict(height=45, width=67, channels=c, seed=230 + c, mask="random", window_size=k), k, s)
            cases[f"45x67x{c} black window lmse {k},{s}"] = (dict(height=45, width=67, channels=c, seed=240 + c, black_window=True, window_size=k), k, s)
    cases["240x320x3 mask random"] = (dict(height=240, width=320, channels=3, seed=250, mask="random"), 20, 10)
    h, w = SECOND_TRIP_SHAPE
    cases[f"{h}x{w}x3 mask random lmse 2,1"] = (dict(height=h, width=w, channels=3, seed=260, mask="random", window_size=2), 2, 1)
    return cases
