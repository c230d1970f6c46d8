"""The frame-image rules of include/inerf.h ("Frame images") restated in numpy, float32 throughout - what the tests compare
``inerf_frame_products`` / ``inerf_frame_range`` and ``frames.depth2rgb`` against, byte for byte.  The jet table is the committed
``tests/golden/jet256.npz`` (scripts/gen_jet_table.py, from matplotlib)."""
import os
import warnings

import numpy as np

TO8B, U16, U8_CAST, THRESH, PALETTE, JET_KIND = range(6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jet256.npz")
JET = np.load(GOLDEN)["jet"]                       # uint8 [256, 3]
F = np.float32

# the casts' edge list of the issue: (value, what numpy's float32 -> uint16 cast gives)
U16_EDGES = [(65535.9, 65535), (65536.0, 0), (70000.0, 4464), (-1.0, 65535), (-0.5, 0), (float("nan"), 0), (float("inf"), 0),
             (float("-inf"), 0), (3e9, 0), (0.0, 0), (1.0, 1), (65535.0, 65535), (-65536.0, 0), (2147483520.0, 65408), (-2147483648.0, 0)]


def to_i32(x):
    """(int32)x: truncation toward zero; 0 for NaN and |x| >= 2^31.  int64 array."""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        ok = np.abs(x) < F(2147483648.0)
        return np.where(ok, np.trunc(np.where(ok, x, F(0))), 0).astype(np.int64)


def to8b(x):
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        c = np.where(x < 0, F(0), np.where(x > 1, F(1), x))
        return np.where(np.isnan(c), 0, (F(255) * np.where(np.isnan(c), F(0), c)).astype(np.int64)).astype(np.uint8)


def u16(x, scale):
    with np.errstate(all="ignore"):
        return (to_i32(np.asarray(x, F) * F(scale)) & 0xffff).astype(np.uint16)


def u8_cast(x):
    return (to_i32(x) & 0xff).astype(np.uint8)


def thresh(x, t):
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(x, F) > F(t), 255, 0).astype(np.uint8)


def palette(x, colours):
    """colours[l] for l = (int32)x in [0, C); black otherwise - NaN, negative labels, labels >= C, values beyond int32."""
    x = np.asarray(x, F)
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        ok = np.abs(x) < F(2147483648.0)
    l = to_i32(x)
    ok &= (l >= 0) & (l < len(colours))
    out = np.zeros(x.shape + (3,), np.uint8)
    out[ok] = colours[l[ok]]
    return out


def jet(x, lo, hi):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        t = (x - F(lo)) / (F(hi) - F(lo))
        nan = np.isnan(t)
        c = np.minimum(np.maximum(np.where(nan, F(0), t), F(0)), F(1))
        out = JET[np.minimum((c * F(256)).astype(np.int64), 255)]
    out[nan] = 0
    return out


def frame_range(x):
    """(nanmin, nanmax) in float32; (NaN, NaN) for an all-NaN or empty map."""
    x = np.asarray(x, F).reshape(-1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if x.size == 0:
            return F("nan"), F("nan")
        return F(np.nanmin(x)), F(np.nanmax(x))


def bytes_per_pixel(kind, width):
    return width if kind == TO8B else {U16: 2, U8_CAST: 1, THRESH: 1, PALETTE: 3, JET_KIND: 3}[kind]


def layout(n, products):
    """[(offset, bytes)] per product and the total: plane k starts at a multiple of 16 after plane k - 1."""
    at, planes = 0, []
    for kind, column, width, *_ in products:
        size = n * bytes_per_pixel(kind, width)
        planes.append((at, size))
        at += (size + 15) // 16 * 16
    return planes, at


def product(frame, spec, colours=None):
    """The plane of one product ``(kind, column, width, a, b, range)`` as a flat uint8 array; ``range``: None or (lo, hi)."""
    kind, column, width, a, b, rng = spec
    x = frame[:, column:column + width] if width > 1 else frame[:, column]
    if kind == TO8B:
        out = to8b(x)
    elif kind == U16:
        out = u16(x, a).astype("<u2").view(np.uint8)
    elif kind == U8_CAST:
        out = u8_cast(x)
    elif kind == THRESH:
        out = thresh(x, a)
    elif kind == PALETTE:
        out = palette(x, colours)
    else:
        lo, hi = (a, b) if rng is None else rng
        out = jet(x, lo, hi)
    return np.ascontiguousarray(out).reshape(-1)


def mpl_depth2rgb(depth, lo, hi):
    """The matplotlib expression the JET rule was checked against: normalise, NaN to 0, colormap, round, NaN to black."""
    import matplotlib
    depth = np.asarray(depth, F)
    with np.errstate(all="ignore"):
        t = (depth - F(lo)) / (F(hi) - F(lo))
        nan = np.isnan(t)
        out = (matplotlib.colormaps["jet"](np.where(nan, F(0), t))[..., :3] * 255).round().astype(np.uint8)
    out[nan] = 0
    return out


def edge_frame(h=37, w=53, lo=0.1, hi=10.0, seed=0):
    """The issue's 37x53 fp32 test image: values inside and outside [lo, hi], NaN and +-inf sprinkled in."""
    g = np.random.default_rng(seed)
    x = g.uniform(lo - 2.0, hi + 2.0, size=(h, w)).astype(F)
    flat = x.reshape(-1)
    idx = g.permutation(flat.size)
    flat[idx[:40]] = np.nan
    flat[idx[40:50]] = np.inf
    flat[idx[50:60]] = -np.inf
    flat[idx[60:64]] = [lo, hi, np.nextafter(F(hi), F(0)), np.nextafter(F(lo), F(100))]
    return x
