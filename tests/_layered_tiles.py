"""Case tables and references for the fp32 layer kernel of csrc/layered.hip (``k_linear_f32`` and the small kernels beside it):
used by test_layered_tiles_cpu.py (the tables are fair) and test_layered_tiles_gpu.py (the kernel holds them).

The exact lattice.  Operands, bias and ``add`` hold integers in [-8, 8] stored as fp32, ``gate`` integers in [-2, 2].  A product is
then at most 64 in magnitude, a sum over k of them at most 64 k, and with bias and ``add`` 64 k + 16: while that stays below 2^24
every product and every partial sum IN ANY ORDER is an integer fp32 holds exactly, so the matrix core's result, whatever its
accumulation order and however the reduction is split, must equal the int64 product - no tolerance.  An element dropped, taken
twice or taken from the wrong row at an edge changes an integer; a masked or clamped load that leaked finds the NaN every buffer
holds around its live range.

Everything here is CPU torch / numpy; nothing imports the package.
"""
import functools

import numpy as np
import torch

LATTICE = 8                      # operands, bias, add: integers in [-LATTICE, LATTICE]
GATE_LATTICE = 2                 # gate: integers in [-2, 2], so zeros and negatives occur
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
SENTINEL = -12345.5              # no lattice value: outputs are integers


# ---------------------------------------------------------------------------------------------------------------------
# launch_linear / tile_for, wgrad_splits, wgrad_k_per of csrc/layered.hip, restated
# ---------------------------------------------------------------------------------------------------------------------
TILES = {"128x32": (128, 32, 6), "32x128": (32, 128, 6), "64x64": (64, 64, 6), "128x64": (128, 64, 4), "128x128": (128, 128, 3)}
K_STEP = 16                      # kKS: k per LDS stage
COLSUM_POINTS = 512              # kColsumPoints
COLSUM_COLUMNS = 256             # columns of dz per blockIdx.y of k_colsum


def tile_for(m, n):
    """Name of the tile ``launch_linear`` picks for an m x n product."""
    if n <= 32:
        return "128x32"
    if m <= 32:
        return "32x128"
    if m <= 64 and n <= 64:
        return "64x64"
    if n <= 64:
        return "128x64"
    return "128x128"


def wgrad_splits(n_points, rows, cols, cus):
    tm, tn, per_cu = TILES[tile_for(rows, cols)]
    tiles = ((rows + tm - 1) // tm) * ((cols + tn - 1) // tn)
    want = per_cu * cus // tiles
    return max(1, min(want, (n_points + 255) // 256))


def wgrad_k_per(n_points, splits):
    per = (n_points + splits - 1) // splits
    return (per + K_STEP - 1) // K_STEP * K_STEP


def empty_splits(n_points, splits):
    """Splits whose point range starts at or behind n_points (k_per rounds up to 16, so the last ones can be empty)."""
    k_per = max(wgrad_k_per(n_points, splits), K_STEP)
    return splits - (n_points + k_per - 1) // k_per


def splits_from_workspace(nbytes, n_points, rows, cols):
    """Split count behind ``inerf_linear_wgrad_workspace_bytes`` = 4 (align64(splits rows cols) + ceil(n / 512) rows): exact when
    rows cols is a multiple of 64."""
    assert rows * cols % 64 == 0 and nbytes % 4 == 0
    floats = nbytes // 4 - (n_points + COLSUM_POINTS - 1) // COLSUM_POINTS * rows
    assert floats % (rows * cols) == 0, (floats, rows, cols)
    return floats // (rows * cols)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the sweep: (layout, tile) -> (m, n, k)
# ---------------------------------------------------------------------------------------------------------------------
# (a_kc, b_kc): is k the unit stride of A / of B
LAYOUTS = {"forward": (1, 1), "input_gradient": (1, 0), "weight_gradient": (0, 0), "rows_by_k": (0, 1)}
SWEEP_MN = {
    "128x32": ((1, 127, 128, 129, 257), (1, 31, 32)),
    "32x128": ((1, 31, 32), (33, 127, 128, 129, 257)),
    "64x64": ((33, 63, 64), (33, 63, 64)),
    "128x64": ((65, 127, 128, 129), (33, 63, 64)),
    "128x128": ((33, 127, 128, 129, 257), (65, 127, 128, 129, 257, 513)),
}
# One row of outputs with 33 <= n <= 64 is NOT a 64x64 launch: launch_linear asks m <= 32 first, so m = 1 goes to 32x128 whatever n.  Those
# shapes are run under the tile they land on, and 64x64 gets its own lower edge m = 33 instead.
SWEEP_MN_MORE = {"32x128": ((1, 63), (1, 64))}
SWEEP_K = (1, 15, 16, 17, 33, 63)          # 16: one LDS stage and no `more` step; 17: two stages, a one-element tail
SWEEP_K_LONG = 515                          # on the 128x128 tile only
M_MAX, N_MAX, K_MAX = 257, 513, 515
# (act, bias, add, gate)
EPILOGUES = tuple((act, *form) for act in (ACT_NONE, ACT_RELU) for form in ((1, 0, 0), (1, 1, 0), (0, 1, 1)))


def sweep_ks(layout, tile):
    ks = list(SWEEP_K)
    if tile == "128x128":
        ks.append(SWEEP_K_LONG)
    if LAYOUTS[layout] == (1, 1):
        ks.append(0)                        # accepted by inerf_linear: act(bias [+ add])
    return ks


def sweep_mn(tile):
    ms, ns = SWEEP_MN[tile]
    return [(m, n) for m in ms for n in ns] + list(SWEEP_MN_MORE.get(tile, ()))


def sweep_cases(layout, tile):
    return [(m, n, k) for m, n in sweep_mn(tile) for k in sweep_ks(layout, tile)]


def lattice_bound_holds(k):
    return LATTICE * LATTICE * k + 2 * LATTICE < 2 ** 24


def framed(src, k_contiguous=True, fill=float("nan")):
    """``src`` [r, c] (float32, any device) inside a wider buffer: one frame row above, two below, two frame columns on the left, three
    on the right, all ``fill``; stored transposed unless ``k_contiguous``.  Returns (buffer, offset in floats of element (0, 0), stride
    of the r index, stride of the c index)."""
    mat = src if k_contiguous else src.t()
    rows, cols = mat.shape
    buf = torch.full((rows + 3, cols + 5), fill, dtype=torch.float32, device=src.device)
    buf[1:1 + rows, 2:2 + cols] = mat
    ld = cols + 5
    return (buf, ld + 2, ld, 1) if k_contiguous else (buf, ld + 2, 1, ld)


def _ints(gen, shape, hi):
    return torch.randint(-hi, hi + 1, shape, generator=gen, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def lattice():
    """The sweep's operands, drawn once: case (m, n, k) uses A[:m, :k], B[:n, :k], bias[:n], add[:m, :n], gate[:m, :n]."""
    g = torch.Generator().manual_seed(20240611)
    return dict(A=_ints(g, (M_MAX, K_MAX), LATTICE), B=_ints(g, (N_MAX, K_MAX), LATTICE), bias=_ints(g, (N_MAX,), LATTICE),
                add=_ints(g, (M_MAX, N_MAX), LATTICE), gate=_ints(g, (M_MAX, N_MAX), GATE_LATTICE))


def int_matmul(a, b_t):
    """a [m, k] @ b_t [n, k]^T in int64."""
    assert a.dtype == torch.int64 and b_t.dtype == torch.int64
    if a.shape[1] == 0:
        return torch.zeros(a.shape[0], b_t.shape[0], dtype=torch.int64)
    return a @ b_t.t()


def naive_matmul(a, b_t):
    out = [[0] * b_t.shape[0] for _ in range(a.shape[0])]
    al, bl = a.tolist(), b_t.tolist()
    for i in range(a.shape[0]):
        for j in range(b_t.shape[0]):
            s = 0
            for kk in range(a.shape[1]):
                s += al[i][kk] * bl[j][kk]
            out[i][j] = s
    return torch.tensor(out, dtype=torch.int64).reshape(a.shape[0], b_t.shape[0])


@functools.lru_cache(maxsize=None)
def lattice_product(k):
    """A[:, :k] B[:, :k]^T of the whole lattice in int64, once per k: case (m, n, k) reads its corner."""
    lt = lattice()
    return int_matmul(lt["A"][:, :k].contiguous(), lt["B"][:, :k].contiguous())


def epilogue_int(prod, bias, add, gate, epi):
    """What k_linear_f32's epilogue makes of an exact product, in int64: + bias, + add, ReLU, then zero where gate <= 0."""
    act, use_bias, use_add, use_gate = epi
    v = prod.clone()
    if use_bias:
        v = v + bias[None, :]
    if use_add:
        v = v + add
    if act == ACT_RELU:
        v = v.clamp_min(0)
    if use_gate:
        v = torch.where(gate > 0, v, torch.zeros_like(v))
    return v


def sweep_expected(m, n, k):
    """int64 [len(EPILOGUES), m, n]."""
    lt = lattice()
    prod = lattice_product(k)[:m, :n]
    return torch.stack([epilogue_int(prod, lt["bias"][:n], lt["add"][:m, :n], lt["gate"][:m, :n], e) for e in EPILOGUES])


# ---------------------------------------------------------------------------------------------------------------------
# 2. inerf_linear_wgrad on the lattice
# ---------------------------------------------------------------------------------------------------------------------
WGRAD_POINTS = (1, 15, 16, 17, 255, 256, 257, 513, 4097)
WGRAD_PAIRS = {                                   # (rows, cols) by the tile they are listed under
    "128x32": ((1, 1), (128, 32), (129, 17)),
    "32x128": ((3, 128), (32, 257)),
    "64x64": ((64, 64), (33, 40)),
    "128x64": ((65, 64), (128, 33)),
    "128x128": ((80, 119), (256, 319)),
}
WGRAD_COLSUM_PAIR = (300, 40)                     # rows > 256: the second blockIdx.y of k_colsum
WGRAD_LARGE = (40000, 256, 319)                   # the last splits are empty
WGRAD_ROWS_MAX, WGRAD_COLS_MAX = 300, 319
ABI_POINTS = 257                                  # point count of the accumulate / NULL bias / short workspace calls


@functools.lru_cache(maxsize=None)
def wgrad_lattice():
    g = torch.Generator().manual_seed(20240612)
    n = WGRAD_LARGE[0]
    return dict(dz=_ints(g, (n, WGRAD_ROWS_MAX), LATTICE), x=_ints(g, (n, WGRAD_COLS_MAX), LATTICE),
                dw0=_ints(g, (WGRAD_ROWS_MAX, WGRAD_COLS_MAX), LATTICE), db0=_ints(g, (WGRAD_ROWS_MAX,), LATTICE))


@functools.lru_cache(maxsize=None)
def _wgrad_prefix():
    """dz[:n]^T x[:n] of the whole lattice for every n of WGRAD_POINTS, built up range by range (int64), and the column sums."""
    wl = wgrad_lattice()
    out, acc, accb, at = {}, torch.zeros(WGRAD_ROWS_MAX, WGRAD_COLS_MAX, dtype=torch.int64), torch.zeros(WGRAD_ROWS_MAX, dtype=torch.int64), 0
    for n in WGRAD_POINTS:
        acc = acc + wl["dz"][at:n].t() @ wl["x"][at:n]
        accb = accb + wl["dz"][at:n].sum(0)
        out[n], at = (acc, accb), n
    return out


def wgrad_expected(n, rows, cols):
    """(dW [rows, cols], db [rows]) in int64 for the first n points and the leading rows / cols of the lattice."""
    if n in WGRAD_POINTS:
        dw, db = _wgrad_prefix()[n]
        return dw[:rows, :cols], db[:rows]
    return _wgrad_large()[0][:rows, :cols], _wgrad_large()[1][:rows]


@functools.lru_cache(maxsize=None)
def _wgrad_large():
    n, rows, cols = WGRAD_LARGE
    wl = wgrad_lattice()
    return wl["dz"][:n, :rows].t().contiguous() @ wl["x"][:n, :cols].contiguous(), wl["dz"][:n, :rows].sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. real-valued cases against fp64, the bounds of test_layered_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
LIN_ATOL, LIN_RTOL = 1e-5, 1e-5                   # forward and input gradient: x ~ N(0, 1), w ~ N(0, 1 / k)
WGRAD_TOL = 3e-6                                  # weight gradient: 3e-6 sqrt(n) + 3e-6 |want|
REAL_MN = {"128x32": (129, 31), "32x128": (31, 129), "64x64": (63, 63), "128x64": (129, 63), "128x128": (129, 257)}
REAL_K = (17, 63, 283, 515)
REAL_COL0 = 3                                     # input gradient: first column of W that is read
REAL_WGRAD_POINTS = 4097
NAN_K = 283                                       # NaN containment runs at this reduction length


def act_f64(v, act):
    return torch.relu(v) if act == ACT_RELU else torch.sigmoid(v) if act == ACT_SIGMOID else v


@functools.lru_cache(maxsize=None)
def real_forward_case(tile, k):
    m, n = REAL_MN[tile]
    g = torch.Generator().manual_seed(1000 * k + m + n)
    x, w, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / np.sqrt(k), torch.randn(n, generator=g)
    pre = x.double() @ w.double().t() + b.double()
    return dict(x=x, w=w, b=b, want={a: act_f64(pre, a) for a in (ACT_NONE, ACT_RELU, ACT_SIGMOID)})


@functools.lru_cache(maxsize=None)
def real_dgrad_case(tile, o):
    """out [m, n] = (dz [m, o] @ w[:, col0 : col0 + n] + add) * (gate > 0), w [o, col0 + n] ~ N(0, 1 / o)."""
    m, n = REAL_MN[tile]
    g = torch.Generator().manual_seed(2000 * o + m + n)
    dz, w = torch.randn(m, o, generator=g), torch.randn(o, REAL_COL0 + n, generator=g) / np.sqrt(o)
    add, gate = torch.randn(m, n, generator=g), torch.randn(m, n, generator=g)
    want = (dz.double() @ w.double()[:, REAL_COL0:] + add.double()) * (gate > 0)
    return dict(dz=dz, w=w, add=add, gate=gate, want=want)


@functools.lru_cache(maxsize=None)
def real_wgrad_case(tile):
    rows, cols = WGRAD_PAIRS[tile][-1]
    n = REAL_WGRAD_POINTS
    g = torch.Generator().manual_seed(3000 + rows + cols)
    dz, x = torch.randn(n, rows, generator=g), torch.randn(n, cols, generator=g)
    return dict(dz=dz, x=x, want_w=dz.double().t() @ x.double(), want_b=dz.double().sum(0))


def worst_ratio(got, want, atol, rtol):
    """max |got - want| / (atol + rtol |want|); inf where exactly one of the two is NaN."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    if not torch.equal(torch.isnan(got), torch.isnan(want)):
        return float("inf")
    r = (got - want).abs() / (atol + rtol * want.abs())
    return float(torch.nan_to_num(r, nan=0.0).max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 6. the small kernels
# ---------------------------------------------------------------------------------------------------------------------
SMALL_N = (1, 255, 256, 257)
RAW_LD = 14                                       # wider than the 11 base channels; the extra columns hold NaN


@functools.lru_cache(maxsize=None)
def combine_case(n):
    """raw rows as the heads leave them (sigmoid outputs in columns 4..10, sigma in 3, rgb not yet formed) and a cotangent."""
    g = torch.Generator().manual_seed(4000 + n)
    raw = torch.randn(n, 11, generator=g)
    raw[:, 4:11] = torch.sigmoid(2.0 * raw[:, 4:11])
    return raw.numpy().copy(), torch.randn(n, 11, generator=g).numpy().copy()


def combine_f32(raw):
    """k_intrinsic_combine in numpy fp32: rgb = albedo * shading, rounded, + residual, rounded."""
    out = raw.astype(np.float32).copy()
    for c in range(3):
        out[:, c] = (out[:, 4 + c] * out[:, 7]).astype(np.float32) + out[:, 8 + c]
    return out


def combine_bwd(raw, g, dtype):
    """k_intrinsic_combine_bwd in its stated order, every product and sum rounded to ``dtype``: dz [n, 8]."""
    r, g = raw.astype(dtype), g.astype(dtype)
    one = dtype(1.0)
    sh, d_sh = r[:, 7], g[:, 7]
    o = np.zeros((r.shape[0], 8), dtype=dtype)
    for c in range(3):
        alb, res = r[:, 4 + c], r[:, 8 + c]
        d_alb = g[:, 4 + c] + g[:, c] * sh
        d_sh = d_sh + g[:, c] * alb
        d_res = g[:, 8 + c] + g[:, c]
        o[:, c] = (d_alb * (one - alb)) * alb
        o[:, 4 + c] = (d_res * (one - res)) * res
    o[:, 3] = (d_sh * (one - sh)) * sh
    return o


EMBED_FREQS, EMBED_DIVS = (0, 1, 10), (1.0, 10.0)
EMBED_ATOL = 2e-7
# (rays, samples) whose point x band counts stand at the 256-thread workgroup edge.  255, 256 and 257 themselves exist for one band
# (n_freqs = 0) only; with 2 and 11 bands the nearest counts on either side of 256 are 254 / 256 / 258 and 253 / 264.
EMBED_POINTS = {0: ((85, 3), (64, 4), (257, 1)), 1: ((127, 1), (32, 4), (43, 3)), 10: ((23, 1), (8, 3))}


@functools.lru_cache(maxsize=None)
def embed_case(n_rays, n_samples):
    g = torch.Generator().manual_seed(5000 + 16 * n_rays + n_samples)
    return torch.randn(n_rays, 11, generator=g), torch.rand(n_rays, n_samples, generator=g) * 4 + 2


def embed_f64(rays, z, n_freqs, div, directions):
    """fp64 bands of the SAME fp32 arguments (o + d z rounded twice, then the division, in fp32 on the CPU)."""
    n, s = z.shape
    if directions:
        x = rays[:, None, 8:11].expand(n, s, 3).reshape(-1, 3)
    else:
        x = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
        if div != 1.0:
            x = x / div
    x = x.double()
    return torch.cat([x] + [f(x * float(2 ** k)) for k in range(n_freqs) for f in (torch.sin, torch.cos)], -1)
