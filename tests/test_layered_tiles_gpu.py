"""The fp32 layer kernel of csrc/layered.hip - ``k_linear_f32`` on each of its five tiles, in each of the four operand layouts, at every
edge of tile, LDS stage and split - and the small kernels beside it (cases and references: tests/_layered_tiles.py; that they are fair:
test_layered_tiles_cpu.py).

  1. the exact lattice: integer operands, the int64 product bit for bit (``torch.equal``), NaN around every live range, a sentinel
     around every output;
  2. ``inerf_linear_wgrad`` on the same lattice: dW, db, ``accumulate``, ``d_bias = NULL``, a short workspace, empty trailing splits;
  3. real-valued operands against fp64 at the bounds of test_layered_gpu.py, one shape per tile at k = 17, 63, 283, 515;
  4. NaN containment: one NaN in an operand reaches exactly its row / column, everything else keeps its bits;
  5. width 512, both networks, forward and parameter gradients against fp64 autograd;
  6. ``inerf_intrinsic_combine`` (+ backward) bit for bit against fp32 numpy, ``inerf_embed`` into a framed column range.

Every figure the module prints starts with "layered_tiles |" (profiles/layered_tiles.txt holds them as an MI355X gave them: 57 tests,
3 s).  Worst err / bound there: forward 0.25 (32x128, k = 515), input gradient 0.19, weight gradient 0.36 (dW, 256 x 319 at 4 097
points), width-512 raw 0.009 and parameter gradients 8.7e-7 of their norm, combine backward against fp64 0.076, embed 0.32; all 13 170
lattice launches and all 109 lattice weight-gradient cases (three calls each) equal the int64 product.

What scratch builds of the kernel with one value changed (no address differs) gave: `gate >= 0` for `gate > 0` fails every lattice
group and both width-512 networks; k_wgrad_reduce leaving out the last of more than 16 splits fails every weight-gradient test at 4 097
points.  A k tail let through the mask on ONE operand only is no error: the other operand's zero at that k annihilates it.
"""
import copy
import ctypes as C
import time

import numpy as np
import pytest
import torch

import _layered_tiles as lt
from test_layered_gpu import close, grad_close

pytestmark = pytest.mark.gpu
TAG = "layered_tiles |"
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"\n{TAG} module wall time {time.time() - t0:.1f} s")


class View:
    """A matrix inside a framed buffer, as the launches take it: ``ptr`` of element (0, 0) and the leading dimension (the duck type of
    ``layered.Cols``)."""

    def __init__(self, src, k_contiguous=True, fill=NAN):
        self.buf, self.off, self.s_row, self.s_col = lt.framed(src, k_contiguous, fill)
        self.shape = tuple(src.shape)
        torch.as_strided(self.buf, self.shape, (self.s_row, self.s_col), self.off)       # raises if any address leaves the buffer

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    @property
    def ld(self):
        return max(self.s_row, self.s_col)

    def live(self, buf=None):
        return torch.as_strided(self.buf if buf is None else buf, self.shape, (self.s_row, self.s_col), self.off)

    def frame_intact(self, fill):
        """Everything outside the live range still holds ``fill`` (checked on a host copy)."""
        host = self.buf.to("cpu", copy=True)
        self.live(host).fill_(fill)
        return bool((host == fill).all())


def _framed_vector(v):
    buf = torch.full((v.numel() + 2,), NAN, dtype=torch.float32, device=v.device)
    buf[1:-1] = v
    return buf[1:-1]


_cache = {}


def _lattice_dev():
    if "lattice" not in _cache:
        _cache["lattice"] = {k: v.float().to(DEV) for k, v in lt.lattice().items()}
    return _cache["lattice"]


def _wgrad_lattice_dev():
    if "wgrad" not in _cache:
        _cache["wgrad"] = {k: v.float().to(DEV) for k, v in lt.wgrad_lattice().items()}
    return _cache["wgrad"]


def _report(problems, what):
    assert not problems, f"{what}: {len(problems)} failed, first: " + "; ".join(problems[:5])


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact-lattice sweep
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", list(lt.SWEEP_MN))
@pytest.mark.parametrize("layout", list(lt.LAYOUTS))
def test_lattice_sweep_equals_the_int64_product(layout, tile):
    """Every (m, n) of the tile x every k x {none, ReLU} x {bias, bias + add, add + gate}, through ``layered._linear`` with explicit strides:
    the live range equals the int64 reference (so no NaN of the operands', add's or gate's frames got in), the output's frame keeps
    its sentinel."""
    from intrinsicnerf_amd import layered
    a_kc, b_kc = lt.LAYOUTS[layout]
    L = _lattice_dev()
    problems, launches = [], 0
    for m, n in lt.sweep_mn(tile):
        assert lt.tile_for(m, n) == tile
        bias = _framed_vector(L["bias"][:n])
        add, gate = View(L["add"][:m, :n]), View(L["gate"][:m, :n])
        for k in lt.sweep_ks(layout, tile):
            assert lt.lattice_bound_holds(k)
            a, b = View(L["A"][:m, :k], a_kc), View(L["B"][:n, :k], b_kc)
            outs = [View(torch.empty(m, n, device=DEV).fill_(lt.SENTINEL), True, lt.SENTINEL) for _ in lt.EPILOGUES]
            for out, (act, use_bias, use_add, use_gate) in zip(outs, lt.EPILOGUES):
                layered._linear(a.ptr, a.s_row, a.s_col, b.ptr, b.s_row, b.s_col, out, m, n, k, out.buf, bias=bias if use_bias else None,
                                add=add if use_add else None, gate=gate if use_gate else None, act=act)
                launches += 1
            want = lt.sweep_expected(m, n, k).float()
            host = torch.stack([out.buf for out in outs]).cpu()                 # [epilogue, 1 + m + 2, 2 + n + 3]
            live = host[:, 1:1 + m, 2:2 + n]
            for e in range(len(outs)):
                if not torch.equal(live[e], want[e]):
                    bad = live[e] != want[e]
                    problems.append(f"{layout} m={m} n={n} k={k} epilogue(act, bias, add, gate)={lt.EPILOGUES[e]}: {int(bad.sum())} of {m * n} "
                                    f"differ, first at {tuple(int(i) for i in bad.nonzero()[0])}")
            live.fill_(lt.SENTINEL)
            if not bool((host == lt.SENTINEL).all()):
                problems.append(f"{layout} m={m} n={n} k={k}: wrote outside its range")
    print(f"\n{TAG} lattice {layout} (a_kc, b_kc)={a_kc, b_kc} tile {tile}: {launches} launches, {len(problems)} differ from the int64 product")
    _report(problems, f"lattice {layout} {tile}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. inerf_linear_wgrad on the lattice
# ---------------------------------------------------------------------------------------------------------------------
def _p(v):
    return None if v is None else C.c_void_p(v)


def _workspace_bytes(n, rows, cols):
    from intrinsicnerf_amd import _capi
    nbytes = int(_capi.lib().inerf_linear_wgrad_workspace_bytes(n, rows, cols))
    assert nbytes > 0
    return nbytes


def _wgrad(dz, x, n, dw, db, accumulate=0, short_by=0):
    """The C call on framed operands; the workspace has 256 guard bytes behind it.  Returns (rc, guard intact)."""
    from intrinsicnerf_amd import _capi
    from intrinsicnerf_amd.kernels import _stream
    rows, cols = dz.shape[1], x.shape[1]
    nbytes = _workspace_bytes(n, rows, cols)
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = _capi.lib().inerf_linear_wgrad(_p(dz.ptr), dz.ld, rows, _p(x.ptr), x.ld, cols, n, _p(dw.data_ptr()), _p(None if db is None else db.data_ptr()),
                                        accumulate, _p(ws.data_ptr()), nbytes - short_by, _stream(dw))
    untouched = ws if short_by else ws[nbytes:]
    return rc, bool((untouched == 0xA5).all())


def _wgrad_lattice_case(n, rows, cols, problems):
    W = _wgrad_lattice_dev()
    dz, x = View(W["dz"][:n, :rows]), View(W["x"][:n, :cols])          # rows beyond n and columns beside the range: NaN
    want_w, want_b = (t.float() for t in lt.wgrad_expected(n, rows, cols))
    tag = f"wgrad n={n} rows={rows} cols={cols}"
    dw, db = (torch.full(s, lt.SENTINEL, device=DEV) for s in ((rows, cols), (rows,)))
    rc, guard = _wgrad(dz, x, n, dw, db)
    dw2, db2 = (torch.full(s, lt.SENTINEL, device=DEV) for s in ((rows, cols), (rows,)))
    rc2, guard2 = _wgrad(dz, x, n, dw2, db2)
    if rc or rc2 or not (guard and guard2):
        problems.append(f"{tag}: rc {rc}, {rc2}, workspace guard intact {guard}, {guard2}")
    if not (torch.equal(dw.cpu(), want_w) and torch.equal(db.cpu(), want_b)):
        problems.append(f"{tag}: {int((dw.cpu() != want_w).sum())} of dW, {int((db.cpu() != want_b).sum())} of db differ from int64")
    if not (torch.equal(dw.view(torch.int32), dw2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32))):
        problems.append(f"{tag}: two calls differ")
    # accumulate = 1 onto integers
    dw0, db0 = W["dw0"][:rows, :cols].clone(), W["db0"][:rows].clone()
    want_w0, want_b0 = dw0.cpu() + want_w, db0.cpu() + want_b
    rc, guard = _wgrad(dz, x, n, dw0, db0, accumulate=1)
    if rc or not guard or not (torch.equal(dw0.cpu(), want_w0) and torch.equal(db0.cpu(), want_b0)):
        problems.append(f"{tag}: accumulate = 1: rc {rc}, {int((dw0.cpu() != want_w0).sum())} of dW, {int((db0.cpu() != want_b0).sum())} of db differ")


@pytest.mark.parametrize("tile", list(lt.WGRAD_PAIRS) + ["colsum"])
def test_wgrad_lattice_equals_the_int64_product(tile):
    """dW and db of every point count x the tile's (rows, cols), operands framed in NaN with rows beyond n_points: equal to int64, twice
    the same bytes, and accumulated onto an integer-filled dW / db.  ``colsum``: 300 rows, the second blockIdx.y of k_colsum."""
    pairs = [lt.WGRAD_COLSUM_PAIR] if tile == "colsum" else lt.WGRAD_PAIRS[tile]
    problems = []
    for rows, cols in pairs:
        for n in lt.WGRAD_POINTS:
            _wgrad_lattice_case(n, rows, cols, problems)
    print(f"\n{TAG} lattice wgrad {tile}: {len(pairs)} x {len(lt.WGRAD_POINTS)} cases x (plain, repeat, accumulate), {len(problems)} problems")
    _report(problems, f"lattice wgrad {tile}")


def test_wgrad_lattice_with_empty_trailing_splits():
    """40 000 points into 256 x 319: one round of workgroups is 128 splits on 256 CUs, each of 320 points (rounded up to 16), so the
    last splits start behind the data and must contribute exact zeros."""
    n, rows, cols = lt.WGRAD_LARGE
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    splits = lt.splits_from_workspace(_workspace_bytes(n, rows, cols), n, rows, cols)
    assert splits == lt.wgrad_splits(n, rows, cols, cus), (splits, cus)
    empty = lt.empty_splits(n, splits)
    print(f"\n{TAG} wgrad {n} points {rows} x {cols}: {cus} CUs, {splits} splits of {lt.wgrad_k_per(n, splits)} points, {empty} empty")
    assert empty >= 1, "no empty split on this device"
    problems = []
    _wgrad_lattice_case(n, rows, cols, problems)
    _report(problems, "lattice wgrad, empty splits")


def test_wgrad_null_bias_and_short_workspace():
    from intrinsicnerf_amd import _capi
    W = _wgrad_lattice_dev()
    n = lt.ABI_POINTS
    problems = []
    for rows, cols in [p for pairs in lt.WGRAD_PAIRS.values() for p in pairs] + [lt.WGRAD_COLSUM_PAIR]:
        dz, x = View(W["dz"][:n, :rows]), View(W["x"][:n, :cols])
        want_w = lt.wgrad_expected(n, rows, cols)[0].float()
        tag = f"wgrad n={n} rows={rows} cols={cols}"
        # d_bias = NULL: the caller's bias gradient is not this call's to touch
        dw, db = (torch.full(s, lt.SENTINEL, device=DEV) for s in ((rows, cols), (rows,)))
        rc, guard = _wgrad(dz, x, n, dw, None)
        if rc or not guard or not torch.equal(dw.cpu(), want_w) or not bool((db == lt.SENTINEL).all()):
            problems.append(f"{tag}: d_bias = NULL: rc {rc}, guard {guard}, dW equal {torch.equal(dw.cpu(), want_w)}")
        # one byte short: refused, nothing written (dW, db, the workspace itself)
        dw.fill_(lt.SENTINEL)
        rc, guard = _wgrad(dz, x, n, dw, db, short_by=1)
        if rc != _capi.E_WORKSPACE or not guard or not bool((dw == lt.SENTINEL).all()) or not bool((db == lt.SENTINEL).all()):
            problems.append(f"{tag}: workspace one byte short: rc {rc}, workspace untouched {guard}")
    _report(problems, "wgrad ABI")


# ---------------------------------------------------------------------------------------------------------------------
# 3. real-valued cases against fp64 at the bounds of test_layered_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
def _forward(case, act, x=None, w=None):
    from intrinsicnerf_amd import layered
    x, w = View((case["x"] if x is None else x).to(DEV)), (case["w"] if w is None else w).to(DEV)
    m, k = x.shape
    out = View(torch.empty(m, w.shape[0], device=DEV).fill_(lt.SENTINEL), True, lt.SENTINEL)
    layered._linear(x.ptr, x.s_row, 1, w.data_ptr(), k, 1, out, m, w.shape[0], k, out.buf, bias=case["b"].to(DEV), act=act)
    assert out.frame_intact(lt.SENTINEL), "wrote outside its range"
    return out.live().clone()


def _dgrad(case, gate=None, dz=None):
    from intrinsicnerf_amd import layered
    dz, w = View((case["dz"] if dz is None else dz).to(DEV)), case["w"].to(DEV)
    add, gate = View(case["add"].to(DEV)), View((case["gate"] if gate is None else gate).to(DEV))
    m, o = dz.shape
    n = w.shape[1] - lt.REAL_COL0
    out = View(torch.empty(m, n, device=DEV).fill_(lt.SENTINEL), True, lt.SENTINEL)
    layered._linear(dz.ptr, dz.s_row, 1, w.data_ptr() + 4 * lt.REAL_COL0, 1, w.shape[1], out, m, n, o, out.buf, add=add, gate=gate)
    assert out.frame_intact(lt.SENTINEL), "wrote outside its range"
    return out.live().clone()


@pytest.mark.parametrize("tile", list(lt.REAL_MN))
def test_real_forward_and_input_gradient_match_fp64(tile):
    """x ~ N(0, 1), w ~ N(0, 1 / k), |err| <= 1e-5 + 1e-5 |want|: forward with none / ReLU / sigmoid, input gradient with add and gate."""
    m, n = lt.REAL_MN[tile]
    problems = []
    print()
    for k in lt.REAL_K:
        fc, dc = lt.real_forward_case(tile, k), lt.real_dgrad_case(tile, k)
        ratios = [lt.worst_ratio(_forward(fc, act), fc["want"][act], lt.LIN_ATOL, lt.LIN_RTOL) for act in (0, 1, 2)]
        ratios.append(lt.worst_ratio(_dgrad(dc), dc["want"], lt.LIN_ATOL, lt.LIN_RTOL))
        print(f"{TAG} real {tile} m={m} n={n} k={k}: err / bound forward none {ratios[0]:.3f} relu {ratios[1]:.3f} sigmoid {ratios[2]:.3f}, "
              f"input gradient {ratios[3]:.3f}")
        problems += [f"k={k} {what}: {r:.3f} of the bound" for what, r in zip(("none", "relu", "sigmoid", "input gradient"), ratios) if not r <= 1.0]
    _report(problems, f"real-valued {tile}")


def _wgrad_real(case, dz=None):
    dz, x = View((case["dz"] if dz is None else dz).to(DEV)), View(case["x"].to(DEV))
    rows, cols = dz.shape[1], x.shape[1]
    dw, db = torch.empty(rows, cols, device=DEV), torch.empty(rows, device=DEV)
    rc, guard = _wgrad(dz, x, dz.shape[0], dw, db)
    assert rc == 0 and guard
    return dw, db


@pytest.mark.parametrize("tile", list(lt.WGRAD_PAIRS))
def test_real_weight_gradient_matches_fp64(tile):
    case = lt.real_wgrad_case(tile)
    n = case["dz"].shape[0]
    dw, db = _wgrad_real(case)
    atol = lt.WGRAD_TOL * float(np.sqrt(n))
    rw, rb = lt.worst_ratio(dw, case["want_w"], atol, lt.WGRAD_TOL), lt.worst_ratio(db, case["want_b"], atol, lt.WGRAD_TOL)
    print(f"\n{TAG} real wgrad {tile} n={n} rows={dw.shape[0]} cols={dw.shape[1]}: err / bound dW {rw:.3f} db {rb:.3f}")
    assert rw <= 1.0 and rb <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. NaN containment
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _only(mask_rows, mask_cols, got, base, what):
    """``got`` is NaN exactly on the given rows / columns and keeps ``base``'s bits elsewhere."""
    m, n = got.shape
    want_nan = torch.zeros(m, n, dtype=torch.bool, device=got.device)
    for r in mask_rows:
        want_nan[r, :] = True
    for c in mask_cols:
        want_nan[:, c] = True
    assert torch.equal(torch.isnan(got), want_nan), f"{what}: NaN in {int(torch.isnan(got).sum())} places, expected {int(want_nan.sum())}"
    assert torch.equal(_bits(got)[~want_nan], _bits(base)[~want_nan]), f"{what}: values beside the NaN changed"


@pytest.mark.parametrize("tile", list(lt.REAL_MN))
def test_one_nan_reaches_exactly_its_row_or_column(tile):
    """r0 and o0 sit in the last, partial tile; the NaN's k in the last, partial LDS stage."""
    m, n = lt.REAL_MN[tile]
    k = lt.NAN_K
    fc, dc = lt.real_forward_case(tile, k), lt.real_dgrad_case(tile, k)
    r0, o0 = m - 1, n - 1
    x_nan, w_nan = fc["x"].clone(), fc["w"].clone()
    x_nan[r0, k - 1] = NAN
    w_nan[o0, k - 2] = NAN
    for act in (0, 1, 2):
        base = _forward(fc, act)
        assert not torch.isnan(base).any()
        _only([r0], [], _forward(fc, act, x=x_nan), base, f"{tile} act {act}: NaN in X[{r0}, {k - 1}]")
        _only([], [o0], _forward(fc, act, w=w_nan), base, f"{tile} act {act}: NaN in W[{o0}, {k - 2}]")
    # a NaN in gate: `gate > 0` is false, the output there is 0
    base = _dgrad(dc)
    gate_nan = dc["gate"].clone()
    live = (dc["gate"] > 0).nonzero()
    r, c = (int(i) for i in live[live[:, 0] == r0][-1])                    # an open gate in the last row
    gate_nan[r, c] = NAN
    got = _dgrad(dc, gate=gate_nan)
    assert float(base[r, c]) != 0.0 and float(got[r, c]) == 0.0 and not torch.isnan(got).any()
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[r, c] = False
    assert torch.equal(_bits(got)[keep], _bits(base)[keep]), "values beside the NaN gate changed"
    dz_nan = dc["dz"].clone()
    dz_nan[r0, k - 1] = NAN                                                 # ... and in dZ: row r0, where the gate is open
    got = _dgrad(dc, dz=dz_nan)
    want_nan = torch.zeros_like(got, dtype=torch.bool)
    want_nan[r0] = (dc["gate"][r0] > 0).to(DEV)
    assert torch.equal(torch.isnan(got), want_nan) and torch.equal(_bits(got)[~want_nan], _bits(base)[~want_nan])


@pytest.mark.parametrize("tile", list(lt.WGRAD_PAIRS))
def test_one_nan_in_dz_reaches_one_row_of_the_weight_gradient(tile):
    case = lt.real_wgrad_case(tile)
    n, rows = case["dz"].shape
    dw, db = _wgrad_real(case)
    dz_nan = case["dz"].clone()
    p0, o0 = n - 1, rows - 1
    dz_nan[p0, o0] = NAN
    dw2, db2 = _wgrad_real(case, dz=dz_nan)
    _only([o0], [], dw2, dw, f"{tile}: NaN in dz[{p0}, {o0}]: dW")
    _only([o0], [], db2[:, None], db[:, None], f"{tile}: NaN in dz[{p0}, {o0}]: db")


# ---------------------------------------------------------------------------------------------------------------------
# 5. width 512 at network level
# ---------------------------------------------------------------------------------------------------------------------
def _net512(kind):
    from intrinsicnerf_amd import object_level as ol, ssr
    torch.manual_seed(512)
    if kind == "object":
        embed, ch = ol.get_embedder(10, 0)
        embed_d, ch_d = ol.get_embedder(4, 0)
        net = ol.NeRF(D=3, W=512, input_ch=ch, output_ch=5, skips=[1], input_ch_views=ch_d, use_viewdirs=True)
    else:
        embed, ch = ssr.get_embedder(10, 0, scalar_factor=10.0)
        embed_d, ch_d = ssr.get_embedder(4, 0, scalar_factor=1)
        net = ssr.Semantic_NeRF(True, 5, D=2, W=512, input_ch=ch, output_ch=5, skips=[], input_ch_views=ch_d, use_viewdirs=True)
    return net, embed, embed_d


@pytest.mark.parametrize("kind", ["object", "ssr"])
def test_width_512_forward_and_gradients_match_fp64_autograd(kind):
    """NeRF(D=3, W=512, skips=[1]) / Semantic_NeRF(D=2, W=512, 5 classes) with seeded default-init weights, 65 rays x 3 samples: raw and the
    parameter gradients of sum(cot * raw) against the same module in float64 on the CPU (the encoder's fp32 arguments, as the kernel
    forms them), at the bounds of test_layered_gpu.py."""
    from intrinsicnerf_amd import layered
    from intrinsicnerf_amd.object_level import Embedder
    net, embed, embed_d = _net512(kind)
    g = torch.Generator().manual_seed(65)
    d = torch.randn(65, 3, generator=g)
    rays = torch.cat([0.5 * torch.randn(65, 3, generator=g), d, 2.0 * torch.ones(65, 1), 6.0 * torch.ones(65, 1), d / d.norm(dim=-1, keepdim=True)], -1)
    z = torch.rand(65, 3, generator=g) * 4 + 2
    cot = torch.randn(65, 3, 11 + (5 if kind == "ssr" else 0), generator=g)
    # float64 on the CPU
    net64 = copy.deepcopy(net).double()
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    if embed.scalar_factor != 1.0:
        pts = pts / embed.scalar_factor                                       # in fp32, as k_embed divides
    dirs = rays[:, None, 8:11].expand(65, 3, 3).reshape(-1, 3)
    emb = torch.cat([Embedder(embed.n_freqs)(pts.double()), Embedder(embed_d.n_freqs)(dirs.double())], -1)
    raw64 = net64(emb).reshape(65, 3, -1)
    (cot.double() * raw64).sum().backward()
    # the layer kernels
    net = net.to(DEV)
    spec = layered.spec_for(net, embed, embed_d)
    assert spec is not None and net.fused_desc() is None and spec.width == 512
    raw = layered.evaluate(spec, net, rays.to(DEV), z.to(DEV))
    assert raw.requires_grad
    close(raw, raw64.detach(), f"W=512 {kind}: raw")
    (cot.to(DEV) * raw).sum().backward()
    want = dict(net64.named_parameters())
    worst = 0.0
    for name, p in net.named_parameters():
        assert p.grad is not None and want[name].grad is not None, name
        grad_close(p.grad, want[name].grad, f"W=512 {kind}: d {name}")
        worst = max(worst, float((p.grad.double().cpu() - want[name].grad).norm() / want[name].grad.norm()))
    print(f"\n{TAG} W=512 {kind}: raw err / bound {lt.worst_ratio(raw, raw64.detach(), 1e-5, 1e-4):.3f}, worst parameter gradient {worst:.2e} of its norm (bound 1e-4)")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the small kernels
# ---------------------------------------------------------------------------------------------------------------------
def _raw_buffers(n):
    """raw / d_raw [n + 1, RAW_LD]: NaN in the columns behind the 11 base channels, a sentinel row behind the n points."""
    raw_np, g_np = lt.combine_case(n)
    bufs = []
    for a in (raw_np, g_np):
        b = torch.full((n + 1, lt.RAW_LD), NAN, device=DEV)
        b[:n, :11] = torch.from_numpy(a).to(DEV)
        b[n] = lt.SENTINEL
        bufs.append(b)
    return raw_np, g_np, bufs[0], bufs[1]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


@pytest.mark.parametrize("n", lt.SMALL_N)
def test_intrinsic_combine_and_backward_bit_for_bit(n):
    from intrinsicnerf_amd import _capi
    from intrinsicnerf_amd.kernels import _stream
    raw_np, g_np, raw, d_raw = _raw_buffers(n)
    lib = _capi.lib()
    # backward first (the forward overwrites rgb in place; the backward does not read rgb)
    dz = torch.full((n + 1, 8), lt.SENTINEL, device=DEV)
    assert lib.inerf_intrinsic_combine_backward(_p(raw.data_ptr()), _p(d_raw.data_ptr()), lt.RAW_LD, n, _p(dz.data_ptr()), _stream(raw)) == 0
    got = dz.cpu().numpy()
    want32, want64 = lt.combine_bwd(raw_np, g_np, np.float32), lt.combine_bwd(raw_np, g_np, np.float64)
    assert _same_bits(got[:n], want32), f"{int((got[:n] != want32).sum())} of {8 * n} differ from the fp32 restatement"
    assert not got[:n, 7].any() and (got[n] == lt.SENTINEL).all()
    ratio = float((np.abs(got[:n].astype(np.float64) - want64) / (1e-6 + 1e-6 * np.abs(want64))).max())
    assert ratio <= 1.0, ratio
    # forward, in place
    assert lib.inerf_intrinsic_combine(_p(raw.data_ptr()), lt.RAW_LD, n, _stream(raw)) == 0
    got = raw.cpu().numpy()
    assert _same_bits(got[:n, :11], lt.combine_f32(raw_np)), "rgb = albedo * shading + residual, two rounded operations"
    assert np.isnan(got[:n, 11:]).all() and (got[n] == lt.SENTINEL).all()
    print(f"\n{TAG} intrinsic combine n={n}: forward and backward equal the fp32 restatement bit for bit; backward err / bound vs fp64 {ratio:.3f}")


@pytest.mark.parametrize("n_freqs", lt.EMBED_FREQS)
def test_embed_into_a_framed_column_range(n_freqs):
    from intrinsicnerf_amd import _capi
    from intrinsicnerf_amd.kernels import _stream
    lib = _capi.lib()
    width = 3 + 6 * n_freqs
    worst = 0.0
    for n_rays, n_samples in lt.EMBED_POINTS[n_freqs]:
        rays, z = lt.embed_case(n_rays, n_samples)
        rays_d, z_d = rays.to(DEV), z.to(DEV)
        for div in lt.EMBED_DIVS:
            for directions in ((0, 1) if div == 1.0 else (0,)):
                out = View(torch.empty(n_rays * n_samples, width, device=DEV).fill_(lt.SENTINEL), True, lt.SENTINEL)
                rc = lib.inerf_embed(_p(rays_d.data_ptr()), _p(z_d.data_ptr()), n_rays, n_samples, n_freqs, div, directions, _p(out.ptr), out.ld,
                                     _stream(rays_d))
                assert rc == 0
                want = lt.embed_f64(rays, z, n_freqs, div, directions)
                tag = f"embed L={n_freqs} {n_rays} x {n_samples} div={div} directions={directions}"
                close(out.live(), want, tag, atol=lt.EMBED_ATOL, rtol=0)
                assert out.frame_intact(lt.SENTINEL), f"{tag}: wrote outside its range"
                worst = max(worst, lt.worst_ratio(out.live(), want, lt.EMBED_ATOL, 0.0))
    print(f"\n{TAG} embed L={n_freqs}: point x band counts {[r * s * (n_freqs + 1) for r, s in lt.EMBED_POINTS[n_freqs]]}, worst err / bound {worst:.3f}")
