"""The case tables of tests/_layered_tiles.py are fair - no GPU: every entry lands on the tile it is listed under, every tile occurs in
every operand layout and in the weight gradient, the lattice stays exact in fp32, the int64 reference is a matrix product, and the
restated split arithmetic gives the empty trailing splits the large weight-gradient case is there for."""
import numpy as np
import pytest
import torch

import _layered_tiles as lt


def test_restated_tile_choice_matches_the_listing():
    # the five branches of launch_linear at their thresholds
    assert [lt.tile_for(m, n) for m, n in ((1, 32), (10 ** 6, 32), (32, 33), (33, 33), (64, 64), (65, 64), (64, 65), (33, 65), (32, 65))] == \
        ["128x32", "128x32", "32x128", "64x64", "64x64", "128x64", "128x128", "128x128", "32x128"]
    for tile in lt.SWEEP_MN:
        for m, n in lt.sweep_mn(tile):
            assert lt.tile_for(m, n) == tile, (tile, m, n)
    # one row with 33 <= n <= 64 is a 32x128 launch, not a 64x64 one: run where it lands
    assert {(1, 33), (1, 63), (1, 64)} <= set(lt.sweep_mn("32x128")) and min(lt.SWEEP_MN["64x64"][0]) == 33
    for tile, pairs in lt.WGRAD_PAIRS.items():
        for rows, cols in pairs:
            assert lt.tile_for(rows, cols) == tile, (tile, rows, cols)
    for tile, (m, n) in lt.REAL_MN.items():
        assert lt.tile_for(m, n) == tile
        tm, tn, _ = lt.TILES[tile]
        assert m % tm and n % tn, "the real-valued shapes end in a partial tile on both sides"
    assert lt.WGRAD_COLSUM_PAIR[0] > lt.COLSUM_COLUMNS, "the colsum pair needs a second blockIdx.y"
    assert lt.tile_for(*lt.WGRAD_LARGE[1:]) == "128x128"


def test_every_tile_occurs_in_every_layout_and_in_the_weight_gradient():
    assert sorted(lt.LAYOUTS.values()) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for layout in lt.LAYOUTS:
        seen = {lt.tile_for(m, n) for tile in lt.SWEEP_MN for m, n, _ in lt.sweep_cases(layout, tile)}
        assert seen == set(lt.TILES), (layout, seen)
        for tile in lt.SWEEP_MN:
            ks = lt.sweep_ks(layout, tile)
            assert set(lt.SWEEP_K) <= set(ks)
            assert (lt.SWEEP_K_LONG in ks) == (tile == "128x128")
            assert (0 in ks) == (lt.LAYOUTS[layout] == (1, 1))
    assert {lt.tile_for(r, c) for pairs in lt.WGRAD_PAIRS.values() for r, c in pairs} == set(lt.TILES)
    # both sides of every tile edge and of the stage length
    for tile, (ms, ns) in lt.SWEEP_MN.items():
        tm, tn, _ = lt.TILES[tile]
        assert 1 in ms or tile in ("64x64", "128x64", "128x128")          # (m = 1 belongs to other tiles there)
        assert any(m % tm == 0 for m in ms) and any(m % tm == tm - 1 for m in ms), tile
        assert any(n % tn == 0 for n in ns) and any(n % tn == tn - 1 for n in ns), tile
    assert {lt.K_STEP - 1, lt.K_STEP, lt.K_STEP + 1} <= set(lt.SWEEP_K)
    assert len(lt.EPILOGUES) == 6 and {e[0] for e in lt.EPILOGUES} == {lt.ACT_NONE, lt.ACT_RELU}


def test_the_lattice_is_exact_in_fp32():
    ks = {k for layout in lt.LAYOUTS for tile in lt.SWEEP_MN for k in lt.sweep_ks(layout, tile)}
    ks |= set(lt.WGRAD_POINTS) | {lt.WGRAD_LARGE[0]}
    for k in ks:
        assert lt.lattice_bound_holds(k), k
        assert 64 * k + 16 < 2 ** 24
    assert max(ks) == 40000 and not lt.lattice_bound_holds(2 ** 18)
    l = lt.lattice()
    for key, hi in (("A", 8), ("B", 8), ("bias", 8), ("add", 8), ("gate", 2)):
        assert int(l[key].min()) == -hi and int(l[key].max()) == hi, key
    assert l["A"].shape == (max(max(ms) for ms, _ in lt.SWEEP_MN.values()), lt.SWEEP_K_LONG)
    assert l["B"].shape == (max(max(ns) for _, ns in lt.SWEEP_MN.values()), lt.SWEEP_K_LONG)
    assert float((l["gate"] > 0).double().mean()) < 0.5 and bool((l["gate"] == 0).any())
    w = lt.wgrad_lattice()
    assert int(w["dz"].abs().max()) == 8 and int(w["x"].abs().max()) == 8 and int(w["dw0"].abs().max()) == 8
    # the largest value any case can hold, reached by the reference itself, is an fp32 integer
    big = lt.wgrad_expected(*lt.WGRAD_LARGE)[0]
    assert int(big.abs().max()) < 2 ** 24 and torch.equal(big.float().long(), big)
    assert float(np.float32(lt.SENTINEL)) == lt.SENTINEL and lt.SENTINEL != round(lt.SENTINEL)


@pytest.mark.parametrize("m,n,k", [(1, 1, 1), (3, 5, 4), (7, 2, 17)])
def test_int64_reference_equals_a_naive_triple_loop(m, n, k):
    l = lt.lattice()
    a, b = l["A"][:m, :k].contiguous(), l["B"][:n, :k].contiguous()
    want = lt.naive_matmul(a, b)
    assert torch.equal(lt.int_matmul(a, b), want)
    assert torch.equal(lt.lattice_product(k)[:m, :n], want)
    # the epilogue forms on that product, element by element
    exp = lt.sweep_expected(m, n, k)
    for e, (act, use_bias, use_add, use_gate) in enumerate(lt.EPILOGUES):
        for i in range(m):
            for j in range(n):
                v = int(want[i, j]) + (int(l["bias"][j]) if use_bias else 0) + (int(l["add"][i, j]) if use_add else 0)
                v = max(v, 0) if act == lt.ACT_RELU else v
                v = v if (not use_gate or int(l["gate"][i, j]) > 0) else 0
                assert int(exp[e, i, j]) == v
    # k = 0: act(bias [+ add])
    assert torch.equal(lt.sweep_expected(m, n, 0)[0], l["bias"][None, :n].expand(m, n))
    # the weight gradient's prefix sums against the loop
    wl = lt.wgrad_lattice()
    dw, db = lt.wgrad_expected(17, m, n)
    assert torch.equal(dw, lt.naive_matmul(wl["dz"][:17, :m].t().contiguous(), wl["x"][:17, :n].t().contiguous()))
    assert torch.equal(db, wl["dz"][:17, :m].sum(0))


@pytest.mark.parametrize("r,c", [(1, 1), (5, 0), (7, 3), (257, 16)])
def test_framed_buffers_address_their_live_range_and_nothing_else(r, c):
    src = torch.arange(r * c, dtype=torch.float32).reshape(r, c) + 1
    for kc in (True, False):
        if not kc and c == 0:
            continue
        buf, off, s_r, s_c = lt.framed(src, kc)
        assert torch.equal(torch.as_strided(buf, (r, c), (s_r, s_c), off), src)
        assert 1 in (s_r, s_c) and int(torch.isnan(buf).sum()) == buf.numel() - r * c
        idx = off + s_r * torch.arange(r)[:, None] + s_c * torch.arange(c)[None, :]
        live = torch.zeros(buf.numel(), dtype=torch.bool)
        live[idx.flatten()] = True
        assert torch.equal(live.reshape(buf.shape), ~torch.isnan(buf))
        # a frame on every side of the live range
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all() and torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, -1]).all()


def test_restated_split_arithmetic_gives_empty_trailing_splits():
    n, rows, cols = lt.WGRAD_LARGE
    assert lt.wgrad_splits(n, rows, cols, cus=256) == 128          # 3 workgroups x 256 CUs over 2 x 3 tiles
    assert lt.wgrad_k_per(n, 128) == 320 and lt.empty_splits(n, 128) == 3
    for splits in (1, 2):
        assert lt.empty_splits(257, splits) == 0
    assert lt.wgrad_splits(257, rows, cols, cus=256) == 2 and lt.wgrad_splits(1, 1, 1, cus=256) == 1
    for p in lt.WGRAD_POINTS:
        for pairs in lt.WGRAD_PAIRS.values():
            for r, c in pairs:
                s = lt.wgrad_splits(p, r, c, cus=256)
                assert 1 <= s <= max(1, (p + 255) // 256) and lt.wgrad_k_per(p, s) * s >= p
    # the workspace formula, read backwards
    floats = (128 * rows * cols + 63) // 64 * 64 + (n + 511) // 512 * rows
    assert lt.splits_from_workspace(4 * floats, n, rows, cols) == 128


def test_small_kernel_restatements():
    raw, g = lt.combine_case(257)
    out = lt.combine_f32(raw)
    assert out.dtype == np.float32 and np.array_equal(out[:, 3:], raw[:, 3:])
    np.testing.assert_allclose(out[:, :3], raw[:, 4:7].astype(np.float64) * raw[:, 7:8] + raw[:, 8:11], rtol=3e-7, atol=0)
    # the backward against torch autograd of the same expression in fp64
    r = torch.from_numpy(raw).double()
    pre = torch.logit(r[:, 4:11]).requires_grad_(True)                      # the heads' pre-sigmoid values
    s = torch.sigmoid(pre)
    full = torch.cat([s[:, 0:3] * s[:, 3:4] + s[:, 4:7], r[:, 3:4], s], -1)
    full.backward(torch.from_numpy(g).double())
    dz64 = lt.combine_bwd(raw, g, np.float64)
    np.testing.assert_allclose(dz64[:, :7], pre.grad.numpy(), rtol=1e-9, atol=1e-12)
    assert not dz64[:, 7].any()
    dz32 = lt.combine_bwd(raw, g, np.float32)
    assert dz32.dtype == np.float32 and np.abs(dz32 - dz64).max() <= 1e-6
    for l, cases in lt.EMBED_POINTS.items():
        counts = [r_ * s_ * (l + 1) for r_, s_ in cases]
        assert min(counts) < 256 < max(counts) and (256 in counts or 256 % (l + 1)), (l, counts)
    assert sorted(r_ * s_ for r_, s_ in lt.EMBED_POINTS[0]) == [255, 256, 257]
