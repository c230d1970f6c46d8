"""CPU: tests/_chain.py, the exact comparison of two runs of the input-gradient chain that the GPU differential and repeat tests rest
on.  Its maps from words to (point, channel) against the fragment format kernels.frag_encode restates and the mask-word layout the
GPU mask test reads, and planted faults of the kinds the chain has had - the round-5 k-block-3 corruption of the non-first tiles, one
flipped half, one head-gradient word, one normaliser - which it must report, next to the floor case, which it must let pass."""
import ctypes as C

import numpy as np
import pytest
import torch

import _chain
from intrinsicnerf_amd import kernels


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi


@pytest.mark.parametrize("width", [256, 128, 64, 32])
def test_fragment_half_map_inverts_frag_encode(width):
    """frag_encode of an index ramp (scale 1: integers up to 256 are exact in the hi half, lo = 0) read back through the map."""
    n = 187                                                          # three tiles, the last one ragged
    tiles = (n + 63) // 64
    pmap, cmap, plane = _chain.frag_half_map(width)
    assert torch.equal(torch.sort((pmap * width + cmap) * 2 + plane)[0], torch.arange(128 * width))       # one half per (point, channel, plane)
    point = 64 * torch.arange(tiles)[:, None] + pmap[None, :]
    valid = (point < n) & (plane == 0)[None, :]
    pts = (torch.arange(n)[:, None] + 1).expand(n, width).float()
    chs = (torch.arange(width)[None, :] + 1).expand(n, width).float()
    for ramp, want in ((pts, point + 1), (chs, cmap[None, :].expand(tiles, -1) + 1)):
        frag = kernels.frag_encode(ramp, scale=1.0).float().view(tiles, 128 * width)
        assert torch.equal(frag, torch.where(valid, want, torch.zeros_like(want)).float())


def test_mask_bits_follow_the_word_layout():
    """mask_bits against the layout read off bit by bit: word [tile][layer][wave][lane][rb], channel = 64 wave + 32 rb + 8 g +
    4 (lane >> 5) + i, point = 64 tile + 32 pb + (lane & 31), bit 31 - (16 pb + 4 g + i)."""
    point, chan, _ = _chain.mask_word_map()
    assert len(set((point * 256 + chan).ravel().tolist())) == 64 * 256                       # every (point, channel) of a tile once
    p, tiles = 150, 3
    g = torch.Generator().manual_seed(4)
    words = torch.randint(-2 ** 31, 2 ** 31, (tiles, 8, 4, 64, 2), generator=g, dtype=torch.int64).to(torch.int32)
    save = torch.cat([torch.randn(1000, generator=g), words.view(-1).view(torch.float32), torch.randn(kernels.SAVE_SCALARS, generator=g)])
    w = words.numpy().view(np.uint32)
    for layer in range(8):
        got = _chain.mask_bits(save, p, layer)
        assert got.shape == (p, 256) and 0.3 < float(got.float().mean()) < 0.7
        for q, c in (divmod(int(k), 256) for k in torch.randint(0, p * 256, (300,), generator=g)):
            t, r = divmod(q, 64)
            pb, lo = divmod(r, 32)
            wave, rb, grp, hi, i = c // 64, (c // 32) % 2, (c // 8) % 4, (c // 4) % 2, c % 4
            bit = (int(w[t, layer, wave, 32 * hi + lo, rb]) >> (31 - (16 * pb + 4 * grp + i))) & 1
            assert bool(got[q, c]) == bool(bit), (layer, q, c)


def test_chain_words_and_layout_agree(capi):
    """chain_words cuts the slots h0 .. semh, the head pre-activation gradients and the normalisers out of a gradient buffer in the
    order chain_layout describes."""
    lib = capi.lib()
    for variant, c in ((capi.VARIANT_OBJECT, 0), (capi.VARIANT_SSR, 28), (capi.VARIANT_SSR, 0)):
        desc = capi.net_desc(variant, c, 10, 4, 10.0 if variant == capi.VARIANT_SSR else 1.0, capi.PREC_F16X3)
        p = 761
        dz = torch.arange(lib.inerf_mlp_save_floats(desc, p), dtype=torch.int32).view(torch.float32)
        words = _chain.chain_words(desc, dz, p)
        segs = _chain.chain_layout(desc, p)
        assert segs[0][2] == 0 and sum(s[3] for s in segs) == words.numel()
        names = [s[0] for s in segs]
        assert names == [f"h{i}" for i in range(8)] + ["as1h", "feat", "vh"] + (["semh"] if c else []) + ["dpre", "norm"]
        off, width = C.c_int64(), C.c_int()
        for name, slot, first, n_words, wd in segs:
            assert lib.inerf_mlp_save_slot(desc, slot, p, C.byref(off), C.byref(width)) == capi.OK
            assert wd == width.value or name == "norm"
            assert torch.equal(words[first:first + n_words], torch.arange(off.value, off.value + n_words, dtype=torch.int32)), name


# ---------------------------------------------------------------------------------------------------------------------
# planted faults: SSR with 28 classes (every slot kind the chain writes), 761 points = 12 tiles, a synthetic grid of 4 workgroups
# ---------------------------------------------------------------------------------------------------------------------
P, GRID = 761, 4
TILES = (P + 63) // 64


@pytest.fixture(scope="module")
def case(capi):
    desc = capi.net_desc(capi.VARIANT_SSR, 28, 10, 4, 10.0, capi.PREC_F16X3)
    segs = {s[0]: s for s in _chain.chain_layout(desc, P)}
    g = torch.Generator().manual_seed(11)
    words = torch.randint(-2 ** 31, 2 ** 31, (sum(s[3] for s in segs.values()),), generator=g, dtype=torch.int64).to(torch.int32)
    return desc, segs, words


def _half(segs, name, point, channel, plane):
    """Index of the f16 half holding (point, channel, plane) of a FRAGMENT segment, from include/inerf.h's formula."""
    _, _, first, _, width = segs[name]
    tile, q = divmod(point, 64)
    r = q % 32
    kb = 2 * (q // 32) + r // 16
    lane = 32 * ((r % 8) // 4) + channel % 32
    i = 4 * ((r % 16) // 8) + r % 4
    return 2 * first + (((tile * 4 + kb) * (width // 32) + channel // 32) * 2 + plane) * 512 + lane * 8 + i


def _flip(words, halves):
    w = words.clone()
    h = w.view(torch.int16)
    idx = torch.as_tensor(halves, dtype=torch.int64)
    h[idx] = h[idx] ^ 1
    return w


def _report(desc, a, b, floor):
    return _chain.unexplained_differences(desc, P, a, b, floor)


@pytest.mark.parametrize("slots", ["trunk", "every"])
def test_reports_the_round5_pattern(case, slots):
    """(a) k-block 3 - points 48..63 - of every dZ slot wrong on the non-first tiles of every workgroup (tile >= grid), as the
    round-5 development form of k_mlp_dgrad_dual wrote it; a floor point elsewhere changes nothing."""
    desc, segs, a = case
    names = [n for n in segs if n not in ("dpre", "norm") and (slots == "every" or n.startswith("h"))]
    halves = []
    for name in names:
        _, _, first, _, width = segs[name]
        cbs = width // 32
        for t in range(GRID, TILES):
            start = 2 * first + (t * 4 + 3) * cbs * 1024
            halves.append(torch.arange(start, start + cbs * 1024))
    b = _flip(a, torch.cat(halves))
    got = _report(desc, a, b, {5: (17,)})
    want = {(n, t, 64 * t + q, c) for n in names for t in range(GRID, TILES) for q in range(48, 64) for c in range(segs[n][4])}
    assert len(got) == len(want) and set(got) == want


def test_reports_one_half_at_a_non_floor_point(case):
    """(b) one flipped lo half of dZ_h3 at a point that is not a floor point (another one is)."""
    desc, segs, a = case
    b = _flip(a, [_half(segs, "h3", 100, 77, 1)])
    assert _report(desc, a, b, {101: (3,)}) == [_chain.Difference("h3", 1, 100, 77)]


def test_reports_one_head_gradient_word(case):
    """(c) one word of the head pre-activation gradients (rows [P, 8])."""
    desc, segs, a = case
    b = _flip(a, [2 * (segs["dpre"][2] + 200 * 8 + 5)])
    assert _report(desc, a, b, {}) == [_chain.Difference("dpre", 3, 200, 5)]


def test_reports_one_normaliser(case):
    """(d) one per-point normaliser (its high half: the exponent)."""
    desc, segs, a = case
    b = _flip(a, [2 * (segs["norm"][2] + 300) + 1])
    assert _report(desc, a, b, {300: (0,)}) == [_chain.Difference("norm", 4, 300, -1)]


def test_the_floor_case_is_explained_and_nothing_beyond_it(case):
    """A floor point: d h7 differs in its floor channel and dZ_h6 .. dZ_h0 in every channel - explained.  The same differences
    without the floor, a d h7 difference in another channel, or one in a head slot at the floor point are not."""
    desc, segs, a = case
    pf, cf = 413, 140
    halves = [_half(segs, "h7", pf, cf, pl) for pl in (0, 1)]
    halves += [_half(segs, f"h{k}", pf, c, pl) for k in range(7) for c in range(256) for pl in (0, 1)]
    b = _flip(a, halves)
    assert _report(desc, a, b, {pf: (cf,), 7: (1, 2)}) == []
    assert len(_report(desc, a, b, {})) == 1 + 7 * 256
    assert _report(desc, a, _flip(b, [_half(segs, "h7", pf, cf + 1, 0)]), {pf: (cf,)}) == [_chain.Difference("h7", 6, pf, cf + 1)]
    assert _report(desc, a, _flip(b, [_half(segs, "feat", pf, 9, 0)]), {pf: (cf,)}) == [_chain.Difference("feat", 6, pf, 9)]
    assert _report(desc, a, _flip(b, [_half(segs, "semh", pf, 9, 0)]), {pf: (cf,)}) == [_chain.Difference("semh", 6, pf, 9)]


def test_negative_zero_equals_positive_zero(case):
    """-0 against +0 in a half is no difference (a remainder lo that underflows keeps its sign in a register)."""
    desc, segs, a = case
    a, b = a.clone(), a.clone()
    i = _half(segs, "h2", 50, 3, 1)
    a.view(torch.int16)[i], b.view(torch.int16)[i] = 0, -32768
    assert _report(desc, a, b, {}) == []
    b.view(torch.int16)[i] = 1
    assert _report(desc, a, b, {}) == [_chain.Difference("h2", 0, 50, 3)]
