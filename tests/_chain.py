"""Exact comparison of two runs of the input-gradient chain (csrc/mlp_bwd.hip): which f16 halves of the gradient buffer differ, at
which slot, point and channel, and whether the one legitimate difference between the chain's two forms explains them.

That difference is the FLOOR case: h7 below the fragments' 4e-9 floor decodes to 0 while its ReLU mask bit is set.  The two-workgroup
chain gates d h7 with the mask bit, the eight-wave chain with the decoded value; so at such a point d h7 differs in the floor
channels, and the dense layers below carry that into every channel of dZ_h6 .. dZ_h0 of the same point - and nowhere else."""
import collections
import ctypes as C

import numpy as np
import torch

from intrinsicnerf_amd import _capi, kernels

TRUNK = tuple(range(kernels.SAVE_H0, kernels.SAVE_H0 + 8))
SLOT_NAMES = {kernels.SAVE_H0 + i: f"h{i}" for i in range(8)}
SLOT_NAMES.update({kernels.SAVE_AS1H: "as1h", kernels.SAVE_FEAT: "feat", kernels.SAVE_VH: "vh", kernels.SAVE_SEMH: "semh"})

# one difference nobody explained: slot name ('h0'..'h7', 'as1h', 'feat', 'vh', 'semh', 'dpre', 'norm'), 64-point tile, point, and
# channel (the column for 'dpre', -1 for 'norm')
Difference = collections.namedtuple("Difference", "slot tile point channel")


def slot_range(desc, p, first_slot, last_slot):
    """Element range of the slots first_slot .. last_slot (inclusive) of an activation / gradient buffer."""
    off, width = C.c_int64(), C.c_int()
    lib = _capi.lib()
    _capi.check(lib.inerf_mlp_save_slot(desc, first_slot, p, C.byref(off), C.byref(width)), "inerf_mlp_save_slot")
    first = off.value
    _capi.check(lib.inerf_mlp_save_slot(desc, last_slot, p, C.byref(off), C.byref(width)), "inerf_mlp_save_slot")
    return first, off.value + (p + 63) // 64 * 64 * width.value


def _last_written_slot(desc):
    return kernels.SAVE_SEMH if desc.variant == _capi.VARIANT_SSR else kernels.SAVE_VH


def chain_layout(desc, p):
    """The segments of ``chain_words``: (name, slot, first word, words, width) - the FRAGMENT slots h0 .. the last one the chain
    writes (slot order, width 256 or 128; a slot of width 0 is left out), the head pre-activation gradients (rows [p, 8]) and
    the per-point normalisers (64 * ceil(p / 64) floats)."""
    lib = _capi.lib()
    off, width = C.c_int64(), C.c_int()
    padded = (p + 63) // 64 * 64
    base, end = slot_range(desc, p, kernels.SAVE_H0, _last_written_slot(desc))
    segs = []
    for slot in range(kernels.SAVE_H0, _last_written_slot(desc) + 1):
        _capi.check(lib.inerf_mlp_save_slot(desc, slot, p, C.byref(off), C.byref(width)), "inerf_mlp_save_slot")
        if width.value:
            segs.append((SLOT_NAMES[slot], slot, off.value - base, padded * width.value, width.value))
    segs.append(("dpre", kernels.SAVE_DPRE, end - base, 8 * p, 8))
    segs.append(("norm", kernels.SAVE_ENC, end - base + 8 * p, padded, 1))
    return segs


def chain_words(desc, dz, p):
    """The words the chain writes into a gradient buffer ``dz`` as one int32 tensor (layout: ``chain_layout``)."""
    first, last = slot_range(desc, p, kernels.SAVE_H0, _last_written_slot(desc))
    dpre = slot_range(desc, p, kernels.SAVE_DPRE, kernels.SAVE_DPRE)
    norm = slot_range(desc, p, kernels.SAVE_ENC, kernels.SAVE_ENC)[0]
    return torch.cat([dz[first:last], dz[dpre[0]:dpre[0] + 8 * p], dz[norm:norm + (p + 63) // 64 * 64]]).view(torch.int32).clone()


def frag_half_map(width):
    """(point within the tile, channel, plane) of every f16 half of ONE 64-point tile of a FRAGMENT slot of ``width`` channels,
    in memory order (include/inerf.h: half = (((kb * (width / 32) + cb) * 2 + plane) * 512 + lane * 8 + i;
    channel = 32 cb + (lane & 31), point = 32 (kb >> 1) + (i & 3) + 8 ((i >> 2) + 2 (kb & 1)) + 4 (lane >> 5)).  The map that
    kernels.frag_decode inverts; int64 tensors of 128 * width entries."""
    h = torch.arange(64 * width * 2)
    i, lane, plane, block = h & 7, (h >> 3) & 63, (h >> 9) & 1, h >> 10
    cbs = width // 32
    kb, cb = block // cbs, block % cbs
    point = 32 * (kb >> 1) + (i & 3) + 8 * ((i >> 2) + 2 * (kb & 1)) + 4 * (lane >> 5)
    return point, 32 * cb + (lane & 31), plane


def mask_word_map():
    """The ReLU mask words of one tile and layer (layout.h relu_bits_offset: [tile][layer][wave 4][lane 64][rb 2] 32-bit words behind
    the slots of the activation buffer) -> (point within the tile, channel, bit) of every bit, as numpy arrays indexed
    [wave, lane, rb, pb, g, i]; bit 31 - (16 pb + 4 g + i) of word (wave, lane, rb)."""
    w, l, rb, pb, g, i = np.meshgrid(np.arange(4), np.arange(64), np.arange(2), np.arange(2), np.arange(4), np.arange(4), indexing="ij")
    chan = 64 * w + 32 * rb + 8 * g + 4 * (l >> 5) + i
    point = 32 * pb + (l & 31)
    return point, chan, 31 - (16 * pb + 4 * g + i)


def mask_bits(save, p, layer):
    """The forward's ReLU mask bits of h``layer`` (0..7) as a bool [p, 256] tensor on ``save``'s device."""
    tiles = (p + 63) // 64
    sc = kernels.SAVE_SCALARS                          # (the mask area sits between the slots and the buffer's scalars)
    words = save[-(tiles * 4096 + sc):-sc].view(torch.int32).view(tiles, 8, 512)[:, layer]
    point, chan, bit = mask_word_map()
    word = ((np.arange(4)[:, None, None] * 64 + np.arange(64)[None, :, None]) * 2 + np.arange(2)[None, None, :])[..., None, None, None]
    widx = np.zeros((64, 256), np.int64)
    shift = np.zeros((64, 256), np.int64)
    widx[point, chan] = np.broadcast_to(word, point.shape)
    shift[point, chan] = bit
    widx, shift = torch.from_numpy(widx).to(save.device), torch.from_numpy(shift).to(save.device, torch.int32)
    return (((words[:, widx] >> shift) & 1) != 0).view(tiles * 64, 256)[:p]


def floor_points(desc, save, p):
    """{point: channels} of the floor case: the channels of h7 whose mask bit is set while the decoded h7 is 0."""
    h7 = kernels.save_slot_views(desc, save, p)[kernels.SAVE_H0 + 7]
    floor = mask_bits(save, p, 7) & (h7 == 0)
    return {int(q): tuple(int(c) for c in floor[q].nonzero().flatten()) for q in floor.any(1).nonzero().flatten()}


def _halves(words):
    h = words.view(torch.int16)
    return torch.where(h == -32768, torch.zeros_like(h), h)     # -0 taken as +0 (see the differential test)


def unexplained_differences(desc, p, words_a, words_b, floor):
    """Every differing f16 half of two ``chain_words`` of the same inputs mapped to (slot, point, channel); returns the sorted
    Differences that the floor case (``floor``: ``floor_points``) does not explain - any difference outside h0 .. h7, a trunk
    difference at a point not in ``floor``, and a d h7 difference at a floor point in a channel that is not one of its floor
    channels."""
    assert words_a.shape == words_b.shape and words_a.dtype == words_b.dtype == torch.int32
    diff = (_halves(words_a) != _halves(words_b)).nonzero().flatten()
    dev = diff.device
    fp = torch.tensor(sorted(floor), dtype=torch.int64, device=dev)
    fkey = torch.tensor([q * 256 + c for q in sorted(floor) for c in floor[q]], dtype=torch.int64, device=dev)
    out = []
    for name, slot, first, n_words, width in chain_layout(desc, p):
        local = diff[(diff >= 2 * first) & (diff < 2 * (first + n_words))] - 2 * first
        if local.numel() == 0:
            continue
        if name == "dpre":
            point, chan = local // 16, (local // 2) % 8
        elif name == "norm":
            point, chan = local // 2, torch.full_like(local, -1)
        else:
            pmap, cmap, _ = (m.to(dev) for m in frag_half_map(width))
            within = local % (128 * width)
            point, chan = 64 * (local // (128 * width)) + pmap[within], cmap[within]
        if slot == kernels.SAVE_H0 + 7:
            ok = torch.isin(point * 256 + chan, fkey)
        elif slot in TRUNK:
            ok = torch.isin(point, fp)
        else:
            ok = torch.zeros_like(point, dtype=torch.bool)
        bad = torch.unique(point[~ok] * 512 + chan[~ok] + 1)                     # (channel -1: the normalisers)
        out += [Difference(name, q // 64, q, c) for q, c in zip((bad // 512).tolist(), (bad % 512 - 1).tolist())]
    return out
