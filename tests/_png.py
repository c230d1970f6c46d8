"""The yardstick of the PNG tests: a decoder in plain Python + numpy + zlib, and a DEFLATE block walker.

``decode(data)`` walks the chunks (every CRC against ``zlib.crc32``), inflates the IDAT (zlib verifies the Adler-32), checks the
inflated length and the filter bytes, undoes all five filter types and returns the pixels.  ``blocks(deflate)`` walks a raw
DEFLATE stream and reports each block's type and, for dynamic blocks, its code lengths."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunks(data):
    """[(tag, payload)] of a PNG file; asserts the signature, every CRC and that nothing follows IEND."""
    data = bytes(data)
    assert data[:8] == SIGNATURE, "no PNG signature"
    out, at = [], 8
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        tag, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert len(payload) == n, f"chunk {tag!r} runs past the file"
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(tag + payload) & 0xffffffff, f"CRC of chunk {tag!r}"
        out.append((tag, payload))
        at += 12 + n
        if tag == b"IEND":
            break
    assert at == len(data), "bytes after IEND"
    assert out[0][0] == b"IHDR" and out[-1][0] == b"IEND" and out[-1][1] == b""
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def unfilter(raw, height, row_bytes, bpp):
    """(pixels uint8 [height, row_bytes], filter types [height]) of the inflated scanlines."""
    assert len(raw) == height * (1 + row_bytes), f"inflated length {len(raw)}, expected {height * (1 + row_bytes)}"
    lines = np.frombuffer(raw, dtype=np.uint8).reshape(height, 1 + row_bytes)
    types = lines[:, 0].copy()
    assert types.max(initial=0) <= 4, f"filter byte {types.max()}"
    out = np.zeros((height, row_bytes), dtype=np.uint8)
    prev = np.zeros(row_bytes, dtype=np.int64)
    for r in range(height):
        f, t = lines[r, 1:].astype(np.int64), int(types[r])
        if t == 0:
            cur = f
        elif t == 2:
            cur = (f + prev) & 255
        elif t == 1:
            cur = f.copy()
            for j in range(bpp, row_bytes):
                cur[j] = (cur[j] + cur[j - bpp]) & 255
        else:
            cur = [0] * row_bytes
            fl, pl = f.tolist(), prev.tolist()
            for j in range(row_bytes):
                a = cur[j - bpp] if j >= bpp else 0
                c = pl[j - bpp] if j >= bpp else 0
                cur[j] = (fl[j] + ((a + pl[j]) >> 1 if t == 3 else _paeth(a, pl[j], c))) & 255
            cur = np.array(cur, dtype=np.int64)
        out[r] = cur
        prev = cur
    return out, types


def decode(data, with_info=False):
    """The pixels of a PNG file: uint8 [H, W] / [H, W, 3] or uint16 [H, W].  ``with_info``: also a dict with the filter types per row,
    the zlib stream and the inflated scanlines."""
    ch = chunks(data)
    w, h, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", ch[0][1])
    assert (comp, filt, interlace) == (0, 0, 0)
    assert (colour, depth) in ((0, 8), (0, 16), (2, 8)), f"colour type {colour} at {depth} bits"
    channels = 3 if colour == 2 else 1
    stream = b"".join(p for t, p in ch if t == b"IDAT")
    d = zlib.decompressobj()
    raw = d.decompress(stream)
    assert d.eof and d.unused_data == b"", "the zlib stream does not end where the IDAT does"
    bpp = channels * depth // 8
    pixels, types = unfilter(raw, h, w * bpp, bpp)
    if depth == 16:
        image = pixels.reshape(h, w, 2).astype(np.uint16)
        image = (image[..., 0] << 8 | image[..., 1]).astype(np.uint16)
    else:
        image = pixels.reshape(h, w, 3) if channels == 3 else pixels.reshape(h, w)
    if with_info:
        return image, {"filters": types, "zlib": stream, "raw": raw, "n_idat": sum(t == b"IDAT" for t, _ in ch)}
    return image


class _Bits:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.data[self.at >> 3] >> (self.at & 7)) & 1) << i
            self.at += 1
        return v


def _table(lengths):
    """{(length, code): symbol} of the canonical code; also asserts nothing about completeness (the caller reads `kraft`)."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _symbol(bits, table):
    code = 0
    for l in range(1, 16):
        code = code << 1 | bits.take(1)
        if (l, code) in table:
            return table[(l, code)]
    raise AssertionError("no code matches")


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385,
              24577]
_DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def blocks(deflate):
    """Walks a raw DEFLATE stream.  A list of dicts per block: ``type`` ("stored" | "fixed" | "dynamic"), ``final``, ``bytes`` (what
    it inflates to), ``start`` / ``end`` (bit positions), ``matches`` = [(length, distance)], ``leading_match`` (the block's first token is
    a match: it reaches before the block); dynamic blocks also ``litlen`` and ``dist``
    (their code lengths), ``cl`` (the code-length code's lengths) and ``repeats`` (how many 16 / 17 / 18 symbols the header used)."""
    bits, out = _Bits(bytes(deflate)), []
    while True:
        blk = {"start": bits.at, "final": bool(bits.take(1)), "matches": [], "leading_match": False}
        kind = bits.take(2)
        assert kind != 3, "block type 3"
        if kind == 0:
            bits.at = (bits.at + 7) & ~7
            n, inv = bits.take(16), bits.take(16)
            assert n ^ inv == 0xffff, "stored block: LEN / NLEN"
            blk.update(type="stored", bytes=n)
            bits.at += 8 * n
            assert bits.at <= 8 * len(bits.data)
        else:
            if kind == 1:
                litlen, dist = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
                blk.update(type="fixed")
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_ORDER[i]] = bits.take(3)
                table, lens, repeats = _table(cl), [], 0
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, table)
                    if s < 16:
                        lens.append(s)
                    else:
                        repeats += 1
                        if s == 16:
                            lens += [lens[-1]] * (3 + bits.take(2))
                        else:
                            lens += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
                assert len(lens) == hlit + hdist
                litlen, dist = lens[:hlit], lens[hlit:]
                blk.update(type="dynamic", litlen=litlen, dist=dist, cl=cl, repeats=repeats)
            lt, dt, n = _table(litlen), _table(dist), 0
            while True:
                s = _symbol(bits, lt)
                if s == 256:
                    break
                if s < 256:
                    n += 1
                    continue
                length = _LEN_BASE[s - 257] + bits.take(_LEN_EXTRA[s - 257])
                d = _symbol(bits, dt)
                blk["leading_match"] |= n == 0
                blk["matches"].append((length, _DIST_BASE[d] + bits.take(_DIST_EXTRA[d])))
                n += length
            blk["bytes"] = n
        blk["end"] = bits.at
        out.append(blk)
        if blk["final"]:
            return out


def kraft(lengths):
    """Sum of 2^-l over the non-zero lengths, as an exact fraction of 2^15."""
    return sum(1 << (15 - l) for l in lengths if l)
