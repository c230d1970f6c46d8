"""The numpy model of the device's JPEG encoder (csrc/jpeg.hip): the integer definition of DESIGN.md section 3 ("Frame movies"),
restated without the C code - `encode(image, quality)` gives the complete file the device must produce byte for byte.  Also
`reconstruct`, the exact float64 decode of the model's own quantised coefficients, and `walk`, which splits a file into its marker
segments and restart intervals.  A helper: no tests inside."""
import numpy as np

# T.81 Annex K, Tables K.1 and K.2 (natural order)
LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                 95, 98, 112, 100, 103, 99], dtype=np.int64)
CHROMA = np.full(64, 99, dtype=np.int64)
CHROMA.reshape(8, 8)[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]

# T.81 Annex K, Tables K.3 - K.6: counts per code length 1 .. 16, then the symbols
DC_BITS = (bytes.fromhex("00010501010101010100000000000000"), bytes.fromhex("00030101010101010101010000000000"))
DC_VALS = bytes(range(12))
AC_BITS = (bytes.fromhex("0002010303020403050504040000017d"), bytes.fromhex("00020102040403040705040400010277"))
AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def zigzag():
    """The natural index of every zigzag position: the anti-diagonals of the 8 x 8 block, alternating direction."""
    order = []
    for d in range(15):
        cells = [(y, d - y) for y in range(8) if 0 <= d - y < 8]
        order += cells if d % 2 else cells[::-1]
    return np.array([y * 8 + x for y, x in order])


ZZ = zigzag()


def tables(quality):
    """(luma, chroma) in natural order: libjpeg's quality rule."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA, CHROMA))


def _codes(bits, vals):
    """{symbol: (code, length)} of the canonical code."""
    out, code, at = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[at]] = (code, length)
            code += 1
            at += 1
        code <<= 1
    return out


DC_CODES = [_codes(DC_BITS[t], DC_VALS) for t in range(2)]
AC_CODES = [_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def header(height, width, channels, quality):
    be = lambda v: int(v).to_bytes(2, "big")
    q = tables(quality)
    out = b"\xff\xd8" + b"\xff\xe0" + be(16) + b"JFIF\0" + b"\x01\x01\x00" + be(1) + be(1) + b"\0\0"
    nt = 2 if channels == 3 else 1
    for t in range(nt):
        out += b"\xff\xdb" + be(67) + bytes([t]) + bytes(int(v) for v in q[t][ZZ])
    out += b"\xff\xc0" + be(8 + 3 * channels) + b"\x08" + be(height) + be(width) + bytes([channels])
    for i in range(channels):
        out += bytes([i + 1, 0x11, 1 if i else 0])
    for t in range(nt):
        out += b"\xff\xc4" + be(2 + 1 + 16 + 12) + bytes([t]) + DC_BITS[t] + DC_VALS
        out += b"\xff\xc4" + be(2 + 1 + 16 + 162) + bytes([0x10 | t]) + AC_BITS[t] + AC_VALS[t]
    out += b"\xff\xdd" + be(4) + be((width + 7) // 8)
    out += b"\xff\xda" + be(6 + 2 * channels) + bytes([channels])
    for i in range(channels):
        out += bytes([i + 1, 0x11 if i else 0x00])
    return out + b"\x00\x3f\x00"


def dct_matrix():
    u, x = np.mgrid[0:8, 0:8]
    a = np.where(u == 0, np.sqrt(1 / 8), 0.5)
    return np.rint(8192 * a * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


M = dct_matrix()


def components(image):
    """[C, 8 * rows, 8 * cols] int64 samples 0 .. 255: Y Cb Cr in 16-bit fixed point for an RGB image, padded by edge replication."""
    a = np.asarray(image).astype(np.int64)
    if a.ndim == 3:
        r, g, b = a[..., 0], a[..., 1], a[..., 2]
        a = np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                      (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16,
                      (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16])
    else:
        a = a[None]
    h, w = a.shape[1:]
    return np.pad(a, ((0, 0), (0, -h % 8), (0, -w % 8)), mode="edge")


def quantised(image, quality):
    """[C, rows, cols, 8 (v), 8 (u)] int64: the quantised coefficients, natural order."""
    comp = components(image)
    c, hh, ww = comp.shape
    blocks = (comp - 128).reshape(c, hh // 8, 8, ww // 8, 8).transpose(0, 1, 3, 2, 4)          # [c, by, bx, y, x]
    t = (np.einsum("ux,cijyx->cijyu", M, blocks) + 256) >> 9                   # 4 fraction bits
    coef = (np.einsum("vy,cijyu->cijvu", M, t) + 8192) >> 14                   # 3 fraction bits
    q = tables(quality)
    out = np.empty_like(coef)
    for k in range(c):
        qt = q[1 if k else 0].reshape(8, 8)
        out[k] = np.sign(coef[k]) * ((np.abs(coef[k]) + 4 * qt) // (8 * qt))    # round half away from zero of coef / (8 q)
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, length):
        self.acc = (self.acc << length) | value
        self.n += length

    def done(self):
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        return self.acc.to_bytes(self.n // 8, "big").replace(b"\xff", b"\xff\x00")


def _value(v):
    """(size, value bits) of a DC difference or AC coefficient."""
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def encode(image, quality):
    image = np.asarray(image)
    assert image.dtype == np.uint8 and (image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 3))
    h, w = image.shape[:2]
    c = 1 if image.ndim == 2 else 3
    q = quantised(image, quality).reshape(c, (h + 7) // 8, (w + 7) // 8, 64)[..., ZZ]
    out = header(h, w, c, quality)
    rows = q.shape[1]
    for row in range(rows):
        bits, pred = _Bits(), [0] * c
        for mcu in range(q.shape[2]):
            for k in range(c):
                t, z = 1 if k else 0, [int(v) for v in q[k, row, mcu]]
                size, value = _value(z[0] - pred[k])
                pred[k] = z[0]
                bits.put(*DC_CODES[t][size])
                bits.put(value, size)
                run = 0
                for v in z[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bits.put(*AC_CODES[t][0xf0])
                        run -= 16
                    size, value = _value(v)
                    bits.put(*AC_CODES[t][run << 4 | size])
                    bits.put(value, size)
                    run = 0
                if run:
                    bits.put(*AC_CODES[t][0x00])
        out += bits.done()
        if row + 1 < rows:
            out += bytes([0xff, 0xd0 + row % 8])
    return out + b"\xff\xd9"


def reconstruct(image, quality, limit=False):
    """float64 [H, W] or [H, W, 3]: the exact inverse DCT of the model's dequantised coefficients, + 128, and the JFIF equations
    R = Y + 1.402 (Cr - 128), G = Y - 0.344136 (Cb - 128) - 0.714136 (Cr - 128), B = Y + 1.772 (Cb - 128): unrounded, unclamped.
    ``limit=True`` clamps to 0 .. 255 where every decoder does - each component plane after the inverse DCT, and the result - still
    without rounding: what a decoder's pixels are compared with (a clamp moves two values no further apart, but only when both
    sides apply it at the same place)."""
    image = np.asarray(image)
    h, w = image.shape[:2]
    coef = quantised(image, quality).astype(np.float64)
    q = tables(quality)
    for k in range(coef.shape[0]):
        coef[k] *= q[1 if k else 0].reshape(8, 8)
    u, x = np.mgrid[0:8, 0:8]
    basis = np.where(u == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)          # [u, x]
    px = np.einsum("vy,cijvu,ux->cijyx", basis, coef, basis) + 128
    c, by, bx = px.shape[:3]
    planes = px.transpose(0, 1, 3, 2, 4).reshape(c, by * 8, bx * 8)[:, :h, :w]
    if limit:
        planes = np.clip(planes, 0, 255)
    if c == 1:
        return planes[0]
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], -1)
    return np.clip(rgb, 0, 255) if limit else rgb


def walk(data):
    """(segments, intervals, restarts): [(marker, payload)] of the marker segments in order (SOI and EOI with empty payloads), the
    entropy-coded data split at the RSTm markers (stuffed bytes as in the file), and the m of every RSTm."""
    assert data[:2] == b"\xff\xd8"
    segments, at = [(0xd8, b"")], 2
    while True:
        assert data[at] == 0xff, f"no marker at {at}"
        marker = data[at + 1]
        length = int.from_bytes(data[at + 2:at + 4], "big")
        segments.append((marker, data[at + 4:at + 2 + length]))
        at += 2 + length
        if marker == 0xda:
            break
    intervals, restarts, start = [], [], at
    while True:
        i = data.index(b"\xff", at)
        nxt = data[i + 1]
        if nxt == 0x00:
            at = i + 2
        elif 0xd0 <= nxt <= 0xd7:
            intervals.append(data[start:i])
            restarts.append(nxt - 0xd0)
            start = at = i + 2
        else:
            assert nxt == 0xd9 and i + 2 == len(data), f"marker {nxt:#x} at {i} inside the entropy-coded data"
            intervals.append(data[start:i])
            segments.append((0xd9, b""))
            return segments, intervals, restarts


# ---- the shapes and contents the CPU and GPU tests share ---------------------------------------------------------------------------
CHUNK_MCUS_COLOUR = 32          # csrc/jpeg.hip walks a row in chunks of 96 blocks: 32 colour MCUs
SHAPES = ((1, 1), (8, 8, 3), (9, 17, 3), (16, 24), (72, 8), (8, 8 * (CHUNK_MCUS_COLOUR + 1), 3), (240, 320, 3))


def sparse_block():
    """An 8 x 8 uint8 block whose quantised AC coefficients (quality 50) are non-zero only at zigzag positions 20, 40 and 63: a zero
    run of 19 before the first (ZRL) and no EOB after the last."""
    coef = np.zeros(64)
    coef[ZZ[[20, 40, 63]]] = 150.0
    u, x = np.mgrid[0:8, 0:8]
    basis = np.where(u == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)
    return np.clip(np.rint(basis.T @ coef.reshape(8, 8) @ basis + 128), 0, 255).astype(np.uint8)


def content(name, shape, seed=0):
    h, w = shape[:2]
    if name == "zeros":
        a = np.zeros((h, w))
    elif name == "ones":
        a = np.full((h, w), 255)
    elif name == "checker":
        y, x = np.mgrid[0:h, 0:w]
        a = ((x + y) & 1) * 255
    elif name == "sparse":
        a = np.tile(sparse_block(), ((h + 7) // 8, (w + 7) // 8))[:h, :w]
    elif name == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        a = (x * 2 + y * 3) * 255 // max(2 * (w - 1) + 3 * (h - 1), 1)
        if len(shape) == 3:
            return np.stack([a, a[::-1], 255 - a], -1).astype(np.uint8)
    elif name == "noise":
        return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)
    else:
        raise KeyError(name)
    a = a.astype(np.uint8)
    return np.stack([a, a, a], -1) if len(shape) == 3 else a


QUALITY = {"zeros": 90, "ones": 90, "checker": 90, "sparse": 50, "ramp": 90, "noise": 100}


def cases():
    """[(name, image, quality)]: every content on every shape but the largest, which takes the ramp and the noise."""
    out = []
    for shape in SHAPES:
        big = shape[0] * shape[1] > 10000
        for name in (("ramp", "noise") if big else QUALITY):
            out.append((f"{name}-{'x'.join(map(str, shape))}", content(name, shape, seed=len(out)), QUALITY[name]))
    return out


_files = {}


def model_file(name, image, quality):
    """encode(image, quality), computed once per case and shared."""
    if name not in _files:
        _files[name] = encode(image, quality)
    return _files[name]
