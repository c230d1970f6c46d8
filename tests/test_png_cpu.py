"""PNG encoding without a device: the decoder that the GPU tests measure with (_png.py) against Pillow, the file layout and every
argument check of the C entry points through the built library (made-up pointers, decided before any HIP call), the code-length
routine of csrc/png_huff.h through ``inerf_png_code_lengths``, the ABI number and the launcher switch.

Length-limited codes, recorded here as the issue asks (sum of count * length; this routine | package-merge optimum | unlimited Huffman):
    Fibonacci counts over 22 symbols, limit 15:   121 433 | 121 373 | 121 367   (unlimited depth 21)
    Fibonacci counts over 22 symbols, limit 7:    130 735 | 123 970 | 121 367
    1, 1, 2, 3 .. 144, 9 000, 30 000 and four 1s over 19 symbols, limit 7:   49 844 | 49 844 | 49 759   (unlimited depth 9)
    286 random counts up to 32 768, limit 7:      the routine refuses (286 > 2^7 symbols cannot have 7-bit codes); at limit 15 the optimum
The clamp-and-repair step is 0.05 % above package-merge on the Fibonacci counts at 15 bits and 5.5 % above it at 7 bits - a
depth-21 code squeezed into 7 bits, far from any code-length alphabet a segment produces (19 symbols, depth 9: equal to package-merge)."""
import ctypes as C
import heapq
import os
import re
import sys

import numpy as np
import pytest

import _png

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 32768


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi


def test_header_binding_and_version_agree(capi):
    with open(os.path.join(REPO, "include", "inerf.h")) as fh:
        text = fh.read()
    header = int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1))
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version() and header >= 40025
    for name in ("inerf_png_layout", "inerf_png_workspace_bytes", "inerf_png_encode", "inerf_png_code_lengths"):
        assert name in capi.SYMBOLS and re.search(r"\b%s\(" % name, text)
        assert getattr(capi.lib(), name) is not None
    assert re.search(r"#define INERF_PNG_MAX_IMAGES\s+%d\b" % capi.PNG_MAX_IMAGES, text) and capi.PNG_MAX_IMAGES == 16
    assert re.search(r"#define INERF_PNG_FILTER_ADAPTIVE\s+\(-1\)", text) and capi.PNG_FILTER_ADAPTIVE == -1
    for struct, mirror in (("inerf_png_image", capi.PngImage), ("inerf_png_args", capi.PngArgs)):
        body = text[text.index("typedef struct %s {" % struct):text.index("} %s;" % struct)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"([a-z_0-9]+)(?:\[INERF_PNG_MAX_IMAGES\])?\s*;", body) == [f[0] for f in mirror._fields_]
    assert C.sizeof(capi.PngImage) == 48 and C.sizeof(capi.PngArgs) == 64 + 16 * 48
    from intrinsicnerf_amd import _build
    assert "png.hip" in _build.SOURCES and any(h.endswith("png_huff.h") for h in _build.HEADERS)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def _noisy(shape, dtype, seed):
    g = np.random.default_rng(seed)
    h, w = shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    top = 65535 if dtype == np.uint16 else 255
    base = (x * 3 + y * 5) / (3 * w + 5 * h) * top * 0.8
    if len(shape) == 3:
        base = np.stack([base, base[::-1], base * 0.5], -1)
    out = np.clip(base + g.normal(0, top * 0.03, shape), 0, top)
    out[25:] = g.integers(0, top + 1, out[25:].shape)                       # white noise below: no filter helps, type 0 gets its turn
    return out.astype(dtype)


def test_decoder_equals_pillow_on_pillow_written_files(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    seen = set()
    for k, (shape, dtype) in enumerate((((37, 53, 3), np.uint8), ((37, 53), np.uint8), ((37, 53), np.uint16))):
        for seed in range(3):
            a = _noisy(shape, dtype, 10 * k + seed)
            path = tmp_path / f"{k}_{seed}.png"
            Image.fromarray(a).save(path, optimize=bool(seed & 1))
            data = path.read_bytes()
            got, info = _png.decode(data, with_info=True)
            want = np.array(Image.open(path))
            assert got.dtype == want.dtype == dtype and got.shape == want.shape == shape
            assert np.array_equal(got, want) and np.array_equal(got, a)
            seen |= set(int(t) for t in info["filters"])
            kinds = [b["type"] for b in _png.blocks(info["zlib"][2:-4])]
            assert kinds and set(kinds) <= {"stored", "fixed", "dynamic"}
    assert seen == {0, 1, 2, 3, 4}, seen                                    # Pillow filters adaptively: all five types were undone


def test_decoder_refuses_a_damaged_file():
    import struct
    import zlib
    raw = b"\x00\x01\x02\x03" + b"\x01\x05\x05\x05"

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    good = _png.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 3, 2, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")
    assert np.array_equal(_png.decode(good), [[1, 2, 3], [5, 10, 15]])
    bad = bytearray(good)
    bad[45] ^= 1                                                            # inside the IDAT: its CRC no longer holds
    with pytest.raises(AssertionError):
        _png.decode(bytes(bad))
    short = _png.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 3, 3, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")
    with pytest.raises(AssertionError, match="inflated length"):
        _png.decode(short)
    five = _png.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 3, 2, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(b"\x05" + raw[1:])) + chunk(b"IEND", b"")
    with pytest.raises(AssertionError, match="filter byte"):
        _png.decode(five)
    # the block walker on zlib's own streams
    noise = np.random.default_rng(0).integers(0, 256, 3000).astype(np.uint8).tobytes()
    assert [b["type"] for b in _png.blocks(zlib.compress(noise, 6)[2:-4])] == ["stored"]
    skewed = (np.random.default_rng(1).geometric(0.15, 6000) % 256).astype(np.uint8).tobytes() + b"\x07" * 700
    blk = _png.blocks(zlib.compress(skewed, 6)[2:-4])
    assert blk[-1]["final"] and sum(b["bytes"] for b in blk) == 6700 and any(m == (258, 1) for b in blk for m in b["matches"])
    assert any(b["type"] == "dynamic" and _png.kraft(b["litlen"]) == 1 << 15 for b in blk)


# ---- layout and argument checks ----------------------------------------------------------------------------------------------------
def _args(capi, images, src=0x100000, src_bytes=1 << 24, dst=0x4000000, dst_bytes=1 << 24, sizes=0x8000000, workspace=0x10000000,
          workspace_bytes=1 << 26):
    a = capi.PngArgs()
    a.src, a.src_bytes, a.dst, a.dst_bytes, a.sizes, a.workspace, a.workspace_bytes = src, src_bytes, dst, dst_bytes, sizes, workspace, workspace_bytes
    a.n_images = len(images)
    for k, spec in enumerate(images):
        im = a.images[k]
        im.height, im.width, im.channels, im.bit_depth, im.filter, im.src_offset = spec
    return a


MIX = [(24, 32, 3, 8, -1, 0), (24, 32, 1, 8, 0, 4096), (24, 32, 1, 16, 4, 8192), (400, 300, 3, 8, -1, 16384), (1, 1, 1, 8, -1, 0),
       (1, 32767, 1, 8, 2, 0), (5000, 7, 1, 16, 1, 1 << 20)]


def _capacity(h, w, c, depth):
    row = 1 + w * c * depth // 8
    rows_per_segment = CAP // row
    segments = -(-h // rows_per_segment)
    return 68 + h * row + 5 * segments, segments


def test_layout_offsets_alignment_and_the_capacity_formula(capi):
    lib = capi.lib()
    a = _args(capi, MIX)
    total = lib.inerf_png_layout(C.byref(a))
    end, segments = 0, 0
    for k, (h, w, c, depth, _, _) in enumerate(MIX):
        im = a.images[k]
        cap, n = _capacity(h, w, c, depth)
        assert im.dst_offset % 16 == 0 and im.dst_offset >= end and im.dst_offset - end < 16 and im.dst_capacity == cap, k
        end = im.dst_offset + cap
        segments += n
    assert total % 16 == 0 and 0 <= total - end < 16
    assert lib.inerf_png_workspace_bytes(C.byref(a)) == segments * (32 + CAP + 16)
    assert _capacity(1, 1, 1, 8) == (68 + 2 + 5, 1) and _capacity(400, 300, 3, 8)[1] == 12      # 36 rows of 901 bytes per segment
    from intrinsicnerf_amd import kernels
    args, files, total2, ws = kernels.png_plan([(h, w, c, d, off, f) for h, w, c, d, f, off in MIX])
    assert total2 == total and ws == segments * (32 + CAP + 16) and files == [(a.images[k].dst_offset, a.images[k].dst_capacity) for k in range(len(MIX))]
    assert kernels.png_plan([(2, 2, 1, 8, 0)])[0].images[0].filter == -1                       # the default is the adaptive filter
    with pytest.raises(ValueError):
        kernels.png_plan([(2, 2, 1, 8, 0)] * 17)
    empty = _args(capi, [])
    assert lib.inerf_png_layout(C.byref(empty)) == 0 and lib.inerf_png_workspace_bytes(C.byref(empty)) == 0


def test_validation_codes_come_back_without_a_device(capi):
    """Every refusal below is decided before any HIP call: the pointers are made up and never dereferenced."""
    lib = capi.lib()
    E, U, W = capi.E_INVALID, capi.E_UNSUPPORTED, capi.E_WORKSPACE

    def run(a, lay=True):
        if lay:
            assert lib.inerf_png_layout(C.byref(a)) >= 0
        return lib.inerf_png_encode(C.byref(a), None)

    assert lib.inerf_png_layout(None) == E and lib.inerf_png_workspace_bytes(None) == E and lib.inerf_png_encode(None, None) == E
    assert run(_args(capi, [])) == capi.OK                                                # no image: a no-op, whatever the pointers
    assert run(_args(capi, [], src=None, dst=None, sizes=None, workspace=None)) == capi.OK
    one = [(24, 32, 3, 8, -1, 0)]
    # bad dimensions, channels, bit depth, filter
    for bad in ((0, 32, 3, 8, -1, 0), (24, 0, 3, 8, -1, 0), (-1, 32, 3, 8, -1, 0), (24, -5, 1, 8, 0, 0), (24, 32, 2, 8, -1, 0), (24, 32, 4, 8, -1, 0),
                (24, 32, 0, 8, -1, 0), (24, 32, 3, 16, -1, 0), (24, 32, 1, 4, -1, 0), (24, 32, 1, 32, -1, 0), (24, 32, 1, 8, 5, 0), (24, 32, 1, 8, -2, 0)):
        a = _args(capi, [bad])
        assert lib.inerf_png_layout(C.byref(a)) == E and lib.inerf_png_workspace_bytes(C.byref(a)) == E and run(a, lay=False) == E, bad
    for n in (-1, 17):
        a = _args(capi, one)
        a.n_images = n
        assert lib.inerf_png_layout(C.byref(a)) == E and run(a, lay=False) == E
    # a filtered row that does not fit one segment; the last sizes that fit
    for spec, ok in (((2, 32767, 1, 8, -1, 0), True), ((2, 32768, 1, 8, -1, 0), False), ((2, 10922, 3, 8, -1, 0), True), ((2, 10923, 3, 8, -1, 0), False),
                     ((2, 16383, 1, 16, -1, 0), True), ((2, 16384, 1, 16, -1, 0), False)):
        a = _args(capi, [spec])
        got = lib.inerf_png_layout(C.byref(a))
        assert (got > 0) if ok else (got == U and lib.inerf_png_workspace_bytes(C.byref(a)) == U and run(a, lay=False) == U), spec
    # offsets that are not the layout's
    assert run(_args(capi, one + one), lay=False) == E
    a = _args(capi, one)
    lib.inerf_png_layout(C.byref(a))
    a.images[0].dst_capacity += 1
    assert run(a, lay=False) == E
    a = _args(capi, one + one)
    lib.inerf_png_layout(C.byref(a))
    a.images[1].dst_offset += 16
    assert run(a, lay=False) == E
    # NULL and misaligned buffers
    for field in ("src", "dst", "sizes"):
        assert run(_args(capi, one, **{field: None})) == E, field
    assert run(_args(capi, one, workspace=None)) == W
    assert run(_args(capi, one, dst=0x4000008)) == E and run(_args(capi, one, sizes=0x8000004)) == E and run(_args(capi, one, workspace=0x10000008)) == E
    # a plane that runs past src_bytes, dst_bytes below the total, a workspace that is too small
    assert run(_args(capi, one, src_bytes=24 * 32 * 3 - 1)) == E and run(_args(capi, [(24, 32, 3, 8, -1, 16)], src_bytes=24 * 32 * 3 + 15)) == E
    assert run(_args(capi, [(24, 32, 3, 8, -1, -16)])) == E and run(_args(capi, one, src_bytes=-1)) == E
    a = _args(capi, one)
    total = lib.inerf_png_layout(C.byref(a))
    assert run(_args(capi, one, dst_bytes=total - 1)) == E
    need = lib.inerf_png_workspace_bytes(C.byref(a))
    assert need == 32 + CAP + 16 and run(_args(capi, one, workspace_bytes=need - 1)) == W
    # overlaps: dst, sizes and workspace against src and each other
    S = 0x100000
    assert run(_args(capi, one, src_bytes=4096, dst=S + 4096 - 16)) == E and run(_args(capi, one, src_bytes=4096, dst=S - total + 16)) == E
    assert run(_args(capi, one, src_bytes=4096, sizes=S + 8)) == E and run(_args(capi, one, src_bytes=4096, workspace=S + 2048)) == E
    assert run(_args(capi, one, sizes=0x4000000 + 64)) == E                               # sizes inside dst
    assert run(_args(capi, one, workspace=0x4000000 + 1024)) == E                         # workspace over dst
    assert run(_args(capi, one, sizes=0x10000000 + 128)) == E                             # sizes inside the workspace
    # the Python launchers refuse host tensors
    import torch
    from intrinsicnerf_amd import frames, kernels
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        kernels.png_encode(torch.zeros(24 * 32 * 3, dtype=torch.uint8), kernels.png_plan([(24, 32, 3, 8, 0)]))
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        frames.encode_png(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="encode=True"):
        frames.FrameProducts().files(0)


# ---- code lengths ------------------------------------------------------------------------------------------------------------------
def _lengths(capi, freq, limit):
    f = (C.c_uint32 * len(freq))(*[int(v) for v in freq])
    out = (C.c_ubyte * len(freq))(*([99] * len(freq)))
    rc = capi.lib().inerf_png_code_lengths(f, len(freq), limit, out)
    return rc, list(out)


def _huffman(freq):
    """(cost, depth) of the unconstrained Huffman code over the non-zero counts."""
    heap = [(int(f), i, 0) for i, f in enumerate(freq) if f]
    if len(heap) < 2:
        return sum(f for f, _, _ in heap), 1
    heapq.heapify(heap)
    cost, tick = 0, len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return cost, heap[0][2]


def _package_merge(freq, limit):
    """The optimal cost of a code with no length above ``limit`` (Larmore-Hirschberg package-merge)."""
    leaves = sorted((int(f), (i,)) for i, f in enumerate(freq) if f)
    n = len(leaves)
    assert n >= 2 and n <= 1 << limit
    packages = list(leaves)
    for _ in range(limit - 1):
        paired = [(packages[j][0] + packages[j + 1][0], packages[j][1] + packages[j + 1][1]) for j in range(0, len(packages) - 1, 2)]
        packages = sorted(leaves + paired, key=lambda p: p[0])
    length = {}
    for _, members in packages[:2 * n - 2]:
        for i in members:
            length[i] = length.get(i, 0) + 1
    assert sum(1 << (limit - l) for l in length.values()) == 1 << limit
    return sum(int(freq[i]) * l for i, l in length.items())


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def _vectors():
    g = np.random.default_rng(7)
    out = [("random 286", g.integers(1, 32769, 286)), ("random 286 with zeros", g.integers(0, 32769, 286) * (g.random(286) < 0.6)),
           ("all equal 286", np.full(286, 1000)), ("all equal 19", np.full(19, 3)), ("one", np.eye(286, dtype=np.int64)[77] * 12),
           ("two", np.eye(286, dtype=np.int64)[3] * 5 + np.eye(286, dtype=np.int64)[256]), ("fibonacci 22", np.array(_fib(22) + [0] * 264)),
           ("fibonacci 22 shuffled", g.permutation(np.array(_fib(22) + [0] * 10))), ("random 19", g.integers(0, 32769, 19)),
           ("skewed 19", np.array([30000, 1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 0, 0, 1, 1, 1, 9000])), ("all equal 128", np.full(128, 7)),
           ("all equal 100", np.full(100, 7))]
    return out


@pytest.mark.parametrize("limit", [15, 7])
def test_code_lengths(capi, limit):
    """Zero count -> 0; every length <= limit; Kraft sum exactly 1 with two or more symbols; one symbol -> length 1; the Huffman optimum
    whenever the unconstrained depth fits the limit; elsewhere Kraft and the limit (the cost against package-merge is in the module
    docstring and printed here)."""
    limited = 0
    for name, freq in _vectors():
        used = int(np.count_nonzero(freq))
        rc, lens = _lengths(capi, freq, limit)
        if used > 1 << limit:
            assert rc == capi.E_INVALID, name                               # 286 symbols cannot have 7-bit codes
            continue
        assert rc == capi.OK, name
        assert all((l == 0) == (f == 0) for l, f in zip(lens, freq)), name
        assert max(lens) <= limit, name
        if used == 1:
            assert sorted(lens)[-2:] == [0, 1], name
            continue
        assert _png.kraft(lens) == 1 << 15, name
        cost = sum(int(f) * l for f, l in zip(freq, lens))
        best, depth = _huffman(freq)
        if depth <= limit:
            assert cost == best, (name, cost, best)
        else:
            limited += 1
            optimum = _package_merge(freq, limit)
            print(f"limit {limit}, {name}: this routine {cost}, package-merge {optimum}, unlimited Huffman {best} (depth {depth})")
            assert cost >= optimum >= best, name
    assert limited >= (2 if limit == 7 else 2)                              # the Fibonacci vectors need limiting at both limits
    # deterministic, and no more than the counts matter
    a, b = _lengths(capi, _vectors()[0][1], limit), _lengths(capi, _vectors()[0][1], limit)
    assert a == b
    assert capi.lib().inerf_png_code_lengths(None, 4, limit, None) == capi.E_INVALID
    four = (C.c_uint32 * 4)(1, 2, 3, 4)
    out = (C.c_ubyte * 4)()
    for n, lim in ((0, limit), (289, limit), (4, 0), (4, 16)):
        assert capi.lib().inerf_png_code_lengths(four, n, lim, out) == capi.E_INVALID


# ---- the launcher ------------------------------------------------------------------------------------------------------------------
def test_launcher_switch_implies_frame_products(monkeypatch):
    from intrinsicnerf_amd import _capi, frames, launch
    seen = []

    def fake(*a, **kw):
        seen.append((a, kw))
        import types
        return types.ModuleType("m"), compile("", "x", "exec")

    monkeypatch.setattr(launch, "prepare", fake)
    monkeypatch.setattr(_capi, "lib", lambda: None)
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    launch.main(["train_SSR_main.py", "--inerf-render-path", "--inerf-frame-png", "--config_file", "x.yaml"])
    assert seen[-1] == (("train_SSR_main.py", True, False, False), {"frame_products": True, "frame_png": True}) and sys.argv[1:] == ["--config_file", "x.yaml"]
    launch.main(["run_nerf.py", "--inerf-render-path", "--inerf-frame-products"])
    assert seen[-1] == (("run_nerf.py", True, False, False), {"frame_products": True})    # without the switch the call is what it was
    assert "--inerf-frame-png" in launch.__doc__
    ns = {"create_nerf": lambda: None}
    launch.rebind_object_level(ns, with_render_path=True, frame_png=True)
    assert isinstance(ns["render_path"].keywords["products"], frames.FrameProducts) and ns["render_path"].keywords["products"].encode
    ns = {"create_nerf": lambda: None, "Cluster_Manager": object}
    launch.rebind_object_level(ns, with_render_path=True, frame_products=True)
    assert not ns["render_path"].keywords["products"].encode
    assert frames.FrameProducts().encode is False
