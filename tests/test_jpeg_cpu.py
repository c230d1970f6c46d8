"""JPEG and Motion-JPEG AVI without a device: the library's host-only entry points (tables, header, sizes, every argument check of
``inerf_jpeg_encode`` with made-up pointers - decided before any HIP call), the numpy model of tests/_jpeg.py against Pillow, the
marker structure of its files and the container code of ``frames.MovieWriter`` through its host-side seam ``frames.avi_bytes``.

Measured here (profiles/frame_movies.txt has every figure): Pillow's decoder stays within 0.56 levels (grey; bound 1.5) and 1.89 levels
(colour; bound 5) of ``reconstruct(..., limit=True)`` over all 38 cases.  ``limit=True`` clamps the component planes where a decoder's
range limit does: the derivation's "clamping does not enlarge it" holds only when both sides clamp at the same place (with
unclamped planes white noise at quality 75 differs by 9 levels, none of it the decoder's error)."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import _avi
import _jpeg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Image = pytest.importorskip("PIL.Image")


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
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version() and header >= 40027
    for name in ("inerf_jpeg_workspace_bytes", "inerf_jpeg_frame_bound", "inerf_jpeg_encode", "inerf_jpeg_tables", "inerf_jpeg_header"):
        assert name in capi.SYMBOLS and re.search(r"\b%s\(" % name, text)
    assert re.search(r"#define INERF_JPEG_MAX_IMAGES\s+%d\b" % capi.JPEG_MAX_IMAGES, text) and capi.JPEG_MAX_IMAGES == 16
    for struct, mirror in (("inerf_jpeg_image", capi.JpegImage), ("inerf_jpeg_args", capi.JpegArgs)):
        body = text[text.index("typedef struct %s {" % struct):text.index("} %s;" % struct)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"([a-z_0-9]+)(?:\[INERF_JPEG_MAX_IMAGES\])?\s*;", body) == [f[0] for f in mirror._fields_]
    assert C.sizeof(capi.JpegImage) == 88 and C.sizeof(capi.JpegArgs) == 40 + 16 * 88
    from intrinsicnerf_amd import _build
    assert "jpeg.hip" in _build.SOURCES and any(h.endswith("jpeg_tables.h") for h in _build.HEADERS)


def _pillow_tables(quality, colour):
    a = np.zeros((8, 8, 3) if colour else (8, 8), np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=0)
    return Image.open(io.BytesIO(buf.getvalue())).quantization


@pytest.mark.parametrize("quality", [1, 10, 49, 50, 75, 90, 95, 100])
def test_tables_equal_pillows(capi, quality):
    from intrinsicnerf_amd import kernels
    luma, chroma = kernels.jpeg_tables(quality)
    want = _pillow_tables(quality, True)
    assert luma.tolist() == list(want[0]) and chroma.tolist() == list(want[1])
    assert luma.tolist() == list(_pillow_tables(quality, False)[0])
    model = _jpeg.tables(quality)
    assert luma.tolist() == model[0].tolist() and chroma.tolist() == model[1].tolist()


def test_header_equals_the_models_byte_for_byte(capi):
    from intrinsicnerf_amd import kernels
    for channels in (1, 3):
        for h, w in ((1, 1), (9, 17), (240, 320)):
            for quality in (35, 90):
                got = kernels.jpeg_header(h, w, channels, quality)
                assert got == _jpeg.header(h, w, channels, quality) and len(got) == (334 if channels == 1 else 629)
    # the Huffman tables are the ones Pillow's libjpeg writes (T.81 Annex K)
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, "JPEG", quality=50, subsampling=0)
    theirs = sorted(p for m, p in _jpeg.walk(buf.getvalue())[0] if m == 0xc4)
    ours = sorted(p for m, p in _jpeg.walk(_jpeg.encode(np.zeros((8, 8, 3), np.uint8), 50))[0] if m == 0xc4)
    assert ours == theirs and len(ours) == 4


CASES = _jpeg.cases()
_measured = {}


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_pillow_decodes_every_model_file_within_the_derived_bound(k):
    """1.5 levels for grey: a conforming integer IDCT is within 1 of the rounded ideal, so within 1.5 of the unrounded one.  5 for
    colour: the conversion adds at most 1.772 * 1.5 + 0.5.  Both sides clamp at the same places (module docstring)."""
    name, image, quality = CASES[k]
    data = _jpeg.model_file(name, image, quality)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (image.shape[1], image.shape[0]) and im.mode == ("L" if image.ndim == 2 else "RGB")
    err = float(np.abs(np.array(im).astype(np.float64) - _jpeg.reconstruct(image, quality, limit=True)).max())
    _measured[name] = err
    print(f"{name}: max |Pillow - reconstruct| = {err:.4f}")
    assert err <= (1.5 if image.ndim == 2 else 5.0), (name, err)


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


# The largest shortfall measured over these inputs (profiles/frame_movies.txt): 0.0135 dB; twice that is below the floor of 0.05 dB.
PSNR_MARGIN = 0.05


@pytest.mark.parametrize("kind,quality", [("smooth", 90), ("smooth", 50), ("noise", 90), ("noise", 50)])
@pytest.mark.parametrize("colour", [False, True])
def test_decoded_psnr_against_pillows_own_encoder(kind, quality, colour):
    shape = (64, 96, 3) if colour else (64, 96)
    if kind == "smooth":
        y, x = np.mgrid[0:64, 0:96]
        a = 128 + 90 * np.sin(x / 11.0) * np.cos(y / 7.0)
        image = (np.stack([a, a[::-1], 255 - a], -1) if colour else a).astype(np.uint8)
    else:
        image = np.random.default_rng(7).integers(0, 256, shape).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, "JPEG", quality=quality, subsampling=0)
    theirs = _psnr(np.array(Image.open(io.BytesIO(buf.getvalue()))), image)
    ours = _psnr(np.array(Image.open(io.BytesIO(_jpeg.encode(image, quality)))), image)
    print(f"{kind} {'colour' if colour else 'grey'} q{quality}: model {ours:.4f} dB, Pillow {theirs:.4f} dB, shortfall {theirs - ours:+.4f} dB")
    assert ours >= theirs - PSNR_MARGIN


def test_marker_structure():
    for name, image, quality in CASES:
        data = _jpeg.model_file(name, image, quality)
        segments, intervals, restarts = _jpeg.walk(data)
        colour = image.ndim == 3
        assert [m for m, _ in segments] == [0xd8, 0xe0] + [0xdb] * (2 if colour else 1) + [0xc0] + [0xc4] * (4 if colour else 2) + [0xdd, 0xda, 0xd9], name
        dri = [p for m, p in segments if m == 0xdd][0]
        rows, mcus = (image.shape[0] + 7) // 8, (image.shape[1] + 7) // 8
        assert int.from_bytes(dri, "big") == mcus
        assert len(intervals) == rows and restarts == [r % 8 for r in range(rows - 1)]
        for part in intervals:
            assert len(part) > 0 and all(part[i + 1] == 0 for i in range(len(part) - 1) if part[i] == 0xff) and part[-1] != 0xff, name
    noisy = _jpeg.model_file(*[c for c in CASES if c[0].startswith("noise-240")][0])
    assert noisy.count(b"\xff\x00") >= 1
    sparse = _jpeg.quantised(_jpeg.sparse_block(), 50).reshape(64)[_jpeg.ZZ]
    assert np.nonzero(sparse)[0].tolist() == [20, 40, 63]              # a run of 19 zeros (ZRL) and no EOB


@pytest.mark.parametrize("fps", [30, 24, 12.5])
def test_the_container_holds_what_it_says(capi, fps):
    from intrinsicnerf_amd import frames
    images = [_jpeg.content("ramp", (9, 17, 3)), _jpeg.content("noise", (9, 17, 3), 3), _jpeg.content("checker", (9, 17, 3))]
    files = [_jpeg.encode(image, 90) for image in images]
    files.append(files[0] + b"")                                                # a fourth frame: 4 chunks
    data = frames.avi_bytes(files, 17, 9, fps)
    assert _avi.check(data, 4, 17, 9, fps) == files
    for f, image in zip(_avi.parse(data)["frames"], images):
        im = Image.open(io.BytesIO(f[1]))
        im.load()
        assert im.size == (17, 9) and im.mode == "RGB"
    odd = [b"\xff\xd8" + b"\x00" * k + b"\xff\xd9" for k in (1, 2, 3)]          # odd and even chunk lengths: every chunk stays even-aligned
    assert _avi.check(frames.avi_bytes(odd, 8, 8, fps), 3, 8, 8, fps) == odd
    with pytest.raises(ValueError):
        frames.avi_head([(0, 10)], 1 << 32, 8, 8, 30)                           # 4 GiB: OpenDML is not written


def _args(capi, n=1, **over):
    a = capi.JpegArgs()
    a.n_images = n
    a.src, a.src_bytes = 0x10000, 1 << 20
    a.workspace, a.workspace_bytes = 0x7f0000000000, 1 << 40
    for k in range(max(min(n, 16), 0)):
        im = a.images[k]
        im.height, im.width, im.channels, im.quality, im.src_offset = 16, 24, 3, 90, 0
        im.header, im.header_bytes = 0x20000, 629
        im.arena, im.arena_bytes = 0x30000, 1 << 20
        im.cursor, im.index, im.index_frames, im.status = 0x40000, 0x50000, 4, 0x60000
    for key, value in over.items():
        target = a.images[0] if hasattr(a.images[0], key) and not hasattr(capi.JpegArgs, key) else a
        setattr(target, key, value)
    return a


def test_every_argument_check_comes_before_any_hip_call(capi):
    """Made-up pointers and no device: a check that let one of these through would fault or report a HIP error, not INERF_E_INVALID."""
    lib = capi.lib()
    bad = [dict(n_images=17), dict(n_images=-1), dict(channels=2), dict(channels=4), dict(quality=0), dict(quality=101), dict(height=0),
           dict(width=0), dict(height=65536), dict(width=65536), dict(src=None), dict(src_bytes=-1), dict(src_offset=-1),
           dict(src_offset=(1 << 20) - 100), dict(header=None), dict(header_bytes=334), dict(arena=None), dict(arena_bytes=628),
           dict(cursor=None), dict(cursor=0x40004), dict(index=None), dict(index=0x50004), dict(index_frames=0), dict(status=None),
           dict(status=0x60002), dict(workspace=0x7f0000000008)]
    for over in bad:
        n = over.pop("n_images", 1)
        assert lib.inerf_jpeg_encode(C.byref(_args(capi, n, **over)), None) == capi.E_INVALID, over
    assert lib.inerf_jpeg_encode(None, None) == capi.E_INVALID
    assert lib.inerf_jpeg_encode(C.byref(_args(capi, workspace=None)), None) == capi.E_WORKSPACE
    assert lib.inerf_jpeg_encode(C.byref(_args(capi, workspace_bytes=1000)), None) == capi.E_WORKSPACE
    assert lib.inerf_jpeg_encode(C.byref(_args(capi, 0)), None) == capi.OK                    # nothing to do, nothing launched
    for over in (dict(n_images=17), dict(channels=2), dict(quality=0), dict(quality=101), dict(height=0), dict(width=65536)):
        n = over.pop("n_images", 1)
        assert lib.inerf_jpeg_workspace_bytes(C.byref(_args(capi, n, **over))) == capi.E_INVALID
    # 256 + 2 MCU rows * 16 + 2 slots of (3 MCUs * 3 blocks * 416 + 2 -> 3760) bytes
    assert lib.inerf_jpeg_workspace_bytes(C.byref(_args(capi))) == 256 + 2 * 16 + 2 * 3760
    assert lib.inerf_jpeg_frame_bound(16, 24, 3) == 8 + 629 + 2 * (9 * 416 + 2) + 2 + 1
    assert lib.inerf_jpeg_frame_bound(0, 24, 3) == lib.inerf_jpeg_frame_bound(16, 24, 2) == lib.inerf_jpeg_frame_bound(16, 70000, 1) == capi.E_INVALID
    buf = (C.c_ubyte * 700)()
    assert lib.inerf_jpeg_header(16, 24, 3, 90, buf, 628) == capi.E_INVALID and lib.inerf_jpeg_header(16, 24, 3, 90, buf, 629) == 629
    assert lib.inerf_jpeg_header(16, 24, 3, 0, buf, 700) == lib.inerf_jpeg_header(16, 24, 2, 90, buf, 700) == capi.E_INVALID
    assert lib.inerf_jpeg_header(16, 24, 3, 90, None, 700) == capi.E_INVALID
    assert lib.inerf_jpeg_tables(0, buf, buf) == lib.inerf_jpeg_tables(101, buf, buf) == lib.inerf_jpeg_tables(50, None, buf) == capi.E_INVALID
    # the model's files never exceed the bound the arena is sized by
    for name, image, quality in CASES:
        c = 1 if image.ndim == 2 else 3
        assert 8 + len(_jpeg.model_file(name, image, quality)) + 1 <= lib.inerf_jpeg_frame_bound(image.shape[0], image.shape[1], c)


def test_python_entry_points_refuse_without_a_device(capi):
    import torch
    from intrinsicnerf_amd import frames, launch
    with pytest.raises(TypeError):
        frames.encode_jpeg(np.zeros((4, 4), np.uint8))
    with pytest.raises(RuntimeError):
        frames.encode_jpeg(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        frames.MovieWriter("x.avi", (8, 8), 1, device="cpu")
    assert [launch.movie_quality(q) for q in (0, 5, 8, 10, None)] == [50, 75, 90, 100, 75]
    with pytest.raises(ValueError):
        launch.movie_quality(11)
    proxy = launch.movie_proxy(np)                      # any module stands for "the real one": other attributes forward
    assert proxy.zeros is np.zeros and callable(proxy.mimwrite)
    with pytest.raises(AttributeError):
        launch.movie_proxy(None).imread
