"""GPU: baseline JPEG files and Motion-JPEG AVI files made on the device (csrc/jpeg.hip).  Every case asserts that the device's file
equals the numpy model's file (_jpeg.py) BYTE FOR BYTE and that Pillow decodes it.  Shapes, each the smallest at which its mechanism
can go wrong: 1 x 1 grey (everything is padding), 8 x 8 colour (one MCU, no restart), 9 x 17 colour (both edges partial, three MCU
rows), 16 x 24 grey, 72 x 8 grey (nine MCU rows: RSTm wraps past 7), 8 x 264 colour (one MCU more than the kernel's chunk of 32: the
carry of predictors and bit position), 240 x 320 colour.  Contents: all 0 and all 255, a pixel checkerboard, a block with AC
coefficients only at zigzag 20, 40 and 63 (ZRL, no EOB), a ramp, white noise at quality 100 (the longest codes, FF bytes to stuff).
Then sixteen images in one call, determinism, sentinels, the arena's cursor and index, overflow, graph replay, the Python entry points
and both ``render_path`` front-ends."""
import io
import os

import numpy as np
import pytest
import torch

import _avi
import _jpeg

pytestmark = pytest.mark.gpu
GUARD = 0xA5
TAIL = 64


def _dev():
    return torch.device("cuda:0")


def _pillow(data, image):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (image.shape[1], image.shape[0]) and im.mode == ("L" if image.ndim == 2 else "RGB")
    return np.array(im)


def _run(items, capacity=None):
    """One ``inerf_jpeg_encode`` call over ``items`` = [(image, quality)], every image into a stream of its own whose arena, index and
    workspace are followed by sentinels.  Checks the sentinels and returns [(file bytes, stream)]."""
    from intrinsicnerf_amd import kernels
    dev = _dev()
    raw, specs, at = [], [], 0
    for image, quality in items:
        h, w = image.shape[:2]
        c = 1 if image.ndim == 2 else 3
        specs.append((h, w, c, quality, at))
        data = image.tobytes() + b"\xee" * (-image.size % 16)
        raw.append(data)
        at += len(data)
    src = torch.from_numpy(np.frombuffer(b"".join(raw), np.uint8).copy()).to(dev)
    plan = kernels.jpeg_plan(specs)
    streams = []
    for h, w, c, quality, _ in specs:
        s = kernels.JpegStream(h, w, c, quality, capacity or kernels.jpeg_frame_bound(h, w, c), 2, dev, tail=TAIL)
        s.arena[s.capacity:] = GUARD
        s.index[s.frames:] = -7
        streams.append(s)
    workspace = torch.full((plan[1] + TAIL,), GUARD, dtype=torch.uint8, device=dev)
    kernels.jpeg_encode(src, plan, streams, workspace=workspace)
    assert (workspace[plan[1]:] == GUARD).all(), "bytes behind the workspace were written"
    out = []
    for s in streams:
        assert (s.arena[s.capacity:] == GUARD).all(), "bytes behind the arena were written"
        assert (s.index[s.frames:] == -7).all(), "entries behind the index were written"
        state = s.state.cpu().numpy()
        used, frames, status, offset, size = (int(v) for v in state[:5])
        assert (frames, status, offset) == (1, 0, 0) and used == 8 + size + (size & 1) <= s.capacity, state[:5]
        chunk = s.arena[:used].cpu().numpy().tobytes()
        assert chunk[:4] == b"00dc" and int.from_bytes(chunk[4:8], "little") == size and (not size & 1 or chunk[-1] == 0)
        out.append((chunk[8:8 + size], s))
    return out


CASES = _jpeg.cases()


def test_every_shape_and_content_equals_the_model_byte_for_byte():
    """All 38 cases in three calls of up to 16 images."""
    stuffed = 0
    for start in range(0, len(CASES), 16):
        batch = CASES[start:start + 16]
        for (name, image, quality), (data, _) in zip(batch, _run([(image, quality) for _, image, quality in batch])):
            want = _jpeg.model_file(name, image, quality)
            assert len(data) == len(want) and data == want, f"{name}: the device's file differs from the model's " \
                f"(first at byte {next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), min(len(data), len(want)))} of {len(want)})"
            _pillow(data, image)
            if name.startswith("noise-240"):
                stuffed = data.count(b"\xff\x00")
    assert stuffed >= 1, "the white-noise file holds no stuffed FF 00"


def test_sixteen_mixed_images_in_one_call_and_two_runs_give_the_same_bytes():
    g = np.random.default_rng(5)
    shapes = [(9, 17, 3), (16, 24), (1, 1), (8, 264, 3), (33, 70), (72, 8), (8, 8, 3), (25, 31, 3)] * 2
    items = [(g.integers(0, 256, s).astype(np.uint8) if k % 3 else _jpeg.content("ramp", s), (100, 90, 35)[k % 3]) for k, s in enumerate(shapes)]
    first = [d for d, _ in _run(items)]
    for (image, quality), data in zip(items, first):
        assert data == _jpeg.encode(image, quality)
        _pillow(data, image)
    assert [d for d, _ in _run(items)] == first


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def test_three_adds_append_three_chunks(tmp_path):
    from intrinsicnerf_amd import frames
    dev = _dev()
    images = [_noise((20, 28, 3), k) for k in range(3)]
    w = frames.MovieWriter(str(tmp_path / "m.avi"), (20, 28), 3, fps=25, quality=80, frames=4, bytes_per_sample=None, device=dev)
    for image in images:
        w.add(torch.from_numpy(image).to(dev))
    state = w.stream.state.cpu().numpy()
    files = [_jpeg.encode(image, 80) for image in images]
    at = 0
    for k, data in enumerate(files):
        assert tuple(state[3 + 2 * k:5 + 2 * k]) == (at, len(data))
        at += 8 + len(data) + (len(data) & 1)
    assert tuple(state[:3]) == (at, 3, 0)
    w.close()
    data = (tmp_path / "m.avi").read_bytes()
    assert _avi.check(data, 3, 28, 20, 25) == files
    info = _avi.parse(data)
    assert data[info["movi_at"] + 4:info["movi_at"] + 4 + at] == w.stream.arena[:at].cpu().numpy().tobytes()       # the arena, verbatim


def test_a_frame_that_does_not_fit_is_refused(tmp_path):
    """An arena with room for one frame of noise (and 38 .. 40 bytes more) takes the first and refuses the second."""
    from intrinsicnerf_amd import frames, kernels
    dev = _dev()
    a, b = _noise((24, 24), 1), _noise((24, 24), 2)
    fa, fb = _jpeg.encode(a, 100), _jpeg.encode(b, 100)
    chunk = lambda f: 8 + len(f) + (len(f) & 1)
    header = len(kernels.jpeg_header(24, 24, 1, 100))
    w = frames.MovieWriter(str(tmp_path / "m.avi"), (24, 24), 1, quality=100, frames=2, device=dev, _tail=TAIL,
                           bytes_per_sample=((chunk(fa) + 40) / 2 - header) / 576)
    assert chunk(fa) <= w.stream.capacity < chunk(fa) + chunk(fb)
    w.stream.arena[:] = GUARD
    w.add(torch.from_numpy(a).to(dev))
    w.add(torch.from_numpy(b).to(dev))
    state = w.stream.state.cpu().numpy()
    assert tuple(state[:2]) == (chunk(fa), 1), "the cursor moved for the refused frame"
    assert int(state[2]) == chunk(fa) + chunk(fb), "the status word does not hold the capacity that was needed"
    arena = w.stream.arena.cpu().numpy()
    assert arena[8:8 + len(fa)].tobytes() == fa and (arena[chunk(fa):] == GUARD).all(), "bytes of the refused frame were written"
    with pytest.raises(RuntimeError, match=str(chunk(fa) + chunk(fb))):
        w.close()
    assert not (tmp_path / "m.avi").exists()


def test_a_captured_call_replayed_three_times_appends_three_frames():
    from intrinsicnerf_amd import kernels
    dev = _dev()
    images = [_jpeg.content("ramp", (24, 40, 3)), _noise((24, 40, 3), 3), _jpeg.content("checker", (24, 40, 3))]
    plan = kernels.jpeg_plan([(24, 40, 3, 90, 0)])
    stream = kernels.JpegStream(24, 40, 3, 90, 4 * kernels.jpeg_frame_bound(24, 40, 3), 4, dev)
    workspace = torch.empty(plan[1], dtype=torch.uint8, device=dev)
    src = torch.from_numpy(images[0].reshape(-1)).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        kernels.jpeg_encode(src, plan, [stream], workspace=workspace)          # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    stream.state.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.jpeg_encode(src, plan, [stream], workspace=workspace)
    for image in images:
        src.copy_(torch.from_numpy(image.reshape(-1)).to(dev))
        graph.replay()
    torch.cuda.synchronize()
    state = stream.state.cpu().numpy()
    assert tuple(state[1:3]) == (3, 0)
    arena = stream.arena.cpu().numpy()
    files = [arena[int(o) + 8:int(o) + 8 + int(n)].tobytes() for o, n in state[3:9].reshape(3, 2)]
    assert files == [_jpeg.encode(image, 90) for image in images] and len(set(files)) == 3


def test_encode_jpeg_and_its_errors():
    from intrinsicnerf_amd import frames
    dev = _dev()
    for image in (_jpeg.content("ramp", (37, 53)), _noise((37, 53, 3), 4)):
        data = frames.encode_jpeg(torch.from_numpy(image).to(dev), quality=75)
        assert isinstance(data, bytes) and data == _jpeg.encode(image, 75)
        _pillow(data, image)
    assert frames.encode_jpeg(torch.from_numpy(_noise((9, 9), 1)).to(dev)) == _jpeg.encode(_noise((9, 9), 1), 90)
    with pytest.raises(TypeError):
        frames.encode_jpeg(np.zeros((4, 4), np.uint8))
    with pytest.raises(RuntimeError):
        frames.encode_jpeg(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        frames.encode_jpeg(torch.zeros(4, 4, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        frames.encode_jpeg(torch.zeros(4, 4, 2, dtype=torch.uint8, device=dev))
    if hasattr(torch, "uint16"):
        with pytest.raises(ValueError):
            frames.encode_jpeg(torch.zeros(4, 4, dtype=torch.int16, device=dev).view(torch.uint16))


def test_write_movie_on_a_colour_and_a_grey_stack(tmp_path):
    from intrinsicnerf_amd import frames
    colour = np.stack([_noise((24, 40, 3), k) if k & 1 else _jpeg.content("ramp", (24, 40, 3)) for k in range(5)])
    path = frames.write_movie(str(tmp_path / "c.avi"), colour, fps=30, quality=90)
    files = _avi.check(open(path, "rb").read(), 5, 40, 24, 30)
    assert files == [_jpeg.encode(f, 90) for f in colour]
    grey = np.stack([_noise((9, 17), k) for k in range(3)])
    path = frames.write_movie(str(tmp_path / "g.avi"), torch.from_numpy(grey).to(_dev()), fps=12, quality=60)
    files = _avi.check(open(path, "rb").read(), 3, 17, 9, 12)
    assert files == [_jpeg.encode(f, 60) for f in grey]
    for f, image in zip(files, grey):
        _pillow(f, image)
    # more frames than one call takes: two batches, one arena used twice
    many = np.stack([_noise((8, 8), k) for k in range(19)])
    files = _avi.check(open(frames.write_movie(str(tmp_path / "m.avi"), many), "rb").read(), 19, 8, 8, 30)
    assert files == [_jpeg.encode(f, 90) for f in many]


def test_the_launcher_proxy_writes_an_avi_file_at_quality_90(tmp_path):
    from intrinsicnerf_amd import launch
    stack = np.stack([_noise((16, 24, 3), k) for k in range(2)])
    proxy = launch.movie_proxy()
    assert launch.movie_quality(8) == 90 and launch.movie_quality(10) == 100
    proxy.mimwrite(str(tmp_path / "x.mp4"), stack, fps=30, quality=8)
    assert not (tmp_path / "x.mp4").exists()
    files = _avi.check((tmp_path / "x.avi").read_bytes(), 2, 24, 16, 30)
    assert files == [_jpeg.encode(f, 90) for f in stack]


def test_ssr_render_path_writes_movies(tmp_path):
    """The SSR front-end built as tests/test_png_gpu.py builds it: one frame per pose in every file, each frame ``encode_jpeg`` of the
    same product's image, and the pass returns what it returns without ``movies=``."""
    import _png
    from intrinsicnerf_amd import frames, ssr
    from oracle import calibration as cal
    dev = _dev()
    H, W, C, N = 12, 17, 5, 3
    r = ssr.SSRRenderer(C, white_bkgd=False, chunk=100, device=dev)
    r.H_scaled, r.W_scaled, r.near, r.far = H, W, 0.1, 10.0
    r.check_numerics = False
    T = torch.eye(4)[None].repeat(N, 1, 1)
    T[1, :3, 3], T[2, :3, 3] = torch.tensor([0.2, 0.0, 0.1]), torch.tensor([-0.3, 0.1, 0.0])
    rays = ssr.create_rays(N, T.to(dev), H, W, 8.0, 8.0, (W - 1) / 2.0, (H - 1) / 2.0, 0.1, 10.0)
    r.ssr_net_coarse.load_state_dict(cal.calibrated_default_init("ssr", C, 0, rays[0].cpu()))
    r.ssr_net_fine.load_state_dict(cal.calibrated_default_init("ssr", C, 1, rays[0].cpu()))
    r.valid_colour_map = (torch.arange(C * 3, dtype=torch.uint8).reshape(C, 3) * 17 + 3).to(dev)
    names = ("rgb", "albedo", "vis_depth", "entropy", "vis_label")
    (tmp_path / "planes").mkdir()
    with torch.no_grad():
        r.frame_products = frames.FrameProducts()
        base = r.render_path(rays, save_dir=str(tmp_path / "planes"))
        r.frame_products = frames.FrameProducts(movies={n: str(tmp_path / f"{n}.avi") for n in names}, fps=24, quality=85)
        out = r.render_path(rays)
        r.frame_products = frames.FrameProducts(movies={"depth": str(tmp_path / "d.avi")})          # a u16 product
        with pytest.raises(ValueError):
            r.render_path(rays)
    assert len(out) == len(base) == 12
    for a, b in zip(out[:11], base[:11]):
        assert (a is None) == (b is None)
        if b is not None:
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    for n in names:
        files = _avi.check((tmp_path / f"{n}.avi").read_bytes(), N, W, H, 24)
        for i, f in enumerate(files):
            plane = _png.decode((tmp_path / "planes" / f"{n}_{i:03d}.png").read_bytes())             # the same product's image
            assert f == frames.encode_jpeg(torch.from_numpy(np.ascontiguousarray(plane)).to(dev), quality=85), (n, i)
            assert f == _jpeg.encode(plane, 85)
            _pillow(f, plane)


def test_object_render_path_writes_movies(tmp_path):
    import bench
    from intrinsicnerf_amd import frames, object_level as ol
    from test_frame_products_gpu import _chair_nets
    dev = _dev()
    side = 45
    K, focal, kw = _chair_nets(dev, side)
    poses = torch.stack([torch.cat([bench.chair_pose(theta_deg=t), torch.tensor([[0., 0., 0., 1.]])], 0) for t in (20., 130.)]).to(dev)
    (tmp_path / "planes").mkdir()
    movies = {"": str(tmp_path / "rgb.avi"), "a": str(tmp_path / "albedo.avi"), "acc": str(tmp_path / "acc.avi")}
    with torch.no_grad():
        rgbs0, disps0, _ = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, savedir=str(tmp_path / "planes"), products=frames.FrameProducts())
        rgbs1, disps1, _ = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, products=frames.FrameProducts(movies=movies, fps=30, quality=90))
        rgbs2, disps2, _ = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw)
    assert np.array_equal(rgbs1, rgbs0) and np.array_equal(disps1, disps0, equal_nan=True)
    assert np.array_equal(rgbs2, rgbs0) and np.array_equal(disps2, disps0, equal_nan=True)
    import _png
    for prefix, path in movies.items():
        files = _avi.check(open(path, "rb").read(), 2, side, side, 30)
        for i, f in enumerate(files):
            plane = _png.decode((tmp_path / "planes" / f"{prefix}{i:03d}.png").read_bytes())       # the same product's image
            assert f == frames.encode_jpeg(torch.from_numpy(np.ascontiguousarray(plane)).to(dev), quality=90), (prefix, i)
            assert f == _jpeg.encode(plane, 90)
