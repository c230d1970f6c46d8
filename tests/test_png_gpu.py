"""GPU: PNG files encoded on the device (csrc/png.hip).  Every file is decoded by the plain Python decoder of _png.py - every CRC,
the Adler-32, the inflated length, the filter bytes - to exactly the source plane, with sentinels around every file's
[dst_offset, dst_offset + dst_capacity) checked; the DEFLATE block walker of _png.py shows segments, block types, matches and
code lengths.  Shapes: the smallest images, the segment boundaries (169 rows of 193 bytes fill a segment of a 64-wide RGB image),
the widest rows, an SSR frame's eleven products.  Contents: flat, runs of chosen lengths, white noise, a ramp, Fibonacci counts,
16-bit byte order.  Then determinism, graph capture and both ``render_path`` front-ends."""
import heapq
import os

import numpy as np
import pytest
import torch

import _png

pytestmark = pytest.mark.gpu
CAP = 32768
GUARD = 0xA5


def _dev():
    return torch.device("cuda:0")


def _pack(planes):
    """The planes side by side at multiples of 16 bytes, as ``inerf_frame_products`` lays them out: (bytes, specs)."""
    chunks, specs, at = [], [], 0
    for plane, flt in planes:
        a = np.ascontiguousarray(plane)
        depth = 16 if a.dtype == np.uint16 else 8
        assert a.dtype in (np.uint8, np.uint16)
        raw = a.astype("<u2").tobytes() if depth == 16 else a.tobytes()
        specs.append((a.shape[0], a.shape[1], 3 if a.ndim == 3 else 1, depth, at, flt))
        raw += b"\xee" * (-len(raw) % 16)
        chunks.append(raw)
        at += len(raw)
    return np.frombuffer(b"".join(chunks), np.uint8).copy(), specs


def _segments(plane):
    h, row = plane.shape[0], 1 + plane[0].size * plane.dtype.itemsize
    rows = CAP // row
    return [min(rows, h - r) * row for r in range(0, h, rows)]


def _encode(planes, check=True):
    """One call over ``planes`` = [(array, filter)] into a sentinel-filled buffer.  Checks the sentinels around every file's window,
    sizes[k] <= dst_capacity and - ``check`` - that file k decodes to plane k and is cut into the expected segments.  Returns
    [(file bytes, info)]."""
    from intrinsicnerf_amd import kernels
    dev = _dev()
    host, specs = _pack(planes)
    plan = kernels.png_plan(specs)
    _, files, total, _ = plan
    out = torch.full((total + 64,), GUARD, dtype=torch.uint8, device=dev)
    _, sizes = kernels.png_encode(torch.from_numpy(host).to(dev), plan, out=out)
    got, sizes = out.cpu().numpy(), sizes.cpu().numpy()
    end, result = 0, []
    for k, ((off, cap), (plane, _)) in enumerate(zip(files, planes)):
        assert (got[end:off] == GUARD).all(), f"bytes before file {k} were written"
        assert 0 < sizes[k] <= cap, (k, sizes[k], cap)
        end = off + cap
        data = got[off:off + int(sizes[k])].tobytes()
        if check:
            image, info = _png.decode(data, with_info=True)
            assert image.dtype == plane.dtype and image.shape == plane.shape and np.array_equal(image, plane), f"file {k} decodes to other pixels"
            assert info["n_idat"] == 1
            blocks = _png.blocks(info["zlib"][2:-4])
            assert [b["bytes"] for b in blocks if b["bytes"]] == _segments(plane), k       # one non-empty block per segment
            assert all(d == 1 for b in blocks for _, d in b["matches"]) and not any(b["leading_match"] for b in blocks)
            assert all(b["type"] in ("dynamic", "stored") for b in blocks) and blocks[-1]["final"] and blocks[-1]["bytes"] == 0
            assert all(b["end"] % 8 == 0 for b in blocks if b["type"] == "stored") and not any(b["final"] for b in blocks[:-1])
            assert all(b["start"] % 8 == 0 for b in blocks if b["bytes"] or b["final"])    # every segment starts, so ends, on a byte
            for b in blocks:
                if b["type"] == "dynamic":
                    assert len(b["litlen"]) >= 257 and len(b["dist"]) == 1 and b["repeats"] == 0
                    assert _png.kraft(b["litlen"]) == 1 << 15 and _png.kraft(b["cl"]) == 1 << 15 and max(b["cl"]) <= 7
            info["blocks"] = blocks
            result.append((data, info))
        else:
            result.append((data, None))
    assert (got[end:] == GUARD).all(), "bytes after the last file were written"
    return result


def _smooth(shape, dtype, seed):
    g = np.random.default_rng(seed)
    h, w = shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    top = 65535 if dtype == np.uint16 else 255
    base = (0.5 + 0.4 * np.sin(x / 9.0 + seed) * np.cos(y / 7.0)) * top
    if len(shape) == 3:
        base = np.stack([base, base * 0.7, top - base], -1)
    out = base + g.normal(0, top * 0.004, shape)
    out[: h // 4] = top // 3                                                 # a flat background band
    return np.clip(out, 0, top).astype(dtype)


def test_smallest_images_and_segment_boundaries():
    """1x1 grey, 1x1 RGB, 1x2 16-bit, 3x5 RGB; 64-wide RGB at the heights that fill exactly 1, 2 and 3 segments (169 rows each) and
    one row either side - thirteen files from one call."""
    g = np.random.default_rng(1)
    planes = [(g.integers(0, 256, (1, 1)).astype(np.uint8), -1), (g.integers(0, 256, (1, 1, 3)).astype(np.uint8), -1),
              (g.integers(0, 65536, (1, 2)).astype(np.uint16), -1), (g.integers(0, 256, (3, 5, 3)).astype(np.uint8), -1)]
    assert CAP // (1 + 64 * 3) == 169
    for h in (168, 169, 170, 337, 338, 339, 506, 507, 508):
        planes.append((_smooth((h, 64, 3), np.uint8, h), -1))
    files = _encode(planes)
    assert [len(_segments(p)) for p, _ in planes[4:]] == [1, 1, 2, 2, 2, 3, 3, 3, 4]
    for (data, info), (plane, _) in zip(files[4:], planes[4:]):
        assert len(data) < plane.size and any(b["type"] == "dynamic" for b in info["blocks"])
        assert info["filters"][0] == 1 and info["filters"][1] == 2         # the flat band: Sub on its first row (nothing above), Up below


def test_widest_rows():
    """A filtered row of capacity - 1 bytes, and one of exactly the capacity: the last that fits.  One row per segment."""
    from intrinsicnerf_amd import kernels
    g = np.random.default_rng(2)
    planes = []
    for w in (CAP - 2, CAP - 1):
        x = (np.arange(w) // 40 + g.integers(0, 3, (3, w))).astype(np.uint8)
        planes.append((x, -1))
    files = _encode(planes)
    for (data, info), (plane, _) in zip(files, planes):
        assert _segments(plane) == [plane.shape[1] + 1] * 3 and len(data) < plane.size // 2
    with pytest.raises(RuntimeError, match="unsupported"):
        kernels.png_plan([(3, CAP, 1, 8, 0)])


def test_an_ssr_frames_eleven_products_straight_from_frame_products():
    """rgb, albedo, shading, residual, disp, depth (16-bit), vis_depth (jet), label, entropy, vis_entropy (jet, own range), vis_label
    (palette) of a 24x32 frame: the encoder reads the buffer ``inerf_frame_products`` wrote, at the products' offsets."""
    from intrinsicnerf_amd import _capi as capi, kernels
    dev = _dev()
    H, W = 24, 32
    g = np.random.default_rng(3)
    y, x = np.mgrid[0:H, 0:W]
    cols = [0.5 + 0.4 * np.sin(x / 5.0 + c) * np.cos(y / 4.0 + 0.3 * c) for c in range(12)]
    pack = np.stack(cols, -1).reshape(H * W, 12).astype(np.float32) + g.normal(0, 0.01, (H * W, 12)).astype(np.float32)
    pack[:, 9] = np.abs(pack[:, 9]) * 40000.0                           # disparity
    pack[:, 10] = 0.5 + np.abs(pack[:, 10]) * 6.0                            # depth in metres
    pack[:, 11] = np.floor(np.abs(pack[:, 11]) * 6.0)                        # labels 0 .. 5
    frame = torch.from_numpy(pack).to(dev)
    palette = torch.from_numpy(g.integers(0, 256, (5, 3)).astype(np.uint8)).to(dev)
    rng = kernels.frame_range(frame[:, 8])
    specs = [(capi.FRAME_TO8B, 0, 3, 0., 0., None), (capi.FRAME_TO8B, 3, 3, 0., 0., None), (capi.FRAME_TO8B, 6, 1, 0., 0., None),
             (capi.FRAME_TO8B, 5, 3, 0., 0., None), (capi.FRAME_U16, 9, 1, 1.0, 0., None), (capi.FRAME_U16, 10, 1, 1000.0, 0., None),
             (capi.FRAME_JET, 10, 1, 0.1, 10.0, None), (capi.FRAME_U8_CAST, 11, 1, 0., 0., None), (capi.FRAME_TO8B, 8, 1, 0., 0., None),
             (capi.FRAME_JET, 8, 1, 0., 0., rng), (capi.FRAME_PALETTE, 11, 1, 0., 0., None)]
    planes_buf, planes = kernels.frame_products(frame, specs, palette=palette)
    images = []
    for (kind, _, width, *_), (off, size) in zip(specs, planes):
        rgb = kind in (capi.FRAME_JET, capi.FRAME_PALETTE) or width == 3
        images.append((H, W, 3 if rgb else 1, 16 if kind == capi.FRAME_U16 else 8, off))
    plan = kernels.png_plan(images)
    out = torch.full((plan[2] + 64,), GUARD, dtype=torch.uint8, device=dev)
    _, sizes = kernels.png_encode(planes_buf, plan, out=out)
    got, sizes, src = out.cpu().numpy(), sizes.cpu().numpy(), planes_buf.cpu().numpy()
    end = 0
    for k, ((off, cap), (h, w, c, depth, src_off)) in enumerate(zip(plan[1], images)):
        assert (got[end:off] == GUARD).all() and 0 < sizes[k] <= cap
        end = off + cap
        image = _png.decode(got[off:off + int(sizes[k])].tobytes())
        raw = src[src_off:src_off + h * w * c * depth // 8]
        want = raw.view("<u2").reshape(h, w) if depth == 16 else (raw.reshape(h, w, 3) if c == 3 else raw.reshape(h, w))
        assert image.dtype == want.dtype and np.array_equal(image, want), k
    assert (got[end:] == GUARD).all()
    assert len({got[off:off + int(s)].tobytes() for (off, _), s in zip(plan[1], sizes)}) == 11


def test_flat_images_compress_to_runs_across_segments():
    """All zero and all 255, three segments and a row: 127 matches of 258 bytes per 32 KiB at 3 bits or fewer each plus a block
    header - a file below a fiftieth of the filtered bytes."""
    for value in (0, 255):
        plane = np.full((339, 64, 3), value, np.uint8)
        for flt in (0, -1):
            (data, info), = _encode([(plane, flt)])
            filtered = len(info["raw"])
            assert filtered == 339 * 193 and len(data) < filtered / 50, (value, flt, len(data))
            assert all(b["type"] == "dynamic" for b in info["blocks"] if b["bytes"])
            if (value, flt) == (0, 0):                                       # one run from the first byte to the last, cut by the segments alone
                assert all(l == 258 for b in info["blocks"] for l, _ in b["matches"][:-2])
                assert [sum(l for l, _ in b["matches"]) for b in info["blocks"] if b["bytes"]] == [n - 1 for n in _segments(plane)]
    (data, info), = _encode([(np.zeros((339, 64, 3), np.uint8), 0)])
    first = info["blocks"][0]
    used = [s for s, l in enumerate(first["litlen"]) if l]
    assert {0, 256} <= set(used) <= {0, 256} | set(range(257, 286))                      # one byte value: literal 0, end of block, lengths


def _expected_matches(run):
    if run < 4:
        return []
    q, r = divmod(run - 1, 258)
    if r == 0:
        return [258] * q
    if r >= 3:
        return [258] * q + [r]
    return [258] * (q - 1) + [258 - (3 - r), 3]


def test_runs_of_chosen_lengths_become_the_expected_matches():
    """filter = 0 and one row, so the filtered bytes are the row behind one 0: runs of 1 .. 5, 258 .. 262, 516 .. 520, 775 and 3000
    with another value between them.  A run of L >= 4 is a literal and matches over exactly L - 1 bytes, split as the header says;
    no tail of 1 or 2 bytes is left as literals."""
    runs = [3, 4, 5, 258, 259, 260, 261, 262, 1, 2, 6, 7, 516, 517, 518, 519, 520, 775, 3000, 4, 3, 259, 130, 126, 129]
    row, value = [], 10
    for run in runs:
        row += [value] * run
        value = value + 1 if value < 250 else 10
    plane = np.array(row, np.uint8)[None]
    assert plane.size + 1 <= CAP and (np.diff(plane[0]) != 0).sum() == len(runs) - 1
    (data, info), = _encode([(plane, 0)])
    block = info["blocks"][0]
    assert block["type"] == "dynamic" and block["bytes"] == plane.size + 1
    want = [m for run in runs for m in _expected_matches(run)]
    assert [l for l, _ in block["matches"]] == want
    for run in (3, 4, 5, 258, 259, 260, 261, 262):
        assert sum(_expected_matches(run)) == (run - 1 if run >= 4 else 0) and all(3 <= m <= 258 for m in _expected_matches(run))
    assert _expected_matches(260) == [256, 3] and _expected_matches(261) == [257, 3] and _expected_matches(262) == [258, 3]
    literals = block["bytes"] - sum(want)
    assert literals == 1 + sum(run if run < 4 else 1 for run in runs)                     # the filter byte, then one literal per long run
    # the same runs laid over the rows of an image: the filter byte of every row breaks them, and rows share segments
    plane2 = np.array(row[: 73 * 97], np.uint8).reshape(73, 97)
    _encode([(plane2, 0), (np.full((40, 50), 7, np.uint8), 0)])                          # ... and a single distinct pixel value


def test_white_noise_is_stored():
    g = np.random.default_rng(5)
    plane = g.integers(0, 256, (170, 64, 3)).astype(np.uint8)
    host, specs = _pack([(plane, 0)])
    from intrinsicnerf_amd import kernels
    (offset, capacity), = kernels.png_plan(specs)[1]
    (data, info), = _encode([(plane, 0)])
    assert [b["type"] for b in info["blocks"]] == ["stored", "stored", "stored"] and [b["bytes"] for b in info["blocks"]] == [169 * 193, 193, 0]
    assert len(data) == capacity == 68 + 170 * 193 + 5 * 2                                 # the stored-everything bound, reached


def test_a_ramp_takes_the_sub_filter():
    plane = np.tile(np.arange(200, dtype=np.uint8), (100, 1))
    (adaptive, info), (plain, info0) = _encode([(plane, -1), (plane, 0)])
    assert (info["filters"] != 0).all() and (info0["filters"] == 0).all()
    assert len(adaptive) < len(plain)
    for flt in (1, 2, 3, 4):                                                               # every fixed type, on something less regular
        p = _smooth((50, 41, 3), np.uint8, flt)
        (_, i), = _encode([(p, flt)])
        assert (i["filters"] == flt).all()
    (_, i16), = _encode([(_smooth((50, 41), np.uint16, 9), 4)])
    assert (i16["filters"] == 4).all()


def _huffman_depth(freq):
    heap = [(f, i, 0) for i, f in enumerate(freq) if f]
    heapq.heapify(heap)
    tick = len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return heap[0][2]


def test_fibonacci_counts_reach_the_15_bit_limit():
    """19 byte values with the Fibonacci counts 2, 3, 5 .. 10 946 (28 654 bytes, one segment) in a random order that never repeats a
    value four times, so every token is a literal; with the filter byte and the end of block (1, 1) the symbol counts are the
    Fibonacci numbers themselves: a Huffman tree of depth 20 (tallied here with the header's rule), so the block's longest code
    must be exactly 15."""
    import random
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    fib = fib[2:]
    left, row, rnd = list(fib), [], random.Random(6)
    assert sum(fib) == 28654 and sum(fib) + 1 <= CAP
    for _ in range(sum(fib)):
        barred = row[-1] if len(row) >= 3 and row[-1] == row[-2] == row[-3] else -1
        weights = [0 if v + 1 == barred else n for v, n in enumerate(left)]
        v = rnd.choices(range(19), weights)[0]
        left[v] -= 1
        row.append(v + 1)
    row = np.array(row, np.uint8)
    assert np.array_equal(np.bincount(row, minlength=20)[1:], fib)
    stream = np.concatenate([[0], row]).astype(np.int64)
    freq = [0] * 286
    edges = np.flatnonzero(np.diff(stream)) + 1
    for start, stop in zip(np.concatenate([[0], edges]), np.concatenate([edges, [stream.size]])):
        run = int(stop - start)
        assert run < 4
        freq[int(stream[start])] += run
    freq[256] = 1
    assert _huffman_depth(freq) == 20
    (data, info), = _encode([(row[None], 0)])
    block = info["blocks"][0]
    assert block["type"] == "dynamic" and not block["matches"] and max(block["litlen"]) == 15 and len(data) < row.size // 2


def test_sixteen_bit_samples_are_big_endian_in_the_file():
    plane = np.array([[0x00FF, 0xFF00, 0x1234], [0x1234, 0x00FF, 0xFF00]], np.uint16)
    (data, info), = _encode([(plane, 0)])
    assert info["raw"] == bytes([0, 0x00, 0xFF, 0xFF, 0x00, 0x12, 0x34, 0, 0x12, 0x34, 0x00, 0xFF, 0xFF, 0x00])
    (data, info), = _encode([(plane, -1)])
    assert _png.decode(data).tolist() == plane.tolist()


def test_two_calls_give_the_same_bytes_and_a_graph_replays_on_a_second_frame():
    from intrinsicnerf_amd import kernels
    dev = _dev()
    frames_ = []
    for seed in (0, 1):
        planes = [(_smooth((170, 64, 3), np.uint8, seed), -1), (_smooth((24, 32), np.uint16, seed + 5), -1),
                  (np.random.default_rng(seed).integers(0, 256, (40, 33)).astype(np.uint8), 0), (_smooth((30, 50), np.uint8, seed + 9), 2)]
        frames_.append(_pack(planes))
    (host0, specs), (host1, specs1) = frames_
    assert specs == specs1 and not np.array_equal(host0, host1)
    plan = kernels.png_plan(specs)
    src = torch.from_numpy(host0).to(dev)
    out = torch.zeros(plan[2], dtype=torch.uint8, device=dev)
    sizes = torch.zeros(len(specs), dtype=torch.int64, device=dev)
    workspace = torch.empty(plan[3], dtype=torch.uint8, device=dev)

    def run():
        kernels.png_encode(src, plan, out=out, sizes=sizes, workspace=workspace)

    def files():
        o, s = out.cpu().numpy(), sizes.cpu().numpy()
        return [o[off:off + int(n)].tobytes() for (off, _), n in zip(plan[1], s)]

    run()
    first = files()
    out.zero_(); sizes.zero_(); workspace.fill_(0x5A)
    run()
    assert files() == first                                                  # the same bytes, whatever the workspace held
    src.copy_(torch.from_numpy(host1).to(dev))
    out.zero_()
    run()
    direct = files()
    assert direct != first
    src.copy_(torch.from_numpy(host0).to(dev))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    src.copy_(torch.from_numpy(host1).to(dev))
    out.zero_(); sizes.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert files() == direct                                                 # captured on one frame, replayed on another


def test_encode_png_on_the_three_dtypes():
    from intrinsicnerf_amd import frames
    dev = _dev()
    for k, a in enumerate((_smooth((37, 53), np.uint8, 1), _smooth((37, 53, 3), np.uint8, 2), _smooth((37, 53), np.uint16, 3))):
        t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
        if a.dtype == np.uint16:
            t = t.view(torch.uint16)
        data = frames.encode_png(t)
        assert isinstance(data, bytes) and np.array_equal(_png.decode(data), a), k
        image, info = _png.decode(frames.encode_png(t, filter=0), with_info=True)
        assert np.array_equal(image, a) and (info["filters"] == 0).all()
    with pytest.raises(ValueError):
        frames.encode_png(torch.zeros(4, 4, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        frames.encode_png(torch.zeros(4, 4, 2, dtype=torch.uint8, device=dev))


def _decode_dir(path):
    return {name: _png.decode(open(os.path.join(path, name), "rb").read()) for name in sorted(os.listdir(path))}


def test_ssr_render_path_writes_device_encoded_files(tmp_path):
    """Built as tests/test_frame_products_gpu.py builds its SSR front-end: with ``FrameProducts(encode=True)`` the same file names,
    every file the same pixels, the returned arrays identical."""
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
    (tmp_path / "planes").mkdir(); (tmp_path / "files").mkdir()
    with torch.no_grad():
        r.frame_products = frames.FrameProducts()
        base = r.render_path(rays, save_dir=str(tmp_path / "planes"))
        r.frame_products = frames.FrameProducts(encode=True)
        out = r.render_path(rays, save_dir=str(tmp_path / "files"))
    assert len(out) == len(base) == 12
    for a, b in zip(out[:11], base[:11]):
        assert (a is None) == (b is None)
        if b is not None:
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    want, got = _decode_dir(tmp_path / "planes"), _decode_dir(tmp_path / "files")
    names = ("rgb", "albedo", "shading", "residual", "disp", "depth", "vis_depth", "label", "entropy", "vis_entropy", "vis_label")
    assert set(got) == set(want) == {f"{p}_{i:03d}.png" for i in range(N) for p in names}
    for name in want:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    assert got["depth_000.png"].dtype == np.uint16 and got["rgb_001.png"].shape == (H, W, 3)


def test_object_render_path_writes_device_encoded_files(tmp_path):
    import bench
    from intrinsicnerf_amd import frames, object_level as ol
    from test_frame_products_gpu import _chair_nets
    dev = _dev()
    side = 45
    K, focal, kw = _chair_nets(dev, side)
    poses = torch.stack([torch.cat([bench.chair_pose(theta_deg=t), torch.tensor([[0., 0., 0., 1.]])], 0) for t in (20., 130.)]).to(dev)
    with torch.no_grad():
        rgbs0, disps0, _ = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, savedir=str(tmp_path / "planes"), products=frames.FrameProducts())
        rgbs1, disps1, _ = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, savedir=str(tmp_path / "files"),
                                          products=frames.FrameProducts(encode=True))
    assert np.array_equal(rgbs1, rgbs0) and np.array_equal(disps1, disps0, equal_nan=True)
    want, got = _decode_dir(tmp_path / "planes"), _decode_dir(tmp_path / "files")
    assert set(got) == set(want) == {f"{p}{i:03d}.png" for i in range(2) for p in ("", "a", "s", "res", "acc")}
    for name in want:
        assert got[name].dtype == want[name].dtype == np.uint8 and np.array_equal(got[name], want[name]), name
    assert set(np.unique(got["acc000.png"])) <= {0, 255}
