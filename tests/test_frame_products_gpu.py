"""GPU: the frame images of csrc/frame_vis.hip - every product kind at the lane-quad, workgroup and staging-path edges with
sentinels around the planes, the edge values of every rule, ``inerf_frame_range`` bit for bit against numpy, byte equality with
``inerf_frame_to_u8``, determinism and graph capture, and both ``render_path`` front-ends with the device planes against the
host path.  Every comparison is byte equality against the numpy restatement (_frame_vis.py)."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import _frame_vis as V

pytestmark = pytest.mark.gpu
F = np.float32


def _dev():
    return torch.device("cuda:0")


def _case_frame(n, columns=12, seed=0, colours=28):
    """[n, columns] fp32: cols 0-3 around [0, 1], 4 a disparity-like range that wraps 16 bits, 5 a depth in metres, 6 labels around
    [0, colours), 7 an accumulated opacity around the threshold 10, 8 an entropy-like map; NaN and +-inf sprinkled in."""
    g = np.random.default_rng(seed + n)
    x = g.uniform(-0.2, 1.2, (n, columns)).astype(F)
    x[:, 4] = g.uniform(-3.0, 70000.0, n)
    x[:, 5] = g.uniform(0.0, 12.0, n)
    x[:, 6] = g.integers(-1, colours + 2, n)
    x[:, 7] = g.uniform(0.0, 20.0, n)
    x[:, 8] = g.normal(1.0, 0.7, n)
    for j, v in enumerate((np.nan, np.inf, -np.inf)):
        rows = g.integers(0, n, max(n // 40, 1 if n > 3 + j else 0))
        x[rows, g.integers(0, 9, len(rows))] = v
    return x


def _sixteen(rng):
    """16 products over columns 0 .. 8, every kind among them; ``rng``: what the last JET reads its range from."""
    return [(V.TO8B, 0, 3, 0.0, 0.0, None), (V.TO8B, 3, 1, 0.0, 0.0, None), (V.U16, 4, 1, 1.0, 0.0, None), (V.U16, 5, 1, 1000.0, 0.0, None),
            (V.U8_CAST, 6, 1, 0.0, 0.0, None), (V.THRESH, 7, 1, 10.0, 0.0, None), (V.PALETTE, 6, 1, 0.0, 0.0, None),
            (V.JET_KIND, 5, 1, 0.1, 10.0, None), (V.JET_KIND, 8, 1, 0.0, 0.0, rng), (V.TO8B, 3, 3, 0.0, 0.0, None),
            (V.TO8B, 8, 1, 0.0, 0.0, None), (V.U8_CAST, 4, 1, 0.0, 0.0, None), (V.U16, 8, 1, 1000.0, 0.0, None),
            (V.THRESH, 0, 1, 0.5, 0.0, None), (V.JET_KIND, 0, 1, 0.25, 0.25, None), (V.PALETTE, 7, 1, 0.0, 0.0, None)]


def _launch(frame, specs, colours=None, guard=64):
    """One launch into a sentinel-filled buffer; returns (bytes as numpy, planes, total)."""
    from intrinsicnerf_amd import kernels
    pal = None if colours is None else torch.from_numpy(colours).to(frame.device)
    plan = kernels.frame_products_plan(frame.shape[0], specs, 0 if pal is None else pal.shape[0])
    out = torch.full((plan[2] + guard,), 0xA5, dtype=torch.uint8, device=frame.device)
    kernels.frame_products(frame, None, palette=pal, out=out, plan=plan)
    return out.cpu().numpy(), plan[1], plan[2]


def _check(got, planes, total, host_frame, specs, colours, ranges=None):
    """Every plane equals the restatement; every byte between and after the planes is still the sentinel."""
    assert (planes, total) == V.layout(host_frame.shape[0], specs)
    untouched = np.ones(len(got), bool)
    for k, (spec, (off, size)) in enumerate(zip(specs, planes)):
        spec = spec[:5] + ((ranges or {}).get(k),)
        want = V.product(host_frame, spec, colours)
        assert off % 16 == 0 and want.size == size
        assert np.array_equal(got[off:off + size], want), (k, spec[:3], np.flatnonzero(got[off:off + size] != want)[:8])
        untouched[off:off + size] = False
    assert (got[untouched] == 0xA5).all() and untouched[total:].all()


# 1, 3, 4, 5: the lane quad; 255 .. 257 and 511 .. 513: wave and workgroup (512 pixels) edges; 1021, 1025: more than one workgroup
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1021, 1025])
def test_every_kind_in_one_launch_sizes_layout_and_sentinels(n):
    from intrinsicnerf_amd import kernels
    dev = _dev()
    colours = np.random.default_rng(1).integers(0, 256, (28, 3)).astype(np.uint8)
    host = _case_frame(n)
    wide = torch.from_numpy(host).to(dev)                                   # stride 12 > the 9 used columns: the strided staging path
    rng = kernels.frame_range(wide[:, 8])
    specs = _sixteen(rng)
    ranges = {8: V.frame_range(host[:, 8])}
    assert np.array_equal(rng.cpu().numpy(), np.array(ranges[8], F), equal_nan=True)
    _check(*_launch(wide, specs, colours), host, specs, colours, ranges)
    tight = wide[:, :9].contiguous()                                        # stride == span, 16-byte aligned: the 16-byte staging loads
    _check(*_launch(tight, specs, colours), host[:, :9], specs, colours, ranges)
    shifted = torch.empty(n * 9 + 1, dtype=torch.float32, device=dev)[1:].view(n, 9)      # stride == span, 4-byte aligned only
    shifted.copy_(tight)
    _check(*_launch(shifted, specs, colours), host[:, :9], specs, colours, ranges)
    few = [specs[9], specs[2]]                                              # columns 3 .. 5 alone: a span that ends inside the frame
    _check(*_launch(wide, few, None), host, few, None)


def _column(values):
    return torch.from_numpy(np.asarray(values, F).reshape(-1, 1)).to(_dev())


def test_edge_values_to8b_and_integer_casts():
    k = np.arange(256, dtype=np.float64) / 255.0
    base = k.astype(F)
    x = np.concatenate([base, np.nextafter(base, F(-1)), np.nextafter(base, F(2)), F([0.0, -0.0, 1.0, -1e-30, 1e-30, np.nan, np.inf, -np.inf, 1.0000001])])
    y = np.concatenate([F([v for v, _ in V.U16_EDGES]), F([255.0, 255.9, 256.0, 300.0, -255.0, -256.0, -257.0, 1.0005, 65.5359, 65.536])])
    z = np.concatenate([F([9.999999, 10.0, 10.000001, -np.inf, np.inf, np.nan, 0.0]), np.zeros(3, F)])
    n = max(len(x), len(y), len(z))
    host = np.zeros((n, 3), F)
    host[:len(x), 0], host[:len(y), 1], host[:len(z), 2] = x, y, z
    specs = [(V.TO8B, 0, 1, 0.0, 0.0, None), (V.U16, 1, 1, 1.0, 0.0, None), (V.U16, 1, 1, 1000.0, 0.0, None), (V.U8_CAST, 1, 1, 0.0, 0.0, None),
             (V.THRESH, 2, 1, 10.0, 0.0, None), (V.TO8B, 0, 3, 0.0, 0.0, None)]
    got, planes, total = _launch(torch.from_numpy(host).to(_dev()), specs)
    _check(got, planes, total, host, specs, None)
    # ... and against numpy's own casts, the expressions the host path uses
    with np.errstate(invalid="ignore", over="ignore"):
        o, s = planes[1]
        assert np.array_equal(got[o:o + s].view("<u2"), host[:, 1].astype(np.uint16))
        o, s = planes[0]
        finite = ~np.isnan(host[:, 0])
        assert np.array_equal(got[o:o + s][finite], (255 * np.clip(host[finite, 0], 0, 1)).astype(np.uint8))
        o, s = planes[2]
        assert got[o:o + s].view("<u2")[len(V.U16_EDGES) + 7] == 1000                         # float32(1.0005) * 1000


@pytest.mark.parametrize("C", [1, 28, 101])
def test_edge_values_palette(C):
    colours = np.random.default_rng(C).integers(1, 256, (C, 3)).astype(np.uint8)
    labels = F([0, C - 1, C, -1, np.nan, -0.5, C - 0.5, 0.999, 3e9, -3e9, np.inf, -np.inf, 255, 256] + list(range(C)))
    host = labels.reshape(-1, 1)
    specs = [(V.PALETTE, 0, 1, 0.0, 0.0, None), (V.U8_CAST, 0, 1, 0.0, 0.0, None)]
    got, planes, total = _launch(torch.from_numpy(host).to(_dev()), specs, colours)
    _check(got, planes, total, host, specs, colours)
    rgb = got[:planes[0][1]].reshape(-1, 3)
    assert np.array_equal(rgb[0], colours[0]) and np.array_equal(rgb[1], colours[C - 1])
    assert not rgb[2].any() and not rgb[3].any() and not rgb[4].any()                       # C, -1 and NaN: black
    assert np.array_equal(rgb[14:], colours)


@pytest.mark.parametrize("lo,hi", [(0.1, 10.0), (-3.0, 5.5), (0.0, 1.0), (2.0, 2.0), (1e-3, 1e30)])
def test_edge_values_jet(lo, hi):
    from intrinsicnerf_amd import frames
    lo32, hi32 = F(lo), F(hi)
    with np.errstate(all="ignore"):
        steps = (lo32 + np.arange(257, dtype=F) * (hi32 - lo32) / F(256)).astype(F)
    x = np.concatenate([steps, np.nextafter(steps, F(-np.inf)), np.nextafter(steps, F(np.inf)),
                        F([lo, hi, np.nextafter(hi32, F(-np.inf)), np.nextafter(lo32, F(np.inf)), lo - 1.0, hi + 1.0, -1e38, 1e38, np.nan, np.inf,
                           -np.inf, 0.0, -0.0])])
    host = x.reshape(-1, 1)
    dev_range = torch.tensor([lo, hi], dtype=torch.float32, device=_dev())
    specs = [(V.JET_KIND, 0, 1, lo, hi, None), (V.JET_KIND, 0, 1, 0.0, 0.0, dev_range)]
    got, planes, total = _launch(torch.from_numpy(host).to(_dev()), specs)
    _check(got, planes, total, host, specs, None, {1: (lo, hi)})
    rgb = got[:planes[0][1]].reshape(-1, 3)
    if hi > lo:
        assert np.array_equal(rgb[3 * 257], V.JET[0]) and np.array_equal(rgb[3 * 257 + 1], V.JET[255])      # x = lo, x = hi
        assert np.array_equal(rgb[3 * 257 + 4], V.JET[0]) and np.array_equal(rgb[3 * 257 + 5], V.JET[255])  # below lo, above hi
    else:
        assert not rgb[3 * 257].any() and np.array_equal(rgb[3 * 257 + 5], V.JET[255])                       # hi == lo: 0 / 0, and +x / 0
    assert not rgb[3 * 257 + 8].any()                                                                         # NaN
    # frames.depth2rgb on the device is the same launch
    img = frames.depth2rgb(torch.from_numpy(x).to(_dev()).reshape(-1, 7 if len(x) % 7 == 0 else 1), min_value=lo, max_value=hi)
    assert img.dtype == torch.uint8 and np.array_equal(img.cpu().numpy().reshape(-1, 3), rgb)


def _range_case(n, seed=0):
    g = np.random.default_rng(100 + seed + n)
    x = g.normal(0.0, 3.0, n).astype(F)
    if n >= 63:
        x[g.integers(0, n, n // 8)] = np.nan
    return x


# 1, 63 .. 65: a wave; 4097: 17 workgroups; 65537: beyond the grid cap (256 workgroups x 256 lanes), the grid-stride loop
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 65537])
def test_frame_range_is_numpy_nanmin_nanmax_bit_for_bit(n):
    from intrinsicnerf_amd import kernels
    dev = _dev()
    same = lambda t, want: np.array_equal(t.cpu().numpy().view(np.int32), np.array(want, F).view(np.int32))
    x = _range_case(n)
    assert same(kernels.frame_range(torch.from_numpy(x).to(dev)), V.frame_range(x))
    wide = torch.zeros(n, 5, device=dev)                                    # a column of a pack: element stride 5
    wide[:, 3] = torch.from_numpy(x).to(dev)
    assert same(kernels.frame_range(wide[:, 3]), V.frame_range(x))
    y = x.copy()
    y[n // 2] = np.inf
    y[0] = -np.inf if n > 1 else y[0]
    assert same(kernels.frame_range(torch.from_numpy(y).to(dev)), V.frame_range(y))
    nan = np.full(n, np.nan, F)
    got = kernels.frame_range(torch.from_numpy(nan).to(dev)).cpu().numpy()
    assert np.isnan(got).all()                                              # an all-NaN map: (NaN, NaN)


def test_frame_range_accumulates_over_frames_and_feeds_jet():
    from intrinsicnerf_amd import frames, kernels
    dev = _dev()
    parts = [_range_case(4097, 1), np.full(300, np.nan, F), _range_case(1021, 2) * F(4.0)]
    minmax = None
    for i, p in enumerate(parts):
        minmax = kernels.frame_range(torch.from_numpy(p).to(dev), minmax=minmax, accumulate=i > 0)
    want = V.frame_range(np.concatenate(parts))
    assert np.array_equal(minmax.cpu().numpy().view(np.int32), np.array(want, F).view(np.int32))
    # accumulate == 0 overwrites what minmax held
    again = kernels.frame_range(torch.from_numpy(parts[0]).to(dev), minmax=minmax)
    assert np.array_equal(again.cpu().numpy(), np.array(V.frame_range(parts[0]), F))
    # JET with the device range == the restatement with numpy's range: depth2rgb without a given range, and with one bound given
    x = V.edge_frame()
    finite = np.where(np.isinf(x), np.nan, x)
    t = torch.from_numpy(finite).to(dev)
    lo, hi = V.frame_range(finite)
    assert np.array_equal(frames.depth2rgb(t).cpu().numpy(), V.jet(finite, lo, hi))
    assert np.array_equal(frames.depth2rgb(t, min_value=1.0).cpu().numpy(), V.jet(finite, 1.0, hi))
    assert np.array_equal(frames.depth2rgb(t, max_value=7.0).cpu().numpy(), V.jet(finite, lo, 7.0))
    assert np.array_equal(frames.depth2rgb(torch.from_numpy(x).to(dev)).cpu().numpy(), V.jet(x, *V.frame_range(x)))          # +-inf take part
    assert not frames.depth2rgb(torch.full((5, 7), float("nan"), device=dev)).any()


def test_to8b_planes_equal_inerf_frame_to_u8():
    from intrinsicnerf_amd import kernels
    dev = _dev()
    n = 2051
    host = _case_frame(n)
    host[:256, 1] = np.arange(256, dtype=F) / F(255)
    frame = torch.from_numpy(host).to(dev)
    specs = [(V.TO8B, 0, 3, 0.0, 0.0, None), (V.TO8B, 3, 1, 0.0, 0.0, None), (V.TO8B, 8, 1, 0.0, 0.0, None)]
    out, planes = kernels.frame_products(frame, specs)
    for (_, column, width, *_), (off, size) in zip(specs, planes):
        want = kernels.frame_to_u8(frame[:, column:column + width].contiguous())
        assert torch.equal(out[off:off + size], want.reshape(-1))


def _ssr_specs(rng):
    """The eleven products of the SSR front-end over its 14-column pack."""
    return [(V.TO8B, 0, 3, 0.0, 0.0, None), (V.TO8B, 5, 3, 0.0, 0.0, None), (V.TO8B, 8, 1, 0.0, 0.0, None), (V.TO8B, 9, 3, 0.0, 0.0, None),
            (V.U16, 3, 1, 1.0, 0.0, None), (V.U16, 4, 1, 1000.0, 0.0, None), (V.JET_KIND, 4, 1, 0.1, 10.0, None), (V.U8_CAST, 12, 1, 0.0, 0.0, None),
            (V.TO8B, 13, 1, 0.0, 0.0, None), (V.JET_KIND, 13, 1, 0.0, 0.0, rng), (V.PALETTE, 12, 1, 0.0, 0.0, None)]


def _ssr_frame(seed, n=240 * 320):
    g = np.random.default_rng(seed)
    x = g.uniform(-0.1, 1.1, (n, 14)).astype(F)
    x[:, 3] = g.uniform(0.0, 9.0, n)
    x[:, 4] = g.uniform(0.05, 11.0, n)
    x[:, 12] = g.integers(0, 28, n)
    x[:, 13] = g.uniform(0.0, 3.3, n)
    x[g.integers(0, n, 50), 13] = np.nan
    return x


def test_a_240x320_frame_twice_and_a_captured_graph_on_a_second_frame():
    from intrinsicnerf_amd import kernels
    dev = _dev()
    colours = np.random.default_rng(2).integers(0, 256, (28, 3)).astype(np.uint8)
    pal = torch.from_numpy(colours).to(dev)
    hosts = [_ssr_frame(11), _ssr_frame(12)]
    n = hosts[0].shape[0]
    pack = torch.from_numpy(hosts[0]).to(dev)
    rng = torch.full((2,), float("nan"), device=dev)
    specs = _ssr_specs(rng)
    plan = kernels.frame_products_plan(n, specs, 28)
    workspace = torch.empty(kernels.frame_range_workspace_bytes(n) // 4, device=dev)
    out = torch.zeros(plan[2], dtype=torch.uint8, device=dev)

    def run():
        kernels.frame_range(pack[:, 13], minmax=rng, workspace=workspace)
        kernels.frame_products(pack, None, palette=pal, out=out, plan=plan)

    run()
    first = out.cpu().numpy().copy()
    padded = np.concatenate([first, np.full(64, 0xA5, np.uint8)])
    for k, (off, size) in enumerate(plan[1]):                               # the planes; the up to 15 pad bytes between them were zeroed above
        spec = specs[k][:5] + (V.frame_range(hosts[0][:, 13]) if k == 9 else None,)
        assert np.array_equal(padded[off:off + size], V.product(hosts[0], spec, colours)), k
    out.zero_()
    run()
    assert np.array_equal(out.cpu().numpy(), first)                         # the same bytes from a second run
    # range + products captured once, replayed on a second frame's data
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    pack.copy_(torch.from_numpy(hosts[1]).to(dev))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for k, (off, size) in enumerate(plan[1]):
        spec = specs[k][:5] + (V.frame_range(hosts[1][:, 13]) if k == 9 else None,)
        assert np.array_equal(got[off:off + size], V.product(hosts[1], spec, colours)), k
    assert not np.array_equal(got, first)


def _read_png(path):
    data = open(path, "rb").read()
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", data[pos + 8:pos + 8 + n])
        if tag == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    w, h, depth, colour = hdr[:4]
    raw = zlib.decompress(idat)
    bpp = (3 if colour == 2 else 1) * depth // 8
    if any(raw[r * (1 + w * bpp)] != 0 for r in range(h)):                 # another encoder chose a row filter: let PIL decode it
        from PIL import Image
        return np.array(Image.open(path))
    rows = [raw[r * (1 + w * bpp) + 1:(r + 1) * (1 + w * bpp)] for r in range(h)]
    return np.frombuffer(b"".join(rows), dtype=np.uint8 if depth == 8 else ">u2").reshape((h, w, 3) if colour == 2 else (h, w)).astype(
        np.uint8 if depth == 8 else np.uint16)


def test_ssr_render_path_with_frame_products(tmp_path):
    """Built as tests/test_frames_gpu.py builds its SSR front-end.  With ``frame_products`` the visualisations exist without imgviz
    and equal the restatement applied to the returned maps; every file both paths write decodes to the same array."""
    from intrinsicnerf_amd import frames, ssr
    from oracle import calibration as cal
    dev = _dev()
    H, W, C, N = 12, 17, 5, 4                                               # 204 pixels: no multiple of 4 x anything convenient
    r = ssr.SSRRenderer(C, white_bkgd=False, chunk=100, device=dev)
    r.H_scaled, r.W_scaled, r.near, r.far = H, W, 0.1, 10.0
    r.check_numerics = False
    T = torch.eye(4)[None].repeat(N, 1, 1)
    T[1, :3, 3], T[2, :3, 3], T[3, :3, 3] = torch.tensor([0.2, 0.0, 0.1]), torch.tensor([-0.3, 0.1, 0.0]), torch.tensor([0.1, -0.2, 0.3])
    rays = ssr.create_rays(N, T.to(dev), H, W, 8.0, 8.0, (W - 1) / 2.0, (H - 1) / 2.0, 0.1, 10.0)
    r.ssr_net_coarse.load_state_dict(cal.calibrated_default_init("ssr", C, 0, rays[0].cpu()))
    r.ssr_net_fine.load_state_dict(cal.calibrated_default_init("ssr", C, 1, rays[0].cpu()))
    colours = (torch.arange(C * 3, dtype=torch.uint8).reshape(C, 3) * 17 + 3)
    r.valid_colour_map = colours.to(dev)
    (tmp_path / "host").mkdir(); (tmp_path / "dev").mkdir()
    assert r.frame_products is None
    with torch.no_grad():
        base = r.render_path(rays, save_dir=str(tmp_path / "host"))
        r.frame_products = frames.FrameProducts()
        out = r.render_path(rays, save_dir=str(tmp_path / "dev"))
    rgbs, disps, deps, vis_deps, sems, vis_sems, ents, vis_ents, albedos, shadings, residuals, manager = out
    assert manager is None and len(out) == 12
    for a, b in zip(out[:11], base[:11]):                                   # the float maps and what the host path also makes: identical
        if b is not None:
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    try:
        import imgviz  # noqa: F401
    except ImportError:
        assert base[3] is None and base[7] is None                          # the path as it stands: no imgviz, no visualisation
    assert vis_deps.shape == (N, H, W, 3) and vis_deps.dtype == np.uint8 and vis_ents.shape == (N, H, W, 3) and vis_ents.dtype == np.uint8
    assert sems.shape == (N, H, W) and sems.dtype == np.uint8 and vis_sems.shape == (N, H, W, 3) and vis_sems.dtype == np.uint8
    for i in range(N):
        assert np.array_equal(vis_deps[i], V.jet(deps[i], 0.1, 10.0))
        assert np.array_equal(vis_ents[i], V.jet(ents[i], *V.frame_range(ents[i])))
        assert np.array_equal(vis_sems[i], colours.numpy()[sems[i].astype(np.int64)])
    assert len({vis_deps[i].tobytes() for i in range(N)}) > 1 and vis_ents.any()
    host_files, dev_files = sorted(os.listdir(tmp_path / "host")), sorted(os.listdir(tmp_path / "dev"))
    names = ("rgb", "albedo", "shading", "residual", "disp", "depth", "label", "entropy", "vis_label")
    assert set(host_files) >= {f"{p}_{i:03d}.png" for i in range(N) for p in names} and set(dev_files) >= set(host_files)
    for name in host_files:
        a, b = _read_png(tmp_path / "host" / name), _read_png(tmp_path / "dev" / name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    for i in range(N):
        assert np.array_equal(_read_png(tmp_path / "dev" / f"vis_depth_{i:03d}.png"), vis_deps[i])
        assert np.array_equal(_read_png(tmp_path / "dev" / f"vis_entropy_{i:03d}.png"), vis_ents[i])
        assert _read_png(tmp_path / "dev" / f"depth_{i:03d}.png").dtype == np.uint16


def _chair_nets(dev, side):
    import bench
    import oracle
    from intrinsicnerf_amd import object_level as ol
    focal = 0.5 * side / np.tan(0.5 * bench.CAMERA_ANGLE_X)
    K = np.array([[focal, 0, 0.5 * side], [0, focal, 0.5 * side], [0, 0, 1]])
    ro, rd = ol.get_rays(side, side, K, bench.chair_pose())
    vd = rd / rd.norm(dim=-1, keepdim=True)
    rays = torch.cat([ro, rd, 2 * torch.ones_like(rd[..., :1]), 6 * torch.ones_like(rd[..., :1]), vd], -1).reshape(-1, 11)
    probe = rays[::max(1, rays.shape[0] // 384)]
    sd_c, _ = oracle.calibrated_lcg_weights("object", 0, 50, probe)
    sd_f, _ = oracle.calibrated_lcg_weights("object", 0, 51, probe)
    embed, ch = ol.get_embedder(10, 0); embed_d, ch_d = ol.get_embedder(4, 0)
    mk = lambda: ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
    net_c, net_f = mk(), mk()
    net_c.load_state_dict(sd_c); net_f.load_state_dict(sd_f)
    kw = dict(network_fn=net_c, network_fine=net_f, network_query_fn=ol.NetworkQuery(embed, embed_d), N_samples=64, N_importance=128,
              white_bkgd=True, perturb=False, raw_noise_std=0., use_viewdirs=True, ndc=False, lindisp=False, near=2., far=6.)
    return K, focal, kw


def test_object_render_path_with_products(tmp_path):
    """The same files and the same ``(rgbs, disps)`` as without ``products`` - with only rgb and disp travelling as floats, and, under
    a host-side cluster fit, with all maps travelling."""
    import bench
    from intrinsicnerf_amd import frames, object_level as ol
    dev = _dev()
    side = 45                                                               # 2025 pixels: an odd count, four workgroups
    K, focal, kw = _chair_nets(dev, side)
    poses = torch.stack([torch.cat([bench.chair_pose(theta_deg=t), torch.tensor([[0., 0., 0., 1.]])], 0) for t in (20., 75., 130., 200.)]).to(dev)

    class Manager:      # stands in for the reference's Cluster_Manager, as tests/test_frames_gpu.py does
        def __init__(self, class_num):
            pass

        def update_center(self, labels, pixels, band_factor):
            pass

        def dest_color(self, pixel, label):
            return 0.5 * pixel + 0.25

    dirs = {k: tmp_path / k for k in ("host", "dev", "host_fit", "dev_fit")}
    pushed = []
    push = frames.FrameStreamer.push

    def spy(self, pack):
        pushed.append((tuple(pack.shape), pack.dtype))
        return push(self, pack)

    with torch.no_grad():
        rgbs0, disps0, _ = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, savedir=str(dirs["host"]))
        frames.FrameStreamer.push = spy
        try:
            rgbs1, disps1, mgr = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, savedir=str(dirs["dev"]), products=frames.FrameProducts())
        finally:
            frames.FrameStreamer.push = push
        ol.render_path(poses[:2], (side, side, focal), K, 1 << 15, kw, savedir=str(dirs["host_fit"]), update_cluster=True,
                       cluster_manager_factory=Manager)
        rgbs2, disps2, mgr2 = ol.render_path(poses[:2], (side, side, focal), K, 1 << 15, kw, savedir=str(dirs["dev_fit"]), update_cluster=True,
                                             cluster_manager_factory=Manager, products=frames.FrameProducts())
    assert mgr is None and isinstance(mgr2, Manager)
    assert rgbs1.dtype == np.float32 and np.array_equal(rgbs1, rgbs0) and np.array_equal(disps1, disps0, equal_nan=True)
    assert np.array_equal(rgbs2, rgbs0[:2]) and np.array_equal(disps2, disps0[:2], equal_nan=True)
    # per pixel 4 floats and 11 bytes travelled, not the pack's 12 floats
    n = side * side
    pad = lambda b: (b + 15) // 16 * 16
    assert set(pushed) == {((n, 4), torch.float32), ((3 * pad(3 * n) + 2 * pad(n),), torch.uint8)}
    for a, b, count in (("host", "dev", 4), ("host_fit", "dev_fit", 2)):
        names = sorted(os.listdir(dirs[a]))
        want = {f"{p}{i:03d}.png" for i in range(count) for p in (("", "a", "s", "res", "acc") + (("c", "edit") if count == 2 else ()))}
        assert set(names) == want and sorted(os.listdir(dirs[b])) == names
        for name in names:
            x, y = _read_png(dirs[a] / name), _read_png(dirs[b] / name)
            assert x.dtype == y.dtype == np.uint8 and np.array_equal(x, y), (a, name)
    acc = _read_png(dirs["dev"] / "acc000.png")
    assert set(np.unique(acc)) <= {0, 255}


def test_object_render_path_with_products_and_a_cluster_refresh(tmp_path):
    """``render_path(update_cluster=True, refresh=ClusterRefresh(...), products=...)``: the same ``(rgbs, disps)``, the same five
    images and the same ``c`` / ``edit`` files as without ``products`` - with only rgb and disp travelling as floats while the
    refresh pass keeps every pack (12 floats per pixel each), and with all maps travelling as soon as its budget misses one: at
    a budget of 11 floats per pixel and frame, one byte below the packs' real size, and at one byte."""
    import bench
    from intrinsicnerf_amd import cluster as ic, frames, object_level as ol, refresh
    dev = _dev()
    side, N = 45, 3
    n = side * side
    K, focal, kw = _chair_nets(dev, side)
    poses = torch.stack([torch.cat([bench.chair_pose(theta_deg=t), torch.tensor([[0., 0., 0., 1.]])], 0) for t in (20., 75., 130.)]).to(dev)
    assert refresh.ClusterRefresh(keep_bytes=N * n * 48).keeps_all(N, n * 48) and not refresh.ClusterRefresh(keep_bytes=N * n * 48 - 1).keeps_all(N, n * 48)
    variants = [("base", None, False, None), ("fits", N * n * 48, True, True), ("default", None, True, True),
                ("eleven_floats", N * n * 44, True, False), ("one_short", N * n * 48 - 1, True, False), ("one_byte", 1, True, False)]
    push = frames.FrameStreamer.push
    runs = {}
    for name, keep, with_products, slim in variants:
        d = tmp_path / name
        d.mkdir()
        pushed = []

        def spy(self, pack):
            pushed.append((tuple(pack.shape), pack.dtype))
            return push(self, pack)

        frames.FrameStreamer.push = spy
        try:
            with torch.no_grad():
                r = refresh.ClusterRefresh() if keep is None else refresh.ClusterRefresh(keep_bytes=keep)
                out = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, savedir=str(d), update_cluster=True, refresh=r,
                                     products=frames.FrameProducts() if with_products else None)
        finally:
            frames.FrameStreamer.push = push
        runs[name] = (out, d)
        floats = {shape for shape, dtype in pushed if dtype == torch.float32}
        if slim is not None:
            assert floats == ({(n, 4)} if slim else {(n, 12)}), (name, floats)
        else:
            assert floats == {(n, 12)}
    (rgbs0, disps0, mgr0), d0 = runs["base"]
    names = sorted(os.listdir(d0))
    assert set(names) == {f"{p}{i:03d}.png" for i in range(N) for p in ("", "a", "s", "res", "acc", "c", "edit")}
    assert isinstance(mgr0, ic.Cluster_Manager) and mgr0.clusters[0] is not None
    for name, ((rgbs, disps, mgr), d) in runs.items():
        assert isinstance(mgr, ic.Cluster_Manager), name
        assert np.array_equal(rgbs, rgbs0) and np.array_equal(disps, disps0, equal_nan=True), name
        assert sorted(os.listdir(d)) == names, name
        for f in names:
            x, y = _read_png(d0 / f), _read_png(d / f)
            assert x.dtype == y.dtype == np.uint8 and np.array_equal(x, y), (name, f)


def test_the_widest_frame_31_columns():
    """Columns [0, 31): the most a launch stages (1 KB of jet words + 31 x 516 floats = 65 008 bytes of LDS); the 32nd is refused."""
    from intrinsicnerf_amd import _capi, kernels
    dev = _dev()
    colours = np.random.default_rng(4).integers(0, 256, (28, 3)).astype(np.uint8)
    for n in (5, 1021):
        g = np.random.default_rng(n)
        host = g.uniform(-0.2, 1.2, (n, 32)).astype(F)
        host[:, 30] = g.uniform(-1.0, 12.0, n)
        host[:, 27] = g.integers(-1, 30, n)
        host[n // 2, 30] = np.nan
        specs = [(V.TO8B, 28, 3, 0.0, 0.0, None), (V.JET_KIND, 30, 1, 0.1, 10.0, None), (V.U16, 30, 1, 1000.0, 0.0, None), (V.TO8B, 0, 3, 0.0, 0.0, None),
                 (V.PALETTE, 27, 1, 0.0, 0.0, None), (V.TO8B, 15, 1, 0.0, 0.0, None), (V.U8_CAST, 27, 1, 0.0, 0.0, None)]
        wide = torch.from_numpy(host).to(dev)                               # stride 32, span 31
        _check(*_launch(wide, specs, colours), host, specs, colours)
        tight = wide[:, :31].contiguous()                                   # stride == span == 31
        _check(*_launch(tight, specs, colours), host[:, :31], specs, colours)
        with pytest.raises(RuntimeError, match="unsupported"):
            kernels.frame_products(wide, [(V.TO8B, 31, 1, 0.0, 0.0, None)])


def test_an_empty_palette_paints_black():
    """n_colours == 0 with a PALETTE product: 0 <= l < 0 holds for no label, so every pixel - the labels in (-1, 1) included - is black
    and the palette is not read."""
    from intrinsicnerf_amd import kernels
    dev = _dev()
    host = F([-0.5, 0.0, 0.5, -0.999, 1.0, np.nan, 3.0]).reshape(-1, 1)
    specs = [(V.PALETTE, 0, 1, 0.0, 0.0, None)]
    empty = np.zeros((0, 3), np.uint8)
    got, planes, total = _launch(torch.from_numpy(host).to(dev), specs, empty)
    _check(got, planes, total, host, specs, empty)
    assert not got[:planes[0][1]].any()
