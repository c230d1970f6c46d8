"""The cluster-refresh pass on the device (csrc/refresh.hip, intrinsicnerf_amd/refresh.py): inerf_frame_subsample and
inerf_cluster_snap_compose against numpy slicing, ``cluster.lookup`` and ``frames.to8b`` on host arrays, ``cluster.fit(counts=)``
against the host-label fit, and ``render_path(update_cluster=True)`` through a ``ClusterRefresh`` against the host path.
Every expectation comes from code that is itself pinned to the reference; every comparison is exact."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from _cluster_fit_check import GOLD
from conftest import load_golden
from test_cluster import Manager, fixture_clusters

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


# ---- 1. subsample ---------------------------------------------------------------------------------------------------------------
ALBEDO_COL, LABEL_COL, STRIDE = 2, 6, 9         # [pad pad | albedo3 | pad | label | pad pad]


def _labelled_frame(H, W, K, seed):
    g = np.random.RandomState(seed)
    frame = g.rand(H * W, STRIDE).astype(np.float32)
    lab = g.randint(-1, K + 4, size=H * W)
    forced = (-1, K, K + 3, 0)                   # on sampled pixels of row 0 where the frame has room for them
    for j, v in enumerate(forced):
        if 2 * j < W:
            lab[2 * j] = v
    frame[:, LABEL_COL] = lab
    return frame


@pytest.mark.parametrize("H,W,step", [(1, 1, 2), (2, 2, 2), (3, 5, 2), (12, 16, 2), (48, 48, 2), (12, 16, 1)])
@pytest.mark.parametrize("K", [1, 5])
def test_frame_subsample(H, W, step, K):
    from intrinsicnerf_amd import kernels
    dev = _dev()
    host = [_labelled_frame(H, W, K, 100 * H + W + s) for s in (0, 1)]
    rows = -(-H // step) * -(-W // step)
    pixels = torch.full((2 * rows + 1, 3), -7.0, device=dev)
    labels = torch.full((2 * rows + 1,), -77, dtype=torch.int64, device=dev)
    counts = torch.zeros(K, dtype=torch.int32, device=dev)
    for i, f in enumerate(host):                 # two frames at consecutive offsets of one table
        got = kernels.frame_subsample(torch.from_numpy(f).to(dev), H, W, ALBEDO_COL, pixels, offset=i * rows, label_col=LABEL_COL,
                                      out_labels=labels, class_counts=counts, step=step)
        assert got == rows
    want_px = np.concatenate([f.reshape(H, W, STRIDE)[::step, ::step, ALBEDO_COL:ALBEDO_COL + 3].reshape(-1, 3) for f in host], 0)
    want_lab = np.concatenate([f.reshape(H, W, STRIDE)[::step, ::step, LABEL_COL].reshape(-1) for f in host], 0).astype(np.int64)
    assert np.array_equal(pixels.cpu().numpy()[:2 * rows], want_px) and np.array_equal(labels.cpu().numpy()[:2 * rows], want_lab)
    assert (pixels[2 * rows:] == -7.0).all() and (labels[2 * rows:] == -77).all()              # nothing past the two frames
    want_counts = np.bincount(want_lab[(want_lab >= 0) & (want_lab < K)], minlength=K)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    if (H, W) == (48, 48):
        assert {-1, K, K + 3} <= set(want_lab.tolist())
    # no label column: the labels and the counts are left alone
    pixels2 = torch.full((rows, 3), -7.0, device=dev)
    labels2 = torch.full((rows,), -77, dtype=torch.int64, device=dev)
    counts2 = torch.full((K,), 123, dtype=torch.int32, device=dev)
    kernels.frame_subsample(torch.from_numpy(host[0]).to(dev), H, W, ALBEDO_COL, pixels2, label_col=-1, out_labels=labels2,
                            class_counts=counts2, step=step)
    assert np.array_equal(pixels2.cpu().numpy(), want_px[:rows]) and (labels2 == -77).all() and (counts2 == 123).all()


# ---- 2. snap and compose -----------------------------------------------------------------------------------------------------------
SNAP_COLS = dict(shading=0, albedo=1, label=4, residual=5)          # [shading | albedo3 | label | residual3 | pad pad]
SNAP_STRIDE = 10
SNAP_SIZES = (1, 7, 8, 9, 16384, 16385)                             # the 8-pixel tile's edges and the small-batch switch


@pytest.fixture(scope="module")
def lookup_tables():
    from intrinsicnerf_amd import cluster as ic
    fx = load_golden("cluster_lookup")
    dev = _dev()
    clusters = fixture_clusters(fx, dev)
    assert len(clusters) == 5 and clusters[3] is None               # one class has no cluster
    return {"multi": ic.ClusterTables(clusters, dev), "single": ic.ClusterTables([clusters[4]], dev)}


def _snap_inputs(n, mode, K):
    g = np.random.RandomState(7 * n + len(mode))
    pack = np.zeros((n, SNAP_STRIDE), np.float32)
    pack[:, 1:4] = g.rand(n, 3) * 0.95 + 0.02
    pack[:, 0] = g.rand(n) * 2.0                                      # shading
    pack[:, 5:8] = g.rand(n, 3) - 0.5                                 # residual
    pack[:, 8:] = g.rand(n, 2)
    if mode == "uniform":                                             # one label per 8-pixel tile, walking through -1 .. K + 1
        lab = (np.arange(n) // 8 + 1) % (K + 3) - 1
    else:                                                             # mixed-class tiles
        lab = g.randint(-1, K + 2, size=n)
    lab[0] = 0
    pack[0, 1:4] = 0.0                                                # black: intensity 0, a NaN mapped colour
    if n > 3:
        pack[1, 5:8] = -2.0                                           # edit below 0
        pack[2, 5:8] = 2.0                                            # ... above 1
        pack[3, 0] = np.nan                                           # a NaN shading
    pack[:, 4] = lab
    return pack, lab.astype(np.int64)


@pytest.mark.parametrize("n", SNAP_SIZES)
@pytest.mark.parametrize("mode", ["uniform", "random", "ignore"])
def test_cluster_snap_compose(lookup_tables, n, mode):
    from intrinsicnerf_amd import cluster as ic, frames, kernels
    dev = _dev()
    ignore = mode == "ignore"
    tables = lookup_tables["single" if ignore else "multi"]
    pack_np, lab = _snap_inputs(n, mode, tables.n_classes)
    pack = torch.from_numpy(pack_np).to(dev)
    out, colour = kernels.cluster_snap_compose(tables, pack, SNAP_COLS["albedo"], SNAP_COLS["shading"], SNAP_COLS["residual"],
                                               -1 if ignore else SNAP_COLS["label"], want_color=True)
    c, edit = kernels.snap_images(out, n)
    snapped, _ = ic.lookup(tables, pack[:, 1:4].contiguous(), None if ignore else torch.from_numpy(lab).to(dev), ignore_label=ignore)
    assert torch.equal(colour, snapped)
    s = snapped.cpu().numpy()
    assert np.isfinite(s).all()
    if not ignore:
        outside = (lab < 0) | (lab >= tables.n_classes) | (lab == 3)
        assert np.array_equal(s[outside], pack_np[outside, 1:4]) and (n < 100 or outside.any())
    assert np.array_equal(c.cpu().numpy(), frames.to8b(s))
    edit_f = s * pack_np[:, 0][:, None] + pack_np[:, 5:8]                                  # numpy fp32: a product, then a sum
    nan = np.isnan(edit_f)
    assert nan.any() == (n > 3)
    want_edit = frames.to8b(np.where(nan, np.float32(0), edit_f))                         # NaN -> 0, k_frame_to_u8's rule
    assert np.array_equal(edit.cpu().numpy(), want_edit)
    if n > 3:
        assert (want_edit[1] == 0).all() and (want_edit[2] == 255).all() and (want_edit[3] == 0).all()
    # without the optional output nothing else changes
    out2, none = kernels.cluster_snap_compose(tables, pack, SNAP_COLS["albedo"], SNAP_COLS["shading"], SNAP_COLS["residual"],
                                              -1 if ignore else SNAP_COLS["label"])
    assert none is None and all(torch.equal(a, b) for a, b in zip(kernels.snap_images(out2, n), (c, edit)))


# ---- 3. the fit on device labels and their counts ----------------------------------------------------------------------------------
def test_fit_with_device_labels_and_counts():
    from intrinsicnerf_amd import cluster as ic
    dev = _dev()
    with np.load(GOLD) as z:
        px, lab, K = z["ssr_multi_pixels"], z["ssr_multi_labels"].reshape(-1).astype(np.int64), int(z["ssr_multi_class_num"])
    a = ic.fit(px, lab, K, [0.5] * K)
    counts = np.bincount(lab[(lab >= 0) & (lab < K)], minlength=K)
    lab_dev = torch.from_numpy(lab).to(dev)
    for cnt in (torch.from_numpy(counts.astype(np.int32)).to(dev), counts):
        b = ic.fit(torch.from_numpy(px).to(dev), lab_dev, K, [0.5] * K, counts=cnt)
        for x, y in zip(a.centers + a.anchors + a.links, b.centers + b.anchors + b.links):
            assert (x is None and y is None) or torch.equal(x, y)
        assert torch.equal(a.pixel_label, b.pixel_label) and a.bandwidth == b.bandwidth
        assert np.array_equal(a.counts, b.counts) and np.array_equal(a.sample_idx, b.sample_idx)
    with pytest.raises(ValueError):
        ic.fit(px, lab, K, [0.5] * K, counts=counts)                 # host labels: nothing to leave on the device


# ---- 4. end to end against the host path -------------------------------------------------------------------------------------------
def _read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        (length,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + length]
        pos += 12 + length
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
    w, h, depth, colour = head[:4]
    bpp = {0: 1, 2: 3}[colour] * depth // 8
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * bpp)
    rows = np.zeros((h, w * bpp), np.int64)
    for r in range(h):
        kind, line = int(raw[r, 0]), raw[r, 1:].astype(np.int64)
        up = rows[r - 1] if r else np.zeros(w * bpp, np.int64)
        if kind == 0:
            rows[r] = line
        elif kind == 2:
            rows[r] = (line + up) & 255
        else:
            for x in range(w * bpp):
                left = rows[r, x - bpp] if x >= bpp else 0
                ul = up[x - bpp] if x >= bpp else 0
                if kind == 1:
                    pred = left
                elif kind == 3:
                    pred = (left + up[x]) // 2
                else:
                    p = left + up[x] - ul
                    pa, pb, pc = abs(p - left), abs(p - up[x]), abs(p - ul)
                    pred = left if pa <= pb and pa <= pc else (up[x] if pb <= pc else ul)
                rows[r, x] = (line[x] + pred) & 255
    return rows.astype(np.uint8).reshape(h, w, -1), depth


def _same_managers(a, b):
    assert a.class_num == b.class_num and len(a.clusters) == len(b.clusters)
    for x, y in zip(a.clusters, b.clusters):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x.rgb_centers, y.rgb_centers) and torch.equal(x.anchors, y.anchors) and torch.equal(x.links, y.links)


def _same_outputs(runs, dirs):
    base, base_dir = runs[0], dirs[0]
    names = sorted(os.listdir(base_dir))
    assert any(n.startswith("c0") for n in names) and any(n.startswith("edit") for n in names)
    pngs = {n: _read_png(os.path.join(base_dir, n)) for n in names if n.startswith(("c0", "edit"))}
    for out, d in zip(runs[1:], dirs[1:]):
        assert len(out) == len(base)
        for x, y in zip(base[:-1], out[:-1]):
            assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True)
        _same_managers(base[-1], out[-1])
        assert sorted(os.listdir(d)) == names
        for n, (img, depth) in pngs.items():
            got, got_depth = _read_png(os.path.join(d, n))
            assert got_depth == depth and np.array_equal(got, img), n


def test_object_render_path_refresh_equals_the_host_path(tmp_path):
    import bench
    import intrinsicnerf_amd.cluster as ic
    from intrinsicnerf_amd import object_level as ol, refresh
    from test_frames_gpu import _chair_nets
    dev = _dev()
    side = 48
    K, focal, kw = _chair_nets(dev, side)
    poses = torch.stack([torch.cat([bench.chair_pose(theta_deg=t), torch.tensor([[0., 0., 0., 1.]])], 0) for t in (20., 75.)]).to(dev)
    variants = (dict(cluster_manager_factory=ic.Cluster_Manager), dict(refresh=refresh.ClusterRefresh()),
                dict(refresh=refresh.ClusterRefresh(keep_bytes=1)))
    runs, dirs = [], []
    for j, extra in enumerate(variants):
        d = tmp_path / f"run{j}"
        d.mkdir()
        with torch.no_grad():
            runs.append(ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, savedir=str(d), update_cluster=True, **extra))
        dirs.append(str(d))
    assert isinstance(runs[1][-1], ic.Cluster_Manager) and runs[1][-1].clusters[0] is not None
    _same_outputs(runs, dirs)
    assert sorted(n for n in os.listdir(dirs[1]) if n.startswith(("c0", "edit"))) == ["c000.png", "c001.png", "edit000.png", "edit001.png"]
    with pytest.raises(NotImplementedError):
        with torch.no_grad():
            ol.render_path(poses[:1], (side, side, focal), K, 1 << 15, kw, update_cluster=True)


def test_ssr_render_path_refresh_equals_the_host_path(tmp_path):
    import intrinsicnerf_amd.cluster as ic
    from intrinsicnerf_amd import refresh, ssr
    from oracle import calibration as cal
    dev = _dev()
    H, W, C = 12, 16, 5
    r = ssr.SSRRenderer(C, white_bkgd=False, chunk=100, device=dev)
    r.H_scaled, r.W_scaled, r.near, r.far = H, W, 0.1, 10.0
    r.check_numerics = False
    T = torch.eye(4)[None].repeat(2, 1, 1)
    T[1, :3, 3] = torch.tensor([0.2, 0.0, 0.1])
    rays = ssr.create_rays(2, T.to(dev), H, W, 8.0, 8.0, (W - 1) / 2.0, (H - 1) / 2.0, 0.1, 10.0)
    r.ssr_net_coarse.load_state_dict(cal.calibrated_default_init("ssr", C, 0, rays[0].cpu()))
    r.ssr_net_fine.load_state_dict(cal.calibrated_default_init("ssr", C, 1, rays[0].cpu()))
    r.valid_colour_map = torch.arange(C * 3, dtype=torch.uint8).reshape(C, 3).to(dev)
    assert r.cluster_refresh is None
    with pytest.raises(NotImplementedError):
        with torch.no_grad():
            r.render_path(rays[:1], update_cluster=True)
    runs, dirs = [], []
    for j, (factory, refresher) in enumerate(((ic.Cluster_Manager, None), (None, refresh.ClusterRefresh()),
                                              (None, refresh.ClusterRefresh(keep_bytes=1)))):
        d = tmp_path / f"run{j}"
        d.mkdir()
        r.cluster_manager_factory, r.cluster_refresh = factory, refresher
        with torch.no_grad():
            runs.append(r.render_path(rays, save_dir=str(d), update_cluster=True, b_f=0.4))
        dirs.append(str(d))
    mgr = runs[1][-1]
    assert isinstance(mgr, ic.Cluster_Manager) and mgr.class_num == C and any(c is not None for c in mgr.clusters)
    _same_outputs(runs, dirs)


# ---- 5. graph capture --------------------------------------------------------------------------------------------------------------
def test_both_launches_are_capturable(lookup_tables):
    from intrinsicnerf_amd import kernels
    dev = _dev()
    H, W, K = 12, 16, 5
    frame = torch.from_numpy(_labelled_frame(H, W, K, 5)).to(dev)
    rows = (H // 2) * (W // 2)
    tables = lookup_tables["multi"]
    n = 16385
    pack = torch.from_numpy(_snap_inputs(n, "random", K)[0]).to(dev)

    def fresh():
        return (torch.zeros(rows, 3, device=dev), torch.zeros(rows, dtype=torch.int64, device=dev), torch.zeros(K, dtype=torch.int32, device=dev),
                torch.zeros(2, kernels.snap_row_bytes(n), dtype=torch.uint8, device=dev))

    def launch(px, lab, cnt, out):
        kernels.frame_subsample(frame, H, W, ALBEDO_COL, px, label_col=LABEL_COL, out_labels=lab, class_counts=cnt)
        kernels.cluster_snap_compose(tables, pack, SNAP_COLS["albedo"], SNAP_COLS["shading"], SNAP_COLS["residual"], SNAP_COLS["label"], out=out)

    eager = fresh()
    launch(*eager)
    torch.cuda.synchronize()
    captured = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(*captured)
    for replay in range(2):
        captured[2].zero_()                                           # the counts accumulate: zeroed by the caller once per pass
        captured[0].fill_(-1.0); captured[1].fill_(-1); captured[3].fill_(99)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured[:3], eager[:3]):
            assert torch.equal(got, want), replay
        for got, want in zip(kernels.snap_images(captured[3], n), kernels.snap_images(eager[3], n)):
            assert torch.equal(got, want), replay
