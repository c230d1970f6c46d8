"""Mean-shift fit of the albedo clusters on the GPU (csrc/cluster_fit.hip) against the reference + sklearn fixtures
(tests/golden/cluster_fit.npz, make_golden_cluster_fit.py), invariants on training-size inputs, and the end-to-end
paths (render_path(update_cluster=True) with the package's Cluster_Manager, save / load)."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "cluster_fit.npz")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def _voxel_dist(p):
    """choose_anchors' torch expressions (cluster.py:168-170) on the CPU: (voxel id [n,3], dist [n])."""
    p = torch.from_numpy(p)
    vid = torch.clamp((p / 0.01).long(), 0, 99)
    return vid, torch.sum((vid * 0.01 + 0.005 - p) ** 2, dim=1)


def _match(ours, ref, tol):
    """index of our centre for every reference centre (one-to-one, each within tol)."""
    d = torch.cdist(torch.from_numpy(ref).double(), torch.from_numpy(ours).double())
    m = d.argmin(1).numpy()
    assert len(set(m.tolist())) == len(m), f"two reference centres share one fitted centre: {d}"
    worst = float(d[np.arange(len(m)), m].max())
    assert worst <= tol, f"centre off by {worst:.3e} > {tol:.3e}"
    return m


def _check_class(gold, key, pixels_c, factor, res, c):
    import intrinsicnerf_amd.cluster as ic  # noqa: F401
    n_c = pixels_c.shape[0]
    bw = float(gold[f"{key}_bw"])
    # classes of <= 11 pixels: sklearn's NearestNeighbors(n_neighbors=5) switches to the float32 brute-force path, whose
    # distances (|x|^2 + |y|^2 - 2xy) differ from the exact fp64 ones by rounding: points at the radius may fall on the
    # other side, so only the bandwidth (kd-tree up to 3 pixels, floor below) and the centre count are compared exactly
    tiny = n_c <= 11
    assert abs(res.bandwidth[c] - bw) <= 1e-9 * bw, (key, res.bandwidth[c], bw)
    ref_c = gold[f"{key}_centers_mapped"]
    ours_c = res.mapped_centers[c].cpu().numpy()
    assert ours_c.shape == ref_c.shape, (key, ours_c.shape, ref_c.shape)
    assert int(res.stats[c, 1]) == int(gold[f"{key}_n_seeds"]), (key, res.stats[c], int(gold[f"{key}_n_seeds"]))
    tol = 5 * 1e-3 * bw
    m = _match(ours_c, ref_c, tol)
    rgb = res.centers[c].cpu().numpy()
    assert np.abs(rgb[m] - gold[f"{key}_rgb_centers"]).max() <= 1e-5
    # labels_: ours mapped to the reference's centre order
    inv = np.empty(len(m), np.int64)
    inv[m] = np.arange(len(m))
    ours_l = inv[res.labels_c[c]]
    ref_l = gold[f"{key}_labels"]
    bad = np.nonzero(ours_l != ref_l)[0]
    mapped = torch.from_numpy(res.mapped_points[c]).double()
    if len(bad):
        assert tiny or len(bad) <= 1e-3 * n_c, (key, len(bad), n_c)
        rc = torch.from_numpy(ref_c).double()
        d_ours = (mapped[bad] - rc[ours_l[bad]]).norm(dim=1)
        d_ref = (mapped[bad] - rc[ref_l[bad]]).norm(dim=1)
        assert float((d_ours - d_ref).abs().max()) <= tol, f"{key}: a label mismatch that is not a near-tie"
    # anchors: bit-equal, links equal - except voxels whose winning dist ties or whose pixel is a tolerated mismatch
    a_ours, l_ours = res.anchors[c].cpu().numpy(), res.links[c].cpu().numpy().reshape(-1)
    a_ref, l_ref = gold[f"{key}_anchors"], gold[f"{key}_links"].reshape(-1)
    assert a_ours.shape == a_ref.shape and a_ours.dtype == np.float32
    assert res.links[c].dtype == torch.int64 and tuple(res.links[c].shape) == (a_ref.shape[0], 1)
    vid, dist = _voxel_dist(res.mapped_points[c])
    flat = (vid[:, 0] * 100 + vid[:, 1]) * 100 + vid[:, 2]
    best = torch.full((10 ** 6,), float("inf")).scatter_reduce(0, flat, dist, "amin")
    ties = torch.zeros(10 ** 6, dtype=torch.long).index_add_(0, flat, (dist == best[flat]).long())
    diff = np.nonzero(np.any(a_ours != a_ref, axis=1) | (inv[l_ours] != l_ref))[0]
    bad_set = set(bad.tolist())
    row_of = {tuple(r): i for i, r in enumerate(res.mapped_points[c].tolist())}
    for a in diff:
        v = int(flat[row_of[tuple(a_ref[a].tolist())]])
        pixel = row_of[tuple(a_ours[a].tolist())]
        assert ties[v] > 1 or pixel in bad_set, f"{key}: anchor {a} differs without a tie"


def _fit_case(gold, case):
    import intrinsicnerf_amd.cluster as ic
    px = gold[f"{case}_pixels"]
    if case == "cluster_f08":
        cl = ic.Cluster(intensity_factor=float(gold["cluster_f08_factor"]))
        res = ic.fit_cluster(cl, px, band_factor=float(gold["cluster_f08_band_factor"]))
        return res, [px], [float(gold["cluster_f08_factor"])], cl
    K = int(gold[f"{case}_class_num"])
    mgr = ic.Cluster_Manager(class_num=K)
    res = ic.update_center(mgr, gold[f"{case}_labels"], px, band_factor=float(gold[f"{case}_band_factor"]))
    lab = gold[f"{case}_labels"].reshape(-1)
    sets = [px] if K == 1 else [px[lab == c] for c in range(K)]
    return res, sets, [0.5] * K, mgr


def _attach(res, sets, factors):
    """per-class labels_ and mapped points (the reference's mapping_color_np in numpy fp32) for the comparisons."""
    pl = res.pixel_label.cpu().numpy()
    res.labels_c, res.mapped_points = [], []
    K = len(sets)
    lab = None if K == 1 else res._labels
    for c, s in enumerate(sets):
        I = np.sum(s, axis=-1)
        d = np.zeros_like(s)
        d[..., 0] = I / 3.0 * np.float32(factors[c])
        d[..., 1] = s[..., 1] / I
        d[..., 2] = s[..., 2] / I
        res.mapped_points.append(d)
        res.labels_c.append(pl if lab is None else pl[lab == c])


@pytest.mark.parametrize("case", ["ssr_multi", "ssr_single", "cluster_f08"])
def test_fit_matches_reference(gold, case):
    res, sets, factors, owner = _fit_case(gold, case)
    res._labels = None if len(sets) == 1 else gold[f"{case}_labels"].reshape(-1)
    _attach(res, sets, factors)
    clusters = owner.clusters if hasattr(owner, "clusters") else [owner]
    for c, s in enumerate(sets):
        key = f"{case}_c{c}"
        if f"{key}_none" in gold:
            assert clusters[c] is None and len(s) == 0
            continue
        cl = clusters[c]
        assert cl.anchors.dtype == torch.float32 and cl.rgb_centers.dtype == torch.float32 and cl.links.dtype == torch.int64
        assert cl.anchors.is_cuda and cl.rgb_centers.shape[1] == 3
        _check_class(gold, key, s, factors[c], res, c)


def test_manager_method_fails_without_feature_and_works_with_it(gold):
    import intrinsicnerf_amd.cluster as ic
    mgr = ic.Cluster_Manager(class_num=int(gold["ssr_multi_class_num"]))
    mgr.update_center(gold["ssr_multi_labels"], gold["ssr_multi_pixels"], band_factor=0.5)
    assert mgr.clusters[1] is None and all(c is not None for i, c in enumerate(mgr.clusters) if i != 1)
    assert mgr.clusters[0].rgb_centers.shape == gold["ssr_multi_c0_rgb_centers"].shape


def test_fit_is_bit_identical_and_accepts_tensors(gold):
    import intrinsicnerf_amd.cluster as ic
    px, lab = gold["ssr_multi_pixels"], gold["ssr_multi_labels"]
    a = ic.fit(px, lab, 6, [0.5] * 6)
    b = ic.fit(torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda(), 6, [0.5] * 6)
    for x, y in zip(a.centers + a.anchors + a.links, b.centers + b.anchors + b.links):
        assert (x is None and y is None) or torch.equal(x, y)
    assert torch.equal(a.pixel_label, b.pixel_label)


def test_cpu_device_raises():
    import intrinsicnerf_amd.cluster as ic
    with pytest.raises(RuntimeError):
        ic.Cluster_Manager(class_num=1, device="cpu").update_center(np.zeros((4, 1)), np.full((4, 3), 0.5, np.float32))


def test_nonfinite_raises():
    import intrinsicnerf_amd.cluster as ic
    px = np.full((64, 3), 0.5, np.float32)
    px[3] = 0.0
    with pytest.raises(ValueError):
        ic.Cluster().update_center(px)


def _synthetic(n, K, seed):
    g = torch.Generator().manual_seed(seed)
    modes = torch.rand(K, 6, 3, generator=g) * 0.8 + 0.1
    lab = torch.randint(0, K, (n,), generator=g)
    pick = torch.randint(0, 6, (n,), generator=g)
    shade = torch.rand(n, 1, generator=g) * 0.6 + 0.6
    px = (modes[lab, pick] * shade + 0.02 * torch.randn(n, 3, generator=g)).clamp(0.01, 1.0)
    return px, lab


def _invariants(px, lab, K, res):
    dev = torch.device("cuda")
    px_np, lab_np = px.numpy(), lab.numpy()
    pl = res.pixel_label
    for c in range(K):
        sel_np = np.nonzero(lab_np == c)[0] if K > 1 else np.arange(px_np.shape[0])
        if sel_np.size == 0:
            continue
        sel = torch.from_numpy(sel_np).to(dev)
        s = px_np[sel_np]
        I = np.sum(s, axis=-1)                          # mapping_color_np (cluster.py:316-322), numpy fp32 on the host
        d_np = np.zeros_like(s)
        d_np[..., 0] = I / 3.0 * 0.5
        d_np[..., 1] = s[..., 1] / I
        d_np[..., 2] = s[..., 2] / I
        d = torch.from_numpy(d_np).to(dev)
        bw = res.bandwidth[c]
        stop = 1e-3 * bw
        ctr = res.mapped_centers[c].double()
        dd = d.double()
        if ctr.shape[0] > 1:
            pd = torch.cdist(ctr, ctr) + torch.eye(ctr.shape[0], device=dev, dtype=torch.float64) * 1e9
            assert float(pd.min()) > bw * (1 - 1e-12), f"class {c}: two centres within bw"
        dmin = torch.full((sel.numel(),), float("inf"), device=dev, dtype=torch.float64)
        arg = torch.zeros(sel.numel(), dtype=torch.long, device=dev)
        sums = torch.zeros(ctr.shape[0], 3, device=dev, dtype=torch.float64)
        cnts = torch.zeros(ctr.shape[0], device=dev, dtype=torch.float64)
        for i in range(ctr.shape[0]):
            t = (dd - ctr[i]) ** 2
            r2 = (t[:, 0] + t[:, 1]) + t[:, 2]                  # the kernel's fp64 order
            take = r2 < dmin
            dmin, arg = torch.where(take, r2, dmin), torch.where(take, torch.full_like(arg, i), arg)
            w = (r2 <= bw * bw).double()
            sums[i] = (dd * w[:, None]).sum(0)
            cnts[i] = w.sum()
        shift = (sums / cnts[:, None] - ctr).norm(dim=1)
        assert float(shift.max()) <= 2 * stop, f"class {c}: a centre is not a fixed point ({float(shift.max()):.3e})"
        assert torch.equal(pl[sel].long(), arg), f"class {c}: labels are not the fp64 argmin"
        vid, dist = _voxel_dist(d_np)                  # choose_anchors' torch expressions on the CPU, as in the fixtures
        vid, dist = vid.to(dev), dist.to(dev)
        flat = (vid[:, 0] * 100 + vid[:, 1]) * 100 + vid[:, 2]
        best = torch.full((10 ** 6,), float("inf"), device=dev).scatter_reduce(0, flat, dist, "amin")
        occupied = torch.unique(flat)
        anc = res.anchors[c]
        assert anc.shape[0] == occupied.numel(), f"class {c}: not one anchor per occupied voxel"
        avid, adist = _voxel_dist(anc.cpu().numpy())
        aflat = ((avid[:, 0] * 100 + avid[:, 1]) * 100 + avid[:, 2]).to(dev)
        assert torch.equal(aflat, occupied), f"class {c}: anchors not in voxel C-order"
        assert torch.equal(adist.to(dev), best[aflat]), f"class {c}: an anchor is not its voxel's minimum-dist pixel"


@pytest.mark.parametrize("n,K", [(3_460_000, 28), (1_000_000, 1)])
def test_large_inputs_invariants(n, K):
    import intrinsicnerf_amd.cluster as ic
    px, lab = _synthetic(n, K, 7 + K)
    res = ic.fit(px, lab if K > 1 else None, K, [0.5] * K)
    again = ic.fit(px, lab if K > 1 else None, K, [0.5] * K)
    for x, y in zip(res.mapped_centers + res.anchors + res.links, again.mapped_centers + again.anchors + again.links):
        assert (x is None and y is None) or torch.equal(x, y)
    assert torch.equal(res.pixel_label, again.pixel_label)
    _invariants(px, lab, K, res)


def test_single_class_manager_lookup_and_save_load(tmp_path, gold):
    import intrinsicnerf_amd.cluster as ic
    mgr = ic.Cluster_Manager(class_num=1)
    px = gold["ssr_single_pixels"]
    mgr.update_center(np.zeros((px.shape[0], 1), bool), px, band_factor=0.5)
    rgb = torch.from_numpy(px[:4096]).cuda()
    label = torch.zeros(4096, 1, dtype=torch.long, device="cuda")
    got = mgr.dest_color(rgb, label)
    want, _ = ic.lookup(ic.ClusterTables(mgr.clusters, rgb.device), rgb, ignore_label=True)
    assert torch.equal(got, want.squeeze())
    mgr.save(str(tmp_path / "m"))
    back = ic.Cluster_Manager(cluster_config_file=str(tmp_path / "m"), device="cuda")
    assert torch.equal(back.dest_color(rgb, label), got)
    assert torch.equal(back.dest_class(rgb, label), mgr.dest_class(rgb, label))


def test_object_render_path_update_cluster(tmp_path):
    import bench
    import intrinsicnerf_amd.cluster as ic
    from intrinsicnerf_amd import object_level as ol
    from test_frames_gpu import _chair_nets
    dev = torch.device("cuda", torch.cuda.current_device())
    side = 48
    K, focal, kw = _chair_nets(dev, side)
    poses = torch.stack([torch.cat([bench.chair_pose(theta_deg=t), torch.tensor([[0., 0., 0., 1.]])], 0) for t in (20., 75.)]).to(dev)
    with torch.no_grad():
        _, _, mgr = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, savedir=str(tmp_path), update_cluster=True,
                                   cluster_manager_factory=ic.Cluster_Manager)
    assert isinstance(mgr, ic.Cluster_Manager) and mgr.clusters[0] is not None
    rgb = torch.rand(2000, 3, device=dev) * 0.9 + 0.05
    label = torch.zeros(2000, 1, dtype=torch.long, device=dev)
    want, _ = ic.lookup(ic.ClusterTables(mgr.clusters, dev), rgb, ignore_label=True)
    assert torch.equal(mgr.dest_color(rgb, label), want)
    mgr.save(str(tmp_path / "m"))
    back = ic.Cluster_Manager(cluster_config_file=str(tmp_path / "m"), device=dev)
    assert torch.equal(back.dest_color(rgb, label), want)


def test_ssr_render_path_update_cluster(tmp_path):
    import intrinsicnerf_amd.cluster as ic
    from intrinsicnerf_amd import ssr
    from oracle import calibration as cal
    dev = torch.device("cuda", torch.cuda.current_device())
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
    r.cluster_manager_factory = ic.Cluster_Manager
    with torch.no_grad():
        out = r.render_path(rays, save_dir=str(tmp_path), update_cluster=True, b_f=0.4)
    mgr = out[-1]
    assert isinstance(mgr, ic.Cluster_Manager) and mgr.class_num == C and len(mgr.clusters) == C
    assert any(c is not None for c in mgr.clusters)
    rgb = torch.rand(3000, 3, device=dev) * 0.9 + 0.05
    label = torch.randint(0, C, (3000, 1), device=dev)
    want, _ = ic.lookup(ic.ClusterTables(mgr.clusters, dev), rgb, label)
    assert torch.equal(mgr.dest_color(rgb, label), want)
    mgr.save(str(tmp_path / "m"))
    back = ic.Cluster_Manager(cluster_config_file=str(tmp_path / "m"), device=dev)
    assert torch.equal(back.dest_color(rgb, label), want)
