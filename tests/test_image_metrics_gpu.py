"""Intrinsic-image metrics on the device (csrc/imq.hip) against the float64 numpy yardstick (tests/_image_metrics.py).

Shapes: one SSIM position (11 x 11), no LMSE window (19 x 40), the cell / window edge at 29 | 30, the SSIM tile (32 x 16 positions
of the (H-10) x (W-10) valid region) straddled at 25 x 41 | 27 x 43, a 240 x 320 frame, and 267 x 491 at (k, s) = (2, 1), where all
three capped grids (256 workgroups per image and stage) take a second trip.

Tolerances (inputs in [0, 1]; every reduced sum is exact to 64 * 2^-53 * sum|terms| in any tree order):
    mse, si_mse, lmse : derived bound 192 * 2^-53 = 2.1e-14 absolute, asserted at 1e-12
    ssim              : the 11 x 11 filter's cancellation error in sigma^2 (<= ~5e-15) over C2 = 9e-4: ~1.2e-11, asserted at 1e-9
    dssim = (1 - ssim) / 2: half of ssim's; psnr = -10 log10(mse): 10 / ln 10 * 1e-12 / mse
Counts are exact and NaN patterns coincide.  Worst differences measured on an MI355X: profiles/image_metrics.txt (-s prints them)."""
import functools
import os

import numpy as np
import pytest
import torch

import _image_metrics as M

pytestmark = pytest.mark.gpu

TOL = {"mse": 1e-12, "si_mse": 1e-12, "lmse": 1e-12, "ssim": 1e-9, "dssim": 0.5e-9}
CASES = M.case_table()


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def _case(name):
    """(pred, target, mask, k, s, the helper's metrics) of a named case: built and evaluated once, shared, left unchanged."""
    kw, k, s = CASES[name]
    pred, target, mask = M.make_case(**kw)
    for a in (pred, target, mask):
        if a is not None:
            a.setflags(write=False)
    return pred, target, mask, k, s, M.metrics(pred, target, mask, k, s)


def _up(a):
    return None if a is None else torch.tensor(a, device=_dev())


def _check(got, counts, want, what, report=True):
    """One image's finished metrics and counts against the helper's."""
    assert [int(v) for v in counts] == [want["n_valid"], want["n_windows"], want["n_ssim"]], (what, counts)
    worst = {}
    for key in M.KEYS:
        g, w = float(got[key]), float(want[key])
        assert np.isnan(g) == np.isnan(w), (what, key, g, w)
        if np.isnan(w):
            continue
        tol = TOL[key] if key != "psnr" else 10.0 / np.log(10.0) * 1e-12 / want["mse"]
        worst[key] = abs(g - w)
        if report:
            print(f"{what:44s} {key:7s} |diff| = {abs(g - w):.3e}  (tolerance {tol:.3e})")
        assert abs(g - w) <= tol, (what, key, g, w)
    return worst


def _run(pred, target, mask, k, s, **kw):
    from intrinsicnerf_amd import evaluation, kernels
    sums, counts = kernels.image_quality(pred, target, mask, window_size=k, window_shift=s, **kw)
    assert sums.dtype == torch.float64 and counts.dtype == torch.int64 and sums.is_cuda and counts.is_cuda
    return sums, counts, evaluation.finish_image_quality(sums[0].cpu().numpy(), counts[0].cpu().numpy(), pred.shape[-1])


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_helper(name):
    pred, target, mask, k, s, want = _case(name)
    sums, counts, got = _run(_up(pred), _up(target), _up(mask), k, s)
    assert sums.shape == (1, 7) and counts.shape == (1, 3)
    _check(got, counts[0].cpu().numpy(), want, name)
    if name == "11x11x3":
        assert want["n_ssim"] == 1 and want["n_windows"] == 0 and np.isnan(got["lmse"])
    if name == "19x40x1":
        assert want["n_windows"] == 0 and np.isnan(got["lmse"]) and not np.isnan(got["ssim"])
    if "mask zero" in name:
        assert want["n_valid"] == 0 and all(np.isnan(got[key]) for key in M.KEYS)
    if "nan pixel" in name:
        assert all(np.isnan(got[key]) for key in M.KEYS)              # the pixel lies in a window and under the filter
    # the plain sums (Spp, Spg, Sgg, S(g-p)^2, the LMSE denominator) are the helper's own to summation rounding
    want_sums, _ = M.sums_and_counts(pred, target, mask, k, s)
    got_sums = sums[0].cpu().numpy()
    for i in (0, 1, 2, 3, 5):
        if not np.isnan(want_sums[i]):
            assert abs(got_sums[i] - want_sums[i]) <= 64 * 2.0 ** -53 * max(1.0, abs(want_sums[i]) * 2), (i, got_sums[i], want_sums[i])


def test_unsupported_window_and_argument_errors():
    from intrinsicnerf_amd import kernels
    pred, target, _, _, _, _ = _case("45x67x3")
    p, g = _up(pred), _up(target)
    with pytest.raises(RuntimeError, match="unsupported"):
        kernels.image_quality(p, g, window_size=20, window_shift=7)
    with pytest.raises(RuntimeError, match="unsupported"):
        kernels.image_quality(p, g, window_size=18, window_shift=2)
    with pytest.raises(ValueError):
        kernels.image_quality(p, g[:, :60])
    with pytest.raises(ValueError):
        kernels.image_quality(p[..., :2], g[..., :2])
    with pytest.raises(ValueError):
        kernels.image_quality(p.double(), g.double())
    with pytest.raises(RuntimeError, match="HIP device"):
        kernels.image_quality(p.cpu(), g.cpu())


@pytest.mark.parametrize("channels", [1, 3])
def test_columns_of_a_pack(channels):
    """Inputs as column ranges of an 11-wide pack [H * W, 11] (and the mask as one of its columns): read where they are."""
    from intrinsicnerf_amd import evaluation, kernels
    name = f"45x67x{channels} mask random"
    pred, target, mask, k, s, want = _case(name)
    h, w = mask.shape
    pack = torch.full((h * w, 11), float("nan"), device=_dev())
    pack[:, 1:1 + channels] = _up(pred).reshape(h * w, channels)
    pack[:, 5:5 + channels] = _up(target).reshape(h * w, channels)
    pack[:, 9] = _up(mask).reshape(-1)
    p, g, m = pack[:, 1:1 + channels], pack[:, 5:5 + channels], pack[:, 9]
    assert not p.is_contiguous() and m.stride(0) == 11
    sums, counts = kernels.image_quality(p, g, m, shape=(h, w), window_size=k, window_shift=s)
    direct = kernels.image_quality(_up(pred), _up(target), _up(mask), window_size=k, window_shift=s)
    assert sums.cpu().numpy().tobytes() == direct[0].cpu().numpy().tobytes() and torch.equal(counts, direct[1])
    _check(evaluation.finish_image_quality(sums[0].cpu().numpy(), counts[0].cpu().numpy(), channels), counts[0].cpu().numpy(), want,
           name + " (pack)")
    # the [H, W, C] view of the same columns
    again = kernels.image_quality(p.reshape(h, w, channels), g.reshape(h, w, channels), m.reshape(h, w), window_size=k, window_shift=s)
    assert again[0].cpu().numpy().tobytes() == sums.cpu().numpy().tobytes()


def test_a_stack_equals_single_calls_bit_for_bit():
    from intrinsicnerf_amd import kernels
    names = ["45x67x3 mask random", "45x67x3 mask window", "45x67x3 nan pixel"]
    cases = [_case(n) for n in names]
    p = torch.stack([_up(c[0]) for c in cases])
    g = torch.stack([_up(c[1]) for c in cases])
    m = torch.stack([_up(c[2]) if c[2] is not None else torch.ones(45, 67, device=_dev()) for c in cases])
    sums, counts = kernels.image_quality(p, g, m)
    assert sums.shape == (3, 7) and counts.shape == (3, 3)
    for i in range(3):
        one_s, one_c = kernels.image_quality(p[i], g[i], m[i])
        assert one_s.cpu().numpy().tobytes() == sums[i:i + 1].cpu().numpy().tobytes(), names[i]
        assert torch.equal(one_c, counts[i:i + 1])


def test_two_runs_and_a_graph_replay_give_the_same_bytes():
    from intrinsicnerf_amd import kernels
    pred, target, mask, k, s, _ = _case("240x320x3 mask random")
    p, g, m = _up(pred), _up(target), _up(mask)
    first = kernels.image_quality(p, g, m)
    second = kernels.image_quality(p, g, m)
    assert first[0].cpu().numpy().tobytes() == second[0].cpu().numpy().tobytes() and torch.equal(first[1], second[1])
    ws = torch.empty(kernels.image_quality_workspace_bytes(1, 240, 320, 3) // 8, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sums, counts = kernels.image_quality(p, g, m, workspace=ws)
    for _ in range(2):
        sums.fill_(-1.0); counts.fill_(-1); ws.fill_(float("nan"))          # written, not added; nothing left over is read
        graph.replay()
        torch.cuda.synchronize()
        assert sums.cpu().numpy().tobytes() == first[0].cpu().numpy().tobytes() and torch.equal(counts, first[1])


def test_intrinsic_image_metrics_on_a_stack():
    from intrinsicnerf_amd import evaluation
    names = ["45x67x3 mask random", "45x67x3 mask window", "45x67x3 black window"]
    cases = [_case(n) for n in names]
    pred, target = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    mask = np.stack([c[2] if c[2] is not None else np.ones((45, 67), np.float32) for c in cases])
    out = evaluation.intrinsic_image_metrics(pred, torch.from_numpy(target).to(_dev()), mask)
    assert list(out) == ["frames", "mean"] and len(out["frames"]) == 3
    for name, c, f in zip(names, cases, out["frames"]):
        want = c[5] if c[2] is not None else M.metrics(c[0], c[1], np.ones((45, 67)))
        _check(f, [want["n_valid"], want["n_windows"], want["n_ssim"]], want, name + " (stack)", report=False)
    for key in M.KEYS:
        assert out["mean"][key] == np.mean([f[key] for f in out["frames"]])
    # [H, W] is read as one channel; a NaN frame stays visible in the mean
    p1, g1, _, _, _, w1 = _case("29x30x1")
    one = evaluation.intrinsic_image_metrics(p1[..., 0], g1[..., 0])
    _check(one["frames"][0], [w1["n_valid"], w1["n_windows"], w1["n_ssim"]], w1, "29x30 map", report=False)
    nan = evaluation.intrinsic_image_metrics(np.stack([cases[0][0], _case("45x67x3 nan pixel")[0]]), np.stack([cases[0][1]] * 2))
    assert np.isnan(nan["mean"]["ssim"]) and not np.isnan(nan["frames"][0]["ssim"])
    lm = evaluation.intrinsic_image_metrics(cases[0][0], cases[0][1], cases[0][2], window_size=16, window_shift=16)
    assert abs(lm["frames"][0]["lmse"] - M.lmse(cases[0][0], cases[0][1], cases[0][2], 16, 16)[0]) <= 1e-12


def test_frame_evaluator_image_quality_groups():
    """albedo=, shading=, mask= and shape=: results() equals the helper frame by frame, and the three existing groups are those of
    an evaluator without the new targets, bit for bit."""
    from intrinsicnerf_amd import evaluation
    dev, n, h, w, classes = _dev(), 3, 29, 30, 4
    rng = np.random.default_rng(77)
    frames = [M.make_case(h, w, 3, seed=300 + i) for i in range(n)]
    gt_rgb, rgb = np.stack([f[1] for f in frames]), np.stack([f[0] for f in frames])
    alb = [M.make_case(h, w, 3, seed=310 + i) for i in range(n)]
    gt_alb, albedo = np.stack([f[1] for f in alb]), np.stack([f[0] for f in alb])
    shd = [M.make_case(h, w, 1, seed=320 + i) for i in range(n)]
    gt_shd, shading = np.stack([f[1] for f in shd])[..., 0], np.stack([f[0] for f in shd])
    mask = (rng.random((n, h, w)) < 0.7).astype(np.float32)
    gt_depth = (rng.random((n, h, w)) * 4 + 0.5).astype(np.float32)
    depth = (gt_depth * (1 + 0.1 * rng.standard_normal((n, h, w)))).astype(np.float32)
    true = rng.integers(-1, classes, (n, h * w))
    logits = rng.standard_normal((n, h * w, classes)).astype(np.float32)
    rays = [object() for _ in range(n)]

    def run(**extra):
        ev = evaluation.FrameEvaluator(classes)
        ev.register(rays, image=gt_rgb, depth=gt_depth, semantic=true, **extra)
        assert ev.begin(rays)
        for i in range(n):
            more = dict(albedo=_up(albedo[i]), shading=_up(shading[i])) if extra else {}
            ev.add_frame(i, logits=_up(logits[i]), depth=_up(depth[i]), rgb=_up(rgb[i]).reshape(-1, 3), **more)
        return ev, ev.results()

    _, base = run()
    ev, out = run(albedo=gt_alb, shading=gt_shd, mask=mask, shape=(h, w))
    assert list(base) == ["segmentation", "depth", "image"]
    assert list(out) == ["segmentation", "depth", "image", "image_quality", "albedo", "shading"]
    for a, b in zip(base["segmentation"][None], out["segmentation"][None]):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    assert base["depth"] == out["depth"] and base["image"] == out["image"]
    for key, preds, targets in (("image_quality", rgb, gt_rgb), ("albedo", albedo, gt_alb), ("shading", shading, gt_shd)):
        assert list(out[key]) == ["frames", "mean"] and list(out[key]["frames"]) == list(range(n))
        for i in range(n):
            want = M.metrics(preds[i], targets[i].reshape(preds[i].shape), mask[i])
            _check(out[key]["frames"][i], [want["n_valid"], want["n_windows"], want["n_ssim"]], want, f"{key} frame {i}", report=False)
        for k2 in M.KEYS:
            assert out[key]["mean"][k2] == np.mean([out[key]["frames"][i][k2] for i in range(n)])
    # a group appears only when it was seen; reset() forgets the rows
    ev.reset()
    ev.begin(rays)
    ev.add_frame(1, albedo=_up(albedo[1]))
    again = ev.results()
    assert "albedo" in again and "shading" not in again and "image_quality" not in again and list(again["albedo"]["frames"]) == [1]
    assert again["albedo"]["frames"][1] == out["albedo"]["frames"][1]
    with pytest.raises(ValueError, match="shape"):
        evaluation.FrameEvaluator(classes).register(rays, albedo=gt_alb)


def test_object_render_path_with_an_evaluator(tmp_path):
    """A 24 x 24 frame pair, default-init networks, 8 + 8 samples: the same stacks and files as without the evaluator, and its
    metrics are the helper's on the rendered maps."""
    import bench
    from intrinsicnerf_amd import evaluation
    from intrinsicnerf_amd import object_level as ol
    dev, side = _dev(), 24
    focal = 0.5 * side / np.tan(0.5 * bench.CAMERA_ANGLE_X)
    K = np.array([[focal, 0, 0.5 * side], [0, focal, 0.5 * side], [0, 0, 1]])
    embed, ch = ol.get_embedder(10, 0)
    embed_d, ch_d = ol.get_embedder(4, 0)
    torch.manual_seed(4)
    mk = lambda: ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
    kw = dict(network_fn=mk(), network_fine=mk(), network_query_fn=ol.NetworkQuery(embed, embed_d), N_samples=8, N_importance=8,
              white_bkgd=True, perturb=False, raw_noise_std=0., use_viewdirs=True, ndc=False, lindisp=False, near=2., far=6.)
    poses = torch.stack([torch.cat([bench.chair_pose(theta_deg=t), torch.tensor([[0., 0., 0., 1.]])], 0) for t in (20., 75.)]).to(dev)
    rng = np.random.default_rng(5)
    with torch.no_grad():
        maps = [[m.detach().cpu().numpy() for m in ol.render(side, side, K, chunk=1 << 15, c2w=p[:3, :4], **kw)[:6]] for p in poses]
    shading_shape = maps[0][4].shape
    gt_rgb, gt_alb = rng.random((2, side, side, 3), dtype=np.float32), rng.random((2, side, side, 3), dtype=np.float32)
    gt_shd = rng.random((2,) + shading_shape, dtype=np.float32)
    alpha = (rng.random((2, side, side)) < 0.7).astype(np.float32)
    ev = evaluation.FrameEvaluator(1)
    ev.register(poses, image=gt_rgb, albedo=gt_alb, shading=gt_shd, mask=alpha, shape=(side, side))
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    with torch.no_grad():
        base = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, savedir=str(tmp_path / "a"))
        out = ol.render_path(poses, (side, side, focal), K, 1 << 15, kw, savedir=str(tmp_path / "b"), evaluator=ev)
        other = ol.render_path(list(poses), (side, side, focal), K, 1 << 15, kw, evaluator=ev)        # not registered: left alone
    assert np.array_equal(base[0], out[0]) and np.array_equal(base[1], out[1], equal_nan=True) and out[2] is None
    assert np.array_equal(base[0], other[0])
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 10
    for name in names:
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    res = ev.results()
    assert list(res) == ["segmentation", "depth", "image", "image_quality", "albedo", "shading"] and res["image"] is not None
    for key, col, gt in (("image_quality", 0, gt_rgb), ("albedo", 3, gt_alb), ("shading", 4, gt_shd)):
        assert list(res[key]["frames"]) == [0, 1]
        for i in range(2):
            pred = maps[i][col]
            if col == 0:
                assert np.array_equal(pred, out[0][i])
            c = 3 if col != 4 else int(np.prod(shading_shape[2:], dtype=np.int64))
            want = M.metrics(pred.reshape(side, side, c), gt[i].reshape(side, side, c), alpha[i])
            _check(res[key]["frames"][i], [want["n_valid"], want["n_windows"], want["n_ssim"]], want, f"render_path {key} {i}", report=False)
