"""Validation metrics on the device (csrc/eval.hip, intrinsicnerf_amd/evaluation.py) against the CPU references of _evaluation.py.

Sizes, next to the kernel's constants: a wave takes a tile of 64 pixels and a workgroup four of them, so n sits either side of 64
and 256 (1, 63, 64, 65, 255, 256, 257) and at 4 099 (17 workgroups, a ragged last tile); the accumulate grid is capped at 512
workgroups, so 512 * 256 + 65 pixels give some workgroups a second trip.  C = 1, 2, 3, 28, 64, 240 take 1, 2, 4, 32, 64 and 64 lanes
per logits row (four logits per lane at 240); the confusion table lives in LDS up to C = 64 and goes through global atomics above:
63 | 64 | 65.

Entropy yardstick (the project's own, tests/_raw_rows.py): |got - H64| <= 4 D + 2^-21 max(1, |H64|) with D the error of the
reference's fp32 expression on the CPU for the same case.  Worst err / bound measured on an MI355X: profiles/evaluation.txt."""
import numpy as np
import pytest
import torch

import _evaluation as V

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 67


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _guarded(n):
    """([GUARD + n + GUARD] sentinel-filled buffer, its middle [n])."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=_dev())
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


@pytest.mark.parametrize("n_classes", V.CLASSES)
def test_sem_maps_labels_and_entropy(n_classes):
    from intrinsicnerf_amd import kernels
    worst = 0.0
    for n in V.N_SIZES:
        want_label, _, _, _ = V.logit_reference(n, n_classes)
        x = V.logit_case(n, n_classes).to(_dev())
        lbuf, label = _guarded(n)
        ebuf, entropy = _guarded(n)
        got = kernels.sem_maps(x, label=label, entropy=entropy)
        assert got[0] is label and got[1] is entropy
        assert _guards_intact(lbuf, n) and _guards_intact(ebuf, n)
        assert np.array_equal(label.cpu().numpy(), want_label.astype(np.float32)), (n, n_classes)          # every row, the special ones included
        ratio, msg = V.entropy_judgement(entropy.cpu().numpy(), n, n_classes)
        print(f"C = {n_classes:3d}  n = {n:5d}  entropy err / bound = {ratio:.3f}")
        assert msg is None, (n, n_classes, msg)
        worst = max(worst, ratio)
    print(f"C = {n_classes:3d}  worst entropy err / bound = {worst:.3f}")


def test_sem_maps_into_strided_pack_columns_and_from_a_padded_logits_view():
    """Outputs as columns 1 and 4 of a [n, 7] pack (a 4-byte offset from the row start, 28 bytes apart), logits as columns 3 .. 30 of
    a [n, 33] tensor: everything else keeps its sentinel; one output alone leaves the other buffer untouched."""
    from intrinsicnerf_amd import kernels
    n, n_classes = 257, 28
    want_label, _, _, _ = V.logit_reference(n, n_classes)
    wide = torch.full((n, 33), float("nan"), device=_dev())
    wide[:, 3:31] = V.logit_case(n, n_classes).to(_dev())
    pack = torch.full((n, 7), SENTINEL, device=_dev())
    kernels.sem_maps(wide[:, 3:31], label=pack[:, 1], entropy=pack[:, 4])
    host = pack.cpu().numpy()
    assert np.array_equal(host[:, 1], want_label.astype(np.float32))
    assert V.entropy_judgement(host[:, 4], n, n_classes)[1] is None
    assert (host[:, [0, 2, 3, 5, 6]] == SENTINEL).all()
    label, entropy = kernels.sem_maps(wide[:, 3:31], want_entropy=False)
    assert entropy is None and np.array_equal(label.cpu().numpy(), host[:, 1])
    label, entropy = kernels.sem_maps(wide[:, 3:31], want_label=False)
    assert label is None and np.array_equal(entropy.cpu().numpy(), host[:, 4], equal_nan=True)


def _accumulate(n_classes, ignore=-1, workspace=None, **groups):
    from intrinsicnerf_amd import kernels
    counts, sums = kernels.eval_tables(n_classes, _dev())
    maps = kernels.eval_accumulate(counts, sums, n_classes, ignore, workspace=workspace, **{k: v.to(_dev()) for k, v in groups.items()})
    return counts, sums, maps


def _check_case(n, n_classes, kind, ignore=-1, with_depth=True, with_rgb=True):
    """One accumulate case, run twice: integers equal to the restatement, sums within their bounds, identical bytes both times."""
    t, p = V.label_case(n, n_classes, kind, ignore)
    groups = {"true_label": t, "pred_label": p}
    depth = rgb = None
    if with_depth:
        depth = V.depth_case(n)
        groups["depth_trgt"], groups["depth_pred"] = depth
    if with_rgb:
        rgb = V.rgb_case(n)
        groups["rgb_pred"], groups["rgb_trgt"] = rgb
    want_counts, want_sums, want_log, d_log = V.reference_counts(n_classes, ignore, t.numpy(), p.numpy(),
                                                                 None if depth is None else (depth[0].numpy(), depth[1].numpy()),
                                                                 None if rgb is None else (rgb[0].numpy(), rgb[1].numpy()))
    counts, sums, _ = _accumulate(n_classes, ignore, **groups)
    counts2, sums2, _ = _accumulate(n_classes, ignore, **groups)
    got = counts.cpu().numpy()
    assert np.array_equal(got, want_counts), (n, n_classes, kind, np.flatnonzero(got != want_counts)[:8])
    bad = V.sums_judgement(sums.cpu().numpy(), n, want_sums, want_log, d_log)
    assert not bad, (n, n_classes, kind, bad)
    assert counts.cpu().numpy().tobytes() == counts2.cpu().numpy().tobytes() and sums.cpu().numpy().tobytes() == sums2.cpu().numpy().tobytes()
    return counts, sums


@pytest.mark.parametrize("n_classes", V.CLASSES)
def test_accumulate_counts_and_sums(n_classes):
    for n in V.N_SIZES:
        _check_case(n, n_classes, "mixed")


@pytest.mark.parametrize("n_classes", (1, 28, 64, 65, 240))
@pytest.mark.parametrize("kind", ("one_pair", "ignored", "out_of_range"))
def test_accumulate_degenerate_label_sets(n_classes, kind):
    counts, _ = _check_case(4099, n_classes, kind, with_depth=False, with_rgb=False)
    table = counts.cpu().numpy()[:n_classes * n_classes].reshape(n_classes, n_classes)
    if kind == "one_pair":
        assert table[n_classes - 1, 0] == 4099 and table.sum() == 4099            # row = true, column = predicted
    else:
        assert table.sum() == 0


def test_accumulate_other_ignore_label():
    _check_case(257, 28, "mixed", ignore=27)
    _check_case(257, 28, "ignored", ignore=255, with_depth=False, with_rgb=False)


def test_accumulate_second_trip_of_a_workgroup():
    """More pixels than the capped grid covers at once; labels from logits, so sem_tile runs in the looping kernel too."""
    from intrinsicnerf_amd import kernels
    n, n_classes = V.SECOND_TRIP_N, 3
    assert kernels.eval_workspace_bytes(n) == kernels.eval_workspace_bytes(n - 65) == 512 * 48 > kernels.eval_workspace_bytes(4099)
    x = V.logit_case(n, n_classes)
    want_label, _, _, _ = V.logit_reference(n, n_classes)
    t, _ = V.label_case(n, n_classes, "mixed")
    depth = V.depth_case(n)
    want_counts, want_sums, want_log, d_log = V.reference_counts(n_classes, -1, t.numpy(), want_label.astype(np.float32),
                                                                 (depth[0].numpy(), depth[1].numpy()))
    counts, sums, (label, entropy) = _accumulate(n_classes, logits=x, true_label=t, depth_trgt=depth[0], depth_pred=depth[1])
    assert np.array_equal(label.cpu().numpy(), want_label.astype(np.float32))
    assert V.entropy_judgement(entropy.cpu().numpy(), n, n_classes)[1] is None
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert not V.sums_judgement(sums.cpu().numpy(), n, want_sums, want_log, d_log)


@pytest.mark.parametrize("n_classes", (2, 28, 65, 240))
def test_accumulate_from_logits_writes_the_maps_of_sem_maps(n_classes):
    """Label from logits in the accumulate launch: the same maps as inerf_sem_maps bit for bit (one copy of the device code), into
    guarded buffers, and the table of those labels."""
    from intrinsicnerf_amd import kernels
    n = 4099
    x = V.logit_case(n, n_classes).to(_dev())
    want_label, _, _, _ = V.logit_reference(n, n_classes)
    t, _ = V.label_case(n, n_classes, "mixed")
    lbuf, label = _guarded(n)
    ebuf, entropy = _guarded(n)
    counts, sums = kernels.eval_tables(n_classes, _dev())
    kernels.eval_accumulate(counts, sums, n_classes, -1, logits=x, true_label=t.to(_dev()), out_label=label, out_entropy=entropy)
    alone = kernels.sem_maps(x)
    assert _guards_intact(lbuf, n) and _guards_intact(ebuf, n)
    assert torch.equal(label, alone[0]) and label.cpu().numpy().tobytes() == alone[0].cpu().numpy().tobytes()
    assert entropy.cpu().numpy().tobytes() == alone[1].cpu().numpy().tobytes()
    want_counts, _, _, _ = V.reference_counts(n_classes, -1, t.numpy(), want_label.astype(np.float32))
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    # the maps without any target group: nothing accumulates
    counts.zero_()
    l2, e2 = kernels.eval_accumulate(counts, sums, n_classes, -1, logits=x)
    assert torch.equal(l2, alone[0]) and int(counts.abs().sum()) == 0


def test_accumulate_split_calls_and_strided_inputs():
    """4 099 pixels as 1 000 + 3 099 into the same tables: equal integers, sums within the bound; the inputs as columns of one pack."""
    from intrinsicnerf_amd import kernels
    n, n_classes = 4099, 28
    t, p = V.label_case(n, n_classes, "mixed")
    dt, dp = V.depth_case(n)
    x, y = V.rgb_case(n)
    want_counts, want_sums, want_log, d_log = V.reference_counts(n_classes, -1, t.numpy(), p.numpy(), (dt.numpy(), dp.numpy()), (x.numpy(), y.numpy()))
    pack = torch.cat([x, dp[:, None], p[:, None], t[:, None], dt[:, None], y], dim=1).to(_dev())           # [n, 10]
    cols = dict(rgb_pred=pack[:, 0:3], depth_pred=pack[:, 3], pred_label=pack[:, 4], true_label=pack[:, 5], depth_trgt=pack[:, 6], rgb_trgt=pack[:, 7:10])
    counts, sums = kernels.eval_tables(n_classes, _dev())
    kernels.eval_accumulate(counts, sums, n_classes, -1, **{k: v[:1000] for k, v in cols.items()})
    kernels.eval_accumulate(counts, sums, n_classes, -1, **{k: v[1000:] for k, v in cols.items()})
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert not V.sums_judgement(sums.cpu().numpy(), n, want_sums, want_log, d_log)
    whole = kernels.eval_tables(n_classes, _dev())
    kernels.eval_accumulate(*whole, n_classes, -1, **cols)
    assert torch.equal(whole[0], counts)


def test_calculate_functions_equal_finish_of_the_tables_and_the_restatement():
    from intrinsicnerf_amd import evaluation
    n, n_classes = 4099, 28
    t, p = V.label_case(n, n_classes, "mixed")
    dt, dp = V.depth_case(n)
    x, y = V.rgb_case(n)
    counts, sums, _ = _accumulate(n_classes, true_label=t, pred_label=p, depth_trgt=dt, depth_pred=dp, rgb_pred=x, rgb_trgt=y)
    table, scalars = evaluation.split_table(counts.cpu().numpy(), n_classes)
    seg = evaluation.calculate_segmentation_metrics(t.numpy().reshape(1, -1), p.to(_dev()), n_classes, -1)          # host numpy and device torch
    assert V.same_metrics(seg, evaluation.finish_segmentation(table, scalars[0]))
    want_counts, _, _, _ = V.reference_counts(n_classes, -1, t.numpy(), p.numpy())
    assert V.same_metrics(seg, V.segmentation_from_table(want_counts[:-8].reshape(n_classes, n_classes), want_counts[-8]))
    depth = evaluation.calculate_depth_metrics(depth_trgt=dt.double().numpy(), depth_pred=dp)
    assert V.same_metrics(depth, evaluation.finish_depth(scalars, sums.cpu().numpy()))
    assert V.same_metrics(evaluation.image_mse_psnr(x, y.numpy()), evaluation.finish_image(scalars, sums.cpu().numpy()))
    # integer label arrays of any dtype, and the reference's quirk when everything is ignored
    ti, pi = torch.randint(-1, 5, (300,)), torch.randint(0, 5, (300,))
    seg = evaluation.calculate_segmentation_metrics(ti.numpy().astype(np.int16), pi.numpy().astype(np.uint8), 5, -1)
    valid = ti.numpy() != -1
    assert V.same_metrics(seg, V.segmentation_from_table(V.confusion(ti.numpy()[valid], pi.numpy()[valid], 5), int(valid.sum())))
    assert evaluation.calculate_segmentation_metrics(np.full(10, -1), np.zeros(10), 5, -1) == [0, 0, 0, 0]
    empty = evaluation.calculate_depth_metrics(np.zeros(5, dtype=np.float32), np.ones(5, dtype=np.float32))
    assert np.isnan(empty["AbsRel"]) and empty["complete"] == 1.0


def test_frame_evaluator():
    """Three 65-pixel frames with resident targets = one call on the concatenation; an unregistered ray set gives maps and no
    accumulation; two named semantic targets give two tables."""
    from intrinsicnerf_amd import evaluation, kernels
    frames, pix, n_classes = 3, 65, 28
    n = frames * pix
    x = V.logit_case(n, n_classes).to(_dev())
    want_label, _, _, _ = V.logit_reference(n, n_classes)
    t, _ = V.label_case(n, n_classes, "mixed")
    t2 = torch.roll(t, 7)
    dt, dp = V.depth_case(n)
    rp, rt = V.rgb_case(n)
    rays = torch.zeros(frames, pix, 11, device=_dev())
    ev = evaluation.FrameEvaluator(n_classes)
    ev.register(rays, image=rt.numpy().reshape(frames, pix, 3), depth=dt.numpy().reshape(frames, pix),
                semantic={"clean": t.numpy().reshape(frames, pix), "gt": t2.reshape(frames, pix)})
    assert ev.begin(rays)
    labels = []
    for i in range(frames):
        sl = slice(i * pix, (i + 1) * pix)
        label, entropy = ev.add_frame(i, logits=x[sl], depth=dp[sl].to(_dev()), rgb=rp[sl].to(_dev()))
        assert label.shape == entropy.shape == (pix,) and label.dtype == torch.float32
        labels.append(label)
    assert np.array_equal(torch.cat(labels).cpu().numpy(), want_label.astype(np.float32))
    tables = ev.tables()
    assert set(tables) == {"clean", "gt"}
    whole_counts, whole_sums, _ = _accumulate(n_classes, logits=x, true_label=t, depth_trgt=dt, depth_pred=dp, rgb_pred=rp, rgb_trgt=rt)
    assert torch.equal(tables["clean"][0], whole_counts)
    want_counts, want_sums, want_log, d_log = V.reference_counts(n_classes, -1, t.numpy(), want_label.astype(np.float32),
                                                                 (dt.numpy(), dp.numpy()), (rp.numpy(), rt.numpy()))
    assert np.array_equal(whole_counts.cpu().numpy(), want_counts)
    assert not V.sums_judgement(tables["clean"][1].cpu().numpy(), n, want_sums, want_log, d_log)
    want2, _, _, _ = V.reference_counts(n_classes, -1, t2.numpy(), want_label.astype(np.float32))
    assert np.array_equal(tables["gt"][0].cpu().numpy(), want2)
    res = ev.results()
    assert set(res["segmentation"]) == {"clean", "gt"} and list(res["depth"]) == list(evaluation.DEPTH_KEYS) and len(res["image"]) == 2
    table, scalars = evaluation.split_table(want_counts, n_classes)
    assert V.same_metrics(res["segmentation"]["clean"], V.segmentation_from_table(table, scalars[0]))
    assert V.same_metrics(res["depth"], evaluation.finish_depth(scalars, tables["clean"][1].cpu().numpy()))
    # a ray set nobody registered: maps, no accumulation
    before = {k: (c.clone(), s.clone()) for k, (c, s) in tables.items()}
    other = torch.zeros(frames, pix, 11, device=_dev())
    assert not ev.begin(other)
    label, entropy = ev.add_frame(0, logits=x[:pix], depth=dp[:pix].to(_dev()), rgb=rp[:pix].to(_dev()))
    assert torch.equal(label, labels[0])
    for k, (c, s) in ev.tables().items():
        assert torch.equal(c, before[k][0]) and torch.equal(s, before[k][1])
    ev.reset()
    assert all(int(c.abs().sum()) == 0 and float(s.abs().sum()) == 0.0 for c, s in ev.tables().values())
    assert ev.results() == {"segmentation": {}, "depth": None, "image": None}


def test_render_path_with_a_frame_evaluator():
    """The smallest SSR render (two frames, default-init networks, C = 3): with ``frame_evaluator`` set the labels equal the run
    without it, the entropy is within the bound of a float64 evaluation of the logits, every other array is bit-identical, and
    the registered frame set's table is the one of the returned labels."""
    from intrinsicnerf_amd import evaluation, ssr
    from oracle import calibration as cal
    dev = _dev()
    H, W, C = 12, 16, 3
    r = ssr.SSRRenderer(C, white_bkgd=False, chunk=100, device=dev)
    r.H_scaled, r.W_scaled, r.near, r.far = H, W, 0.1, 10.0
    r.check_numerics = False
    T = torch.eye(4)[None].repeat(2, 1, 1)
    T[1, :3, 3] = torch.tensor([0.2, 0.0, 0.1])
    rays = ssr.create_rays(2, T.to(dev), H, W, 8.0, 8.0, (W - 1) / 2.0, (H - 1) / 2.0, 0.1, 10.0)
    r.ssr_net_coarse.load_state_dict(cal.calibrated_default_init("ssr", C, 0, rays[0].cpu()))
    r.ssr_net_fine.load_state_dict(cal.calibrated_default_init("ssr", C, 1, rays[0].cpu()))
    assert ssr.SSRRenderMixin.frame_evaluator is None
    g = torch.Generator().manual_seed(9)
    true = torch.randint(-1, C, (2, H * W), generator=g)
    gt_depth = torch.rand(2, H * W, generator=g) * 4 + 0.5
    with torch.no_grad():
        base = r.render_path(rays)
        logits = [r.render_rays(rays[i])["sem_logits_fine"].double().cpu() for i in range(2)]
        r.frame_evaluator = ev = evaluation.FrameEvaluator(C)
        ev.register(rays, depth=gt_depth, semantic=true)
        out = r.render_path(rays)
    assert len(out) == 12
    for k, (a, b) in enumerate(zip(base, out)):
        if k == 6 or a is None:
            assert k == 6 or b is None
            continue
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    F = torch.nn.functional
    for i in range(2):
        h64 = torch.sum(-F.log_softmax(logits[i], -1) * F.softmax(logits[i], -1), -1).numpy()
        x32 = logits[i].float()
        h32 = torch.sum(-F.log_softmax(x32, -1) * F.softmax(x32, -1), -1).numpy()
        d = float(np.abs(h32 - h64).max())
        got = out[6][i].reshape(-1).astype(np.float64)
        assert out[6].dtype == base[6].dtype == np.float32
        assert (np.abs(got - h64) <= 4 * d + V.EPS21 * np.maximum(1.0, np.abs(h64))).all()
    counts = ev.tables()[None][0].cpu().numpy()
    want, _, _, _ = V.reference_counts(C, -1, true.numpy().reshape(-1).astype(np.float32), out[4].reshape(-1).astype(np.float32),
                                       (gt_depth.numpy().reshape(-1), out[2].reshape(-1)))
    assert np.array_equal(counts, want)
    assert ev.results()["depth"]["complete"] == want[-8 + 2] / want[-8 + 1]


def test_both_calls_replay_from_a_graph():
    """Capturable: no allocation, synchronisation or host read inside the calls.  A captured sem_maps + accumulate pair, replayed
    twice onto zeroed tables, leaves twice the directly launched counts and the same maps."""
    from intrinsicnerf_amd import kernels
    n, n_classes = 4099, 28
    x = V.logit_case(n, n_classes).to(_dev())
    t = V.label_case(n, n_classes, "mixed")[0].to(_dev())
    dt, dp = (v.to(_dev()) for v in V.depth_case(n))
    direct = kernels.eval_tables(n_classes, _dev())
    want_label, want_entropy = kernels.eval_accumulate(*direct, n_classes, -1, logits=x, true_label=t, depth_pred=dp, depth_trgt=dt)
    counts, sums = kernels.eval_tables(n_classes, _dev())
    label, entropy = torch.empty(n, device=_dev()), torch.empty(n, device=_dev())
    alone = torch.empty(n, device=_dev())
    ws = torch.empty(kernels.eval_workspace_bytes(n) // 8, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.sem_maps(x, label=alone, want_entropy=False)
        kernels.eval_accumulate(counts, sums, n_classes, -1, logits=x, true_label=t, depth_pred=dp, depth_trgt=dt, out_label=label,
                                out_entropy=entropy, workspace=ws)
    counts.zero_(); sums.zero_()
    graph.replay(); graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(counts, 2 * direct[0])
    assert torch.equal(label, want_label) and torch.equal(alone, want_label)
    assert entropy.cpu().numpy().tobytes() == want_entropy.cpu().numpy().tobytes()
    assert float((sums - 2 * direct[1]).abs().max()) <= 2 * n * 2.0 ** -52 * float(direct[1].abs().max())
