"""GPU: training-batch assembly (csrc/batch.hip: ``inerf_batch_assemble``, ``batches.ObjectBatcher`` / ``SSRBatcher``,
``ssr.SSRRenderMixin.sample_data``).  Everything here is a gather, an integer draw or the ray generator's fixed operation order, so
every comparison is bit-exact (``torch.equal``):

* form (a) - indices supplied in the reference's draw order - against tests/golden/train_batch.npz, which the reference's own
  statements produced (tests/golden/make_golden_batches.py);
* rays computed in the kernel against ``kernels.gen_rays`` gathered at the same pixels;
* form (b) - indices drawn in the kernel - against the NumPy restatement tests/_batch_draw.py;
* the device step counter: replays of a captured ``next()`` against eager calls.
Never reads the reference tree."""
import numpy as np
import pytest
import torch

import _batch_draw as bd
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return load_golden("train_batch")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def same(got, want, what):
    want = want if isinstance(want, torch.Tensor) else torch.from_numpy(np.asarray(want))
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {got.numel()} elements differ"


def object_batcher(gold, n=9, **kw):
    from intrinsicnerf_amd import batches
    return batches.ObjectBatcher(gold["obj_images"], gold["obj_masks"], gold["obj_poses"], gold["obj_K"], [0, 1, 2], n, device=DEV, **kw)


# ---- form (a) against the reference ----
@pytest.mark.parametrize("tag", ["full_mask", "crop_mask", "full_plain"])
def test_object_batch_equals_the_reference(gold, tag):
    from intrinsicnerf_amd import batches
    masked = tag.endswith("mask")
    b = batches.ObjectBatcher(gold["obj_images"], gold["obj_masks"] if masked else None, gold["obj_poses"], gold["obj_K"], [0, 1, 2], 9,
                              precrop_iters=1, precrop_frac=0.7, device=DEV)
    i = 0 if tag.startswith("crop") else 5
    assert b.window(i) == tuple(int(v) for v in gold[f"obj_{tag}_window"])
    indices = (int(gold[f"obj_{tag}_image"]), gold[f"obj_{tag}_pixels"], gold[f"obj_{tag}_off_row"], gold[f"obj_{tag}_off_col"])
    rays, target_s, target_m = b.next(i, indices=indices)
    same(rays, gold[f"obj_{tag}_batch_rays"], "batch_rays")
    same(target_s, gold[f"obj_{tag}_target_s"], "target_s")
    if masked:
        same(target_m, gold[f"obj_{tag}_target_m"], "target_m")
    else:
        assert target_m is None
    # the image index as a device tensor, the others as device tensors: the same batch
    again = b.next(i, indices=(dev(np.array([indices[0]])), dev(indices[1]), dev(indices[2]), dev(indices[3])))
    assert all(torch.equal(x, y) for x, y in zip((rays, target_s), again[:2]))
    b.check()


SSR_CASES = [("train_sem_unavailable", "train", True), ("train_sem_available", "train", True), ("train_plain", "train", False),
             ("test_sem", "test", True)]


@pytest.mark.parametrize("tag,mode,enable_semantic", SSR_CASES)
def test_ssr_batch_equals_the_reference(gold, tag, mode, enable_semantic):
    from intrinsicnerf_amd import batches
    b = batches.SSRBatcher(gold[f"ssr_{mode}_image"], gold[f"ssr_{mode}_depth"], gold[f"ssr_{mode}_semantic"], 9, rays=gold[f"ssr_{mode}_rays"],
                           mask_ids=gold["ssr_mask_ids"][:gold[f"ssr_{mode}_image"].shape[0]], enable_semantic=enable_semantic, device=DEV)
    out = b.next(0, indices=(int(gold[f"ssr_{tag}_image"]), gold["ssr_pixels"], gold["ssr_off_row"], gold["ssr_off_col"]))
    names = ("rays", "rgb", "depth", "semantic", "flag") if enable_semantic else ("rays", "rgb")
    assert len(out) == len(names)
    for name, got in zip(names, out):
        same(got, gold[f"ssr_{tag}_{name}"], f"{tag}.{name}")
    b.check()


class StandInTrainer:
    """What ``sample_data`` reads of an SSRTrainer (trainer.py:627-691), over the fixture's tables; the draws are the recorded ones
    in the shape ``sampling_index`` returns them (rays.py:153-172: the pixels, then their clamped neighbours)."""

    def __init__(self, gold, enable_semantic, image_index):
        for mode in ("train", "test"):
            for k in ("image", "depth", "semantic"):
                setattr(self, f"{mode}_{k}", dev(gold[f"ssr_{mode}_{k}"]))
        self.num_train, self.num_test = gold["ssr_train_image"].shape[0], gold["ssr_test_image"].shape[0]
        self.enable_semantic, self.n_rays, self.mask_ids = enable_semantic, 9, gold["ssr_mask_ids"]
        h, w = int(gold["H"]), int(gold["W"])
        pix = torch.from_numpy(gold["ssr_pixels"])[None]
        nh = torch.clamp(pix // w + torch.from_numpy(gold["ssr_off_row"]), 0, h - 1)
        nw = torch.clamp(pix % w + torch.from_numpy(gold["ssr_off_col"]), 0, w - 1)
        drawn = (np.array(image_index).reshape((1, 1)), torch.cat((pix, nh * w + nw), 1))
        self.sampling_index = lambda n_rays, batch_size, hh, ww: drawn


@pytest.mark.parametrize("tag,mode,enable_semantic", SSR_CASES)
def test_sample_data_mirror_equals_the_reference(gold, tag, mode, enable_semantic):
    from intrinsicnerf_amd import ssr
    t = StandInTrainer(gold, enable_semantic, int(gold[f"ssr_{tag}_image"]))
    out = ssr.SSRRenderMixin.sample_data(t, 0, dev(gold[f"ssr_{mode}_rays"]), int(gold["H"]), int(gold["W"]), no_batching=True, mode=mode)
    names = ("rays", "rgb", "depth", "semantic", "flag") if enable_semantic else ("rays", "rgb")
    assert len(out) == len(names)
    for name, got in zip(names, out):
        if name == "flag":                                    # mask_ids[index_batch]: a host array, as the reference returns it
            assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, gold[f"ssr_{tag}_flag"])
        else:
            same(got, gold[f"ssr_{tag}_{name}"], f"{tag}.{name}")
    with pytest.raises(AssertionError):
        ssr.SSRRenderMixin.sample_data(t, 0, dev(gold[f"ssr_{mode}_rays"]), int(gold["H"]), int(gold["W"]), mode="vis")


# ---- rays computed in the kernel ----
H2, W2 = 33, 17


@pytest.fixture(scope="module")
def camera():
    g = torch.Generator().manual_seed(5)
    poses = torch.eye(4)[None].repeat(2, 1, 1)
    for k in range(2):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
        poses[k, :3, :3], poses[k, :3, 3] = q, torch.randn(3, generator=g)
    return dict(poses=poses.to(DEV), fx=21.3, fy=20.9, cx=0.5 * W2 + 0.25, cy=0.5 * H2, near=0.1, far=10.0)


@pytest.mark.parametrize("opengl", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_rays_from_poses_equal_gen_rays_gathered(camera, n, opengl):
    from intrinsicnerf_amd import kernels
    c = camera
    table = kernels.gen_rays(c["poses"], H2, W2, c["fx"], c["fy"], c["cx"], c["cy"], c["near"], c["far"], opengl).reshape(2, H2 * W2, 11)
    g = torch.Generator().manual_seed(n)
    pix = torch.randint(0, H2 * W2, (n,), generator=g)
    orow, ocol = torch.randint(-1, 2, (n,), generator=g), torch.randint(-1, 2, (n,), generator=g)
    nei = torch.clamp(pix // W2 + orow, 0, H2 - 1) * W2 + torch.clamp(pix % W2 + ocol, 0, W2 - 1)
    rows = torch.cat([pix, nei]).to(DEV)
    image = torch.rand(2, H2, W2, 3, generator=g).to(DEV)
    idx = (1, pix.to(DEV), orow.to(DEV), ocol.to(DEV))
    cam = dict(c, opengl=opengl)
    from_pose = kernels.batch_ssr(image, None, None, n, camera=cam, indices=idx)
    from_table = kernels.batch_ssr(image, None, None, n, rays=table, indices=idx)
    assert torch.equal(from_pose[0], table[1][rows]) and torch.equal(from_table[0], table[1][rows])      # both paths, the same rows
    assert torch.equal(from_pose[1], image[1].reshape(-1, 3)[rows]) and from_pose[2] is None and from_pose[3] is None
    if opengl:                                                 # the object-level form: origins and directions of the same rows
        rays, target_s, target_m = kernels.batch_object(image, None, c["poses"][:, :3].contiguous(), (c["fx"], c["fy"], c["cx"], c["cy"]),
                                                        (0, 0, H2, W2), n, indices=idx)
        assert torch.equal(rays[0], table[1][rows][:, 0:3]) and torch.equal(rays[1], table[1][rows][:, 3:6])
        assert torch.equal(target_s, image[1].reshape(-1, 3)[rows]) and target_m is None


# ---- form (b) against the NumPy restatement ----
def drawn_object(images, masks, poses, window, n, seed, step, ids=None):
    from intrinsicnerf_amd import kernels
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    draw = dict(seed=seed, step=step, image_ids=None if ids is None else dev(np.asarray(ids, dtype=np.int64)))
    out = kernels.batch_object(images, masks, poses, (9.5, 9.25, 3.3, 2.9), window, n, draw=draw, status=status, return_indices=True)
    return out, int(status.item())


# (H, W, row0, col0, rows, cols): M = 1, 2, 3, 257, 40 000, and the centre crop of a 14 x 22 frame (dH = 3, dW = 5: both odd)
FRAMES = [(3, 4, 0, 0, 1, 1), (6, 8, 3, 4, 1, 2), (7, 5, 2, 1, 3, 1), (259, 3, 0, 0, 257, 1), (203, 204, 1, 2, 200, 200), (14, 22, 4, 6, 6, 10)]


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"M{f[4] * f[5]}")
def test_drawn_object_batch_equals_the_restated_draw(frame):
    from intrinsicnerf_amd import batches, kernels
    h, w, row0, col0, wh, ww = frame
    window, m = frame[2:], wh * ww
    if (h, w) == (14, 22):
        crop = batches.ObjectBatcher.__new__(batches.ObjectBatcher)
        crop.H, crop.W, crop.precrop_iters, crop.precrop_frac = h, w, 1, 0.5
        assert crop.window(0) == window
    g = torch.Generator().manual_seed(m)
    images, masks = torch.rand(3, h, w, 3, generator=g).to(DEV), torch.rand(3, h, w, 1, generator=g).to(DEV)
    poses = torch.randn(3, 3, 4, generator=g).to(DEV)
    ids = [2, 0]
    for seed, step, n in ((7, 0, m), (7, 1, min(m, 300)), (2 ** 40 + 5, -3, max(1, m // 2)), (9, 2 ** 33 + 1, 1)):
        (rays, target_s, target_m, idx), status = drawn_object(images, masks, poses, window, n, seed, step, ids)
        assert status == 0
        img, pix, orow, ocol = bd.object_draw(seed, step, n, m, image_ids=np.array(ids))
        assert int(idx["image"].item()) == img
        same(idx["pixels"], pix, "pixels"), same(idx["off_row"], orow, "off_row"), same(idx["off_col"], ocol, "off_col")
        assert len(set(pix.tolist())) == n                                 # distinct within a step
        if n == m:
            assert torch.equal(torch.sort(idx["pixels"]).values.cpu(), torch.arange(m))
        # the rows are those of form (a) with the same indices
        want = kernels.batch_object(images, masks, poses, (9.5, 9.25, 3.3, 2.9), window, n, indices=(img, dev(pix), dev(orow), dev(ocol)))
        assert torch.equal(rays, want[0]) and torch.equal(target_s, want[1]) and torch.equal(target_m, want[2])
        # ... and the gathers are the plain ones: neighbours clamp to the image, not to the window
        r, c = row0 + pix // ww, col0 + pix % ww
        nr, nc = np.clip(r + orow, 0, h - 1), np.clip(c + ocol, 0, w - 1)
        rows_r, rows_c = dev(np.concatenate([r, nr])), dev(np.concatenate([c, nc]))
        assert torch.equal(target_s, images[img][rows_r, rows_c]) and torch.equal(target_m, masks[img][rows_r, rows_c])
        if m >= 60 and n == m:
            outside = (nr < row0) | (nr >= row0 + wh) | (nc < col0) | (nc >= col0 + ww)
            assert outside.any()                                           # some neighbour left the window and was kept
    with pytest.raises(RuntimeError, match="invalid argument"):            # more distinct pixels than the window holds
        drawn_object(images, masks, poses, window, m + 1, 7, 0)


def test_drawn_ssr_batch_equals_the_restated_draw(gold):
    from intrinsicnerf_amd import kernels
    image, depth, semantic = dev(gold["ssr_train_image"]), dev(gold["ssr_train_depth"]), dev(gold["ssr_train_semantic"])
    rays, avail = dev(gold["ssr_train_rays"]), dev(gold["ssr_mask_ids"])
    h, w = int(gold["H"]), int(gold["W"])
    seen = set()
    for seed, step, n in ((1, 0, 300), (1, 1, 9), (5, 2, 1)):              # n > H * W: with replacement
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = kernels.batch_ssr(image, depth, semantic, n, rays=rays, avail=avail, draw=dict(seed=seed, step=step), status=status,
                                return_indices=True)
        img, pix, orow, ocol = bd.ssr_draw(seed, step, n, h * w, n_images=3)
        idx = out[5]
        assert int(status.item()) == 0 and int(idx["image"].item()) == img
        same(idx["pixels"], pix, "pixels"), same(idx["off_row"], orow, "off_row"), same(idx["off_col"], ocol, "off_col")
        want = kernels.batch_ssr(image, depth, semantic, n, rays=rays, avail=avail, indices=(img, dev(pix), dev(orow), dev(ocol)))
        for got, ref in zip(out[:5], want):
            assert got.dtype == ref.dtype and torch.equal(got, ref)
        assert float(out[4].item()) == float(gold["ssr_mask_ids"][img])
        nei = np.clip(pix // w + orow, 0, h - 1) * w + np.clip(pix % w + ocol, 0, w - 1)
        rows = dev(np.concatenate([pix, nei]))
        assert torch.equal(out[0], rays[img][rows]) and torch.equal(out[3], semantic[img].reshape(-1)[rows].long())
        assert torch.equal(out[1], image[img].reshape(-1, 3)[rows]) and torch.equal(out[2], depth[img].reshape(-1)[rows])
        seen.add(img)
    # labels of every integer width the kernel reads, and fp32 tables
    for dt in (torch.int16, torch.int32, torch.int64):
        out = kernels.batch_ssr(image.float(), depth.float(), semantic.to(dt), 9, rays=rays, draw=dict(seed=1, step=1))
        assert out[1].dtype == torch.float32 and out[2].dtype == torch.float32 and torch.equal(out[3], want_labels(gold, 1, 1, semantic))


def want_labels(gold, seed, step, semantic):
    h, w = int(gold["H"]), int(gold["W"])
    img, pix, orow, ocol = bd.ssr_draw(seed, step, 9, h * w, n_images=3)
    nei = np.clip(pix // w + orow, 0, h - 1) * w + np.clip(pix % w + ocol, 0, w - 1)
    return semantic[img].reshape(-1)[dev(np.concatenate([pix, nei]))].long()


def test_an_index_outside_its_table_is_clamped_and_reported(gold):
    b = object_batcher(gold)
    pixels = gold["obj_full_mask_pixels"].copy()
    pixels[3] = 42                                                          # one past the 6 x 7 frame
    rays, target_s, target_m = b.next(5, indices=(1, pixels, gold["obj_full_mask_off_row"], gold["obj_full_mask_off_col"]))
    assert bool(torch.isfinite(rays).all())
    with pytest.raises(IndexError):
        b.check()


# ---- the device step counter ----
def test_replays_of_a_captured_next_equal_eager_calls(gold):
    eager, graphed = object_batcher(gold, seed=21), object_batcher(gold, seed=21)
    want = [eager.next() for _ in range(3)]
    by_step = [object_batcher(gold, seed=21).next(i) for i in range(3)]     # next(i) draws step i: the same three batches
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = graphed.next()
    got = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got.append([t.clone() for t in out])
    assert int(graphed.step.item()) == 3 == int(eager.step.item())
    for k in range(3):
        for a, b, c in zip(got[k], want[k], by_step[k]):
            assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(got[0][1], got[1][1]) and not torch.equal(got[1][1], got[2][1]) and not torch.equal(got[0][1], got[2][1])
    eager.check(), graphed.check()


def test_ssr_batcher_counter_and_images(gold):
    from intrinsicnerf_amd import batches
    mk = lambda: batches.SSRBatcher(gold["ssr_train_image"], gold["ssr_train_depth"], gold["ssr_train_semantic"], 9, rays=gold["ssr_train_rays"],
                                    mask_ids=gold["ssr_mask_ids"], seed=4, device=DEV)
    a, b = mk(), mk()
    flags = set()
    for i in range(12):
        x, y = a.next(), b.next(i)
        assert len(x) == 5 and all(torch.equal(p, q) for p, q in zip(x, y))
        assert x[4].shape == (1, 1) and x[4].dtype == torch.float64
        flags.add(float(x[4].item()))
    assert flags == {0.0, 1.0} and int(a.step.item()) == 12 and int(b.step.item()) == 0


def test_empty_batch_has_the_right_shapes(gold):
    from intrinsicnerf_amd import kernels
    b = object_batcher(gold, n=0)
    rays, target_s, target_m = b.next()
    assert rays.shape == (2, 0, 3) and target_s.shape == (0, 3) and target_m.shape == (0, 1) and int(b.step.item()) == 0
    out = kernels.batch_ssr(dev(gold["ssr_train_image"]), dev(gold["ssr_train_depth"]), dev(gold["ssr_train_semantic"]), 0,
                            rays=dev(gold["ssr_train_rays"]), draw=dict(seed=1, step=0))
    assert out[0].shape == (0, 11) and out[1].shape == (0, 3) and out[2].shape == (0,) and out[3].shape == (0,)
    assert out[1].dtype == torch.float64 and out[3].dtype == torch.int64
