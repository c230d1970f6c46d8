#!/usr/bin/env python3
"""Golden vectors for training-batch assembly (csrc/batch.hip), from the reference (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_batches.py      ->  tests/golden/train_batch.npz (arrays only)

Object level: the reference's own statements are run - the ``if N_rand is not None:`` block of ``train()`` (run_nerf.py:899-937:
get_rays, the coords meshgrid, select_inds, select_neighbor, the gathers) is taken out of the parsed script and executed as it
stands on a 6 x 7 frame with 3 images, with ``np.random.choice`` answering recorded arrays in the block's draw order (select_inds,
bias_x, bias_y).  The 9 pixels and offsets are chosen by hand: in the whole-frame cases all four corners and all four edges clamp
and each offset value occurs; in the crop case (precrop_frac 0.7: rows 1..4, columns 1..4) neighbours of window-edge pixels leave
the window but not the image.

SSR: the reference's ``SSRTrainer.sample_data`` on a stand-in trainer (6 x 7, 3 train / 2 test images, n = 9) with the draws of
``sampling_index`` (rays.py:153-172: np.random.choice for the image, torch.randint for the pixels, np.random.choice for bias_w
and then bias_h) answered from recorded arrays; both ``enable_semantic`` settings, both modes, a ``mask_ids`` with a 0 and a 1.
Tables in the dtypes the trainer's prepare_data_* leave them in: image and depth fp64 (cv2.imread(...) / 255.0, / 1000.0),
semantic uint8.  Table values are multiples of 1/64 (1/32 for the rays) so that the file compresses well.  The ray table is
random fp32 (create_rays needs >= 332 pixels for its debug print; a gather is a gather).

Recorded: every table, the indices, the offsets and every output.
"""
import ast
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

H, W, N_IMG, N = 6, 7, 3, 9
# (row, col) and (row offset, column offset): corners, edges, interior
PIXELS = [(0, 0), (0, 6), (5, 0), (5, 6), (0, 3), (5, 2), (2, 0), (3, 6), (2, 3)]
OFFSETS = [(-1, -1), (-1, 1), (1, -1), (1, 1), (-1, 0), (1, 0), (0, -1), (1, 1), (0, 0)]
# crop window rows 1..4, columns 1..4 (4 x 4): window indices; edge pixels step out of the window, never out of the image
CROP_PIXELS = [0, 3, 12, 15, 1, 14, 4, 11, 5]
CROP_OFFSETS = [(-1, -1), (-1, 1), (1, -1), (1, 1), (-1, 0), (1, 0), (0, -1), (0, 1), (0, 0)]


class Recorded:
    """Answers calls in order from a list of recorded arrays."""

    def __init__(self, answers):
        self.answers = list(answers)

    def __call__(self, *args, **kwargs):
        return self.answers.pop(0)


def batch_block(run_nerf):
    """The ``if N_rand is not None:`` statement of train()'s one-image branch, compiled from the reference's own source."""
    with open(run_nerf.__file__) as fh:
        tree = ast.parse(fh.read())
    train = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "train")
    found = [n for n in ast.walk(train) if isinstance(n, ast.If) and ast.unparse(n.test) == "N_rand is not None"
             and "get_rays" in ast.unparse(n.body[0])]
    assert len(found) == 1, len(found)
    return compile(ast.fix_missing_locations(ast.Module(body=found, type_ignores=[])), run_nerf.__file__, "exec")


def object_cases(run_nerf, out):
    rng = np.random.RandomState(11)
    images = (rng.randint(0, 64, (N_IMG, H, W, 3)) / 64.0).astype(np.float32)          # (coarse values: the file compresses to a few KB)
    masks = (rng.rand(N_IMG, H, W, 1) > 0.4).astype(np.float32)
    poses = np.stack([mg.pose_spherical(30.0 + 40 * k, -30.0 + 10 * k, 4.0).numpy() for k in range(N_IMG)]).astype(np.float32)
    focal = 7.25
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    out.update(obj_images=images, obj_masks=masks, obj_poses=poses, obj_K=K)
    code = batch_block(run_nerf)
    full = np.array([r * W + c for r, c in PIXELS], dtype=np.int64)
    cases = (("full_mask", 1, "blender_intrinsic", 5, full, OFFSETS),
             ("crop_mask", 2, "blender_intrinsic", 0, np.array(CROP_PIXELS, dtype=np.int64), CROP_OFFSETS),
             ("full_plain", 0, "blender", 5, full, OFFSETS))
    for tag, img_i, dataset_type, i, select, offsets in cases:
        bias_x = np.array([o[0] for o in offsets], dtype=np.int64)        # added to the row (run_nerf.py:923)
        bias_y = np.array([o[1] for o in offsets], dtype=np.int64)        # added to the column
        shim = types.SimpleNamespace(random=types.SimpleNamespace(choice=Recorded([select, bias_x, bias_y])))
        ns = dict(run_nerf.__dict__)
        ns.update(np=shim, H=H, W=W, K=K, N_rand=N, i=i, start=-1, device="cpu", pose=poses[img_i, :3, :4],
                  args=types.SimpleNamespace(precrop_iters=1, precrop_frac=0.7, dataset_type=dataset_type),
                  target=torch.Tensor(images[img_i]), target_mask=torch.Tensor(masks[img_i]))
        exec(code, ns)
        assert not shim.random.choice.answers
        dH, dW = int(H // 2 * 0.7), int(W // 2 * 0.7)
        window = (H // 2 - dH, W // 2 - dW, 2 * dH, 2 * dW) if i < 1 else (0, 0, H, W)
        out.update({f"obj_{tag}_image": np.int64(img_i), f"obj_{tag}_window": np.array(window, dtype=np.int64),
                    f"obj_{tag}_pixels": select, f"obj_{tag}_off_row": bias_x, f"obj_{tag}_off_col": bias_y,
                    f"obj_{tag}_batch_rays": ns["batch_rays"], f"obj_{tag}_target_s": ns["target_s"]})
        if dataset_type == "blender_intrinsic":
            out[f"obj_{tag}_target_m"] = ns["target_m"]
        assert ns["batch_rays"].shape == (2, 2 * N, 3) and ns["target_s"].shape == (2 * N, 3)


def ssr_cases(SSRTrainer, out):
    rng = np.random.RandomState(12)
    n_train, n_test = 3, 2
    tables = {}
    for mode, n in (("train", n_train), ("test", n_test)):
        tables[mode] = dict(image=rng.randint(0, 64, (n, H, W, 3)) / 64.0, depth=rng.randint(1, 320, (n, H, W)) / 64.0,
                            semantic=rng.randint(0, 29, (n, H, W)).astype(np.uint8),
                            rays=(rng.randint(-256, 257, (n, H * W, 11)) / 32.0).astype(np.float32))
        for k, v in tables[mode].items():
            out[f"ssr_{mode}_{k}"] = v
    mask_ids = np.array([1.0, 0.0, 1.0])
    out["ssr_mask_ids"] = mask_ids
    pixels = np.array([[r * W + c for r, c in PIXELS]], dtype=np.int64)
    bias_h = np.array([o[0] for o in OFFSETS], dtype=np.int64)
    bias_w = np.array([o[1] for o in OFFSETS], dtype=np.int64)
    out.update(ssr_pixels=pixels[0], ssr_off_row=bias_h, ssr_off_col=bias_w)
    cases = (("train_sem_unavailable", "train", True, 1), ("train_sem_available", "train", True, 2), ("train_plain", "train", False, 0),
             ("test_sem", "test", True, 1))
    choice, randint = np.random.choice, torch.randint
    try:
        for tag, mode, enable_semantic, img_i in cases:
            t = SSRTrainer.__new__(SSRTrainer)
            t.n_rays, t.enable_semantic, t.mask_ids, t.num_train, t.num_test = N, enable_semantic, mask_ids, n_train, n_test
            for m in ("train", "test"):
                t.__dict__[m + "_image"] = torch.from_numpy(tables[m]["image"])
                t.__dict__[m + "_depth"] = torch.from_numpy(tables[m]["depth"])
                t.__dict__[m + "_semantic"] = torch.from_numpy(tables[m]["semantic"])
            np.random.choice = Recorded([np.array(img_i), bias_w, bias_h])          # rays.py:155, 161, 162
            torch.randint = Recorded([torch.from_numpy(pixels.copy())])              # rays.py:156
            ret = t.sample_data(0, torch.from_numpy(tables[mode]["rays"]), H, W, no_batching=True, mode=mode)
            assert not np.random.choice.answers and not torch.randint.answers
            out[f"ssr_{tag}_image"] = np.int64(img_i)
            names = ("rays", "rgb", "depth", "semantic", "flag") if enable_semantic else ("rays", "rgb")
            assert len(ret) == len(names)
            for name, v in zip(names, ret):
                out[f"ssr_{tag}_{name}"] = v
    finally:
        np.random.choice, torch.randint = choice, randint


def main():
    run_nerf, H_ref, SSRTrainer, ssr_rays, ssr_mu = mg.import_reference()
    out = dict(H=H, W=W, N=N)
    object_cases(run_nerf, out)
    ssr_cases(SSRTrainer, out)
    mg.save("train_batch", **out)
    for k in sorted(out):
        v = out[k]
        v = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        print(f"  {k:34s} {str(v.dtype):8s} {v.shape}")


if __name__ == "__main__":
    main()
