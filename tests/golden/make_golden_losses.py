#!/usr/bin/env python3
"""Golden vectors for the training losses (csrc/losses.hip), from the reference's own functions (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_losses.py

Writes tests/golden/loss_object.npz (compute_intrinsic_loss of object_level/run_nerf_helpers.py:59-86, img2mse :11) and
tests/golden/loss_ssr.npz (SSR/training/training_utils.py:179-207, :124, and nn.CrossEntropyLoss(ignore_index=-1) on label-1,
trainer.py:858-865).  Per case (keys ``<case>/<name>``):

  inputs      gt, key (float mask [N] or [N,1] / int64 labels), target (cluster target, optional) and per level ``l``
              albedo<l>, shading<l>, residual<l>, rgb<l>, logits<l> (SSR)
  weights     the fixed weight of each term, in the order of ``TERMS`` below
  terms<l>    the reference's fp32 terms in that order (absent ones 0)        terms64_<l>  the same from float64 inputs
  total       sum_l sum_t weights[t] * terms<l>[t], as the trainers add it up (fp32)
  g_<name><l> the reference's autograd gradient of ``total`` for every differentiable input (fp32)
  dev_terms<l>, dev_g_<name><l>   the reference's OWN fp32-vs-fp64 deviation: relative per term, and max |g32 - g64| over
              max |g64| per gradient tensor.  (The fp64 gradient tensors themselves are not stored: they would double the file.)

The generator asserts that every deviation of a non-NaN case is below 1e-5 - ten times under the 1e-4 the tests allow - which
is what lets tests/test_losses_gpu.py use the project's plain bound.  In particular |mean(gt) - mean(albedo)| is kept near 0.15:
the intensity term (a squared difference of two means) is the ill-conditioned one.  The second half of gt repeats the first
half (and the second quarter the first) up to a small perturbation, so that exp(-60 d_chroma^2) is not ~0 on every pair.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402

TERMS = ("chroma", "residual", "sparsity", "shading", "far", "intensity", "image", "cluster", "semantic")
WEIGHTS = np.array([1.0, 0.75, 0.8, 0.6, 0.7, 2.0, 1.0, 0.9, 0.5], dtype=np.float32)
DIFF = ("albedo", "shading", "residual", "rgb", "logits")
MAX_DEVIATION = 1e-5


def make_inputs(rng, n, levels, classes=0, mask="vector", target=False, void=0.25, zero_mask=False):
    """One case's tensors (numpy).  classes > 0: the SSR form (labels 0..classes with 0 = void, logits per level)."""
    q = max(1, (n // 2) // 2)
    base = rng.uniform(0.1, 1.0, size=(q, 3))
    gt = np.concatenate([base] * (n // q + 1))[:n] + rng.normal(0, 0.03, size=(n, 3))
    case = {"gt": np.clip(gt, 0.02, 1.0).astype(np.float32)}
    if classes:
        lab = rng.integers(1, classes + 1, size=n)
        lab[n // 2:] = np.where(rng.uniform(size=n - n // 2) < 0.6, lab[:n - n // 2], lab[n // 2:])     # equal and unequal pairs
        lab[rng.uniform(size=n) < void] = 0
        case["key"] = lab.astype(np.int64)
    else:
        m = np.where(rng.uniform(size=n) < 0.7, 1.0, rng.uniform(0, 1, size=n))
        m[rng.uniform(size=n) < 0.15] = 0.0
        if zero_mask:
            m[:] = 0.0
        case["key"] = m.astype(np.float32).reshape((n, 1) if mask == "outer" else (n,))
    if target:
        case["target"] = rng.uniform(0.05, 0.7, size=(n, 3)).astype(np.float32)
    for l in range(levels):
        case[f"albedo{l}"] = rng.uniform(0.05, 0.7, size=(n, 3)).astype(np.float32)
        case[f"shading{l}"] = rng.uniform(0.1, 1.2, size=n).astype(np.float32)
        case[f"residual{l}"] = rng.normal(0, 0.1, size=(n, 3)).astype(np.float32)
        case[f"rgb{l}"] = np.clip(case["gt"] + rng.normal(0, 0.1, size=(n, 3)), 0, 1).astype(np.float32)
        if classes:
            # multiples of 1/16: the softmax is as generic as with any other values and the file compresses
            case[f"logits{l}"] = (np.round(rng.normal(0, 2.0, size=(n, classes)) * 16) / 16).astype(np.float32)
    return case


def evaluate(case, levels, fn, img2mse, dtype):
    """The reference's terms, total and gradients for ``case`` in ``dtype``."""
    f = lambda a: torch.from_numpy(a).to(dtype)
    gt, key = f(case["gt"]), torch.from_numpy(case["key"])
    key = key if key.dtype == torch.int64 else key.to(dtype)
    target = f(case["target"]) if "target" in case else None
    w = [float(x) for x in WEIGHTS]
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1)
    leaves, terms, total = {}, [], 0
    for l in range(levels):
        t = {k: f(case[f"{k}{l}"]).requires_grad_(True) for k in DIFF if f"{k}{l}" in case}
        leaves[l] = t
        disp = acc = torch.zeros(gt.shape[0], dtype=dtype)
        six = fn(t["albedo"], t["shading"], t["residual"], gt, disp, acc, key)
        zero = torch.zeros((), dtype=dtype)
        row = list(six) + [img2mse(t["rgb"], gt), img2mse(t["albedo"], target) if target is not None else zero,
                           ce(t["logits"], key - 1) if "logits" in t else zero]
        present = [True] * 7 + [target is not None, "logits" in t]
        for k in range(len(TERMS)):
            if present[k]:
                total = total + w[k] * row[k]
        terms.append(torch.stack([r.detach() for r in row]))
    total.backward()
    grads = {f"g_{k}{l}": v.grad for l, t in leaves.items() for k, v in t.items()}
    return terms, total.detach(), grads


def relative(a, b):
    a, b = a.double(), b.double()
    d = (a - b).abs()
    return torch.where(b.abs() > 0, d / b.abs(), d)


def record(out, name, case, levels, fn, img2mse):
    t32, tot32, g32 = evaluate(case, levels, fn, img2mse, torch.float32)
    t64, _, g64 = evaluate(case, levels, fn, img2mse, torch.float64)
    for k, v in case.items():
        out[f"{name}/{k}"] = v.astype(np.int16) if v.dtype == np.int64 else v
    out[f"{name}/weights"] = WEIGHTS
    out[f"{name}/levels"] = np.int32(levels)
    out[f"{name}/total"] = tot32.numpy()
    worst = 0.0
    for l in range(levels):
        assert torch.equal(torch.isnan(t32[l]), torch.isnan(t64[l])), name
        dev = relative(t32[l], t64[l])
        out[f"{name}/terms{l}"] = t32[l].numpy()
        out[f"{name}/terms64_{l}"] = t64[l].numpy()
        out[f"{name}/dev_terms{l}"] = dev.numpy()
        worst = max(worst, float(dev[~torch.isnan(dev)].max()))
    for k, g in g32.items():
        assert torch.isfinite(g).all(), (name, k)
        scale = float(g64[k].abs().max())
        dev = float((g.double() - g64[k]).abs().max()) / scale if scale > 0 else float(g.abs().max())
        out[f"{name}/{k}"] = g.numpy()
        out[f"{name}/dev_{k}"] = np.float64(dev)
        worst = max(worst, dev)
    assert worst < MAX_DEVIATION, f"{name}: the reference's own fp32-vs-fp64 deviation is {worst:.2e}"
    print(f"{name:24s} N = {case['gt'].shape[0]:5d}  terms {np.array2string(t32[-1].numpy(), precision=4)}  worst own deviation {worst:.2e}")


def main():
    _, helpers, _, _, _ = mg.import_reference()
    from SSR.training import training_utils as ssr_utils
    rng = np.random.default_rng(20221017)
    obj, ssr = {}, {}
    obj_fn, ssr_fn = helpers.compute_intrinsic_loss, ssr_utils.compute_intrinsic_loss
    for name, kw in (("n2048_mask_target", dict(n=2048, levels=1, target=True)),
                     ("n2048_outer", dict(n=2048, levels=1, mask="outer")),
                     ("n2047_odd", dict(n=2047, levels=1)),
                     ("n3", dict(n=3, levels=1)),
                     ("n2", dict(n=2, levels=1, mask="outer")),
                     ("n512_zero_mask", dict(n=512, levels=1, zero_mask=True)),
                     ("n384_outer_step", dict(n=384, levels=2, mask="outer", target=True)),
                     ("n512_step", dict(n=512, levels=2, target=True))):
        record(obj, name, make_inputs(rng, **kw), kw["levels"], obj_fn, helpers.img2mse)
    for name, kw in (("n1024_c28_target", dict(n=1024, levels=1, classes=28, target=True)),
                     ("n1024_c1", dict(n=1024, levels=1, classes=1)),
                     ("n1024_c101", dict(n=1024, levels=1, classes=101, void=0.4)),
                     ("n1024_c28_all_void", dict(n=1024, levels=1, classes=28, void=2.0)),
                     ("n3_c5", dict(n=3, levels=1, classes=5, void=0.0)),
                     ("n255_c5_step", dict(n=255, levels=2, classes=5, target=True))):
        record(ssr, name, make_inputs(rng, **kw), kw["levels"], ssr_fn, ssr_utils.img2mse)
    for fname, data in (("loss_object.npz", obj), ("loss_ssr.npz", ssr)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
