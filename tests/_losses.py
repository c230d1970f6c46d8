"""Shared by the loss tests: the fixtures of tests/golden/loss_*.npz and a float64 restatement of what csrc/losses.hip computes.

The restatement is written from the kernels' specification (include/inerf.h), not from the reference's text: explicit pair
indices, the factorised form of the [N,1]-mask broadcast, and every term of a level in one vector.  tests/test_losses_cpu.py
holds it against the fixtures (and against the live reference where it is mounted); it is what tells a wrong fixture from a
wrong kernel."""
import os

import numpy as np
import torch

from conftest import load_golden

TERMS = ("chroma", "residual", "sparsity", "shading", "far", "intensity", "image", "cluster", "semantic")
SIX = (0, 1, 2, 3, 4, 5)
DIFF = ("albedo", "shading", "residual", "rgb", "logits")
RTOL = 1e-4             # the project's plain bound (tests/test_backward_golden.py): 1e-4 relative on each term ...
GRAD_SCALE = 1e-5       # ... and RTOL * |want| + 1e-5 of the tensor's largest entry on each gradient tensor


def cases(kind):
    """{case: {name: array}} of tests/golden/loss_<kind>.npz."""
    out = {}
    for k, v in load_golden("loss_" + kind).items():
        case, name = k.split("/", 1)
        out.setdefault(case, {})[name] = v
    return out


def case_names(kind):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"loss_{kind}.npz")
    if not os.path.exists(path):
        return []
    with np.load(path) as z:
        return sorted({k.split("/", 1)[0] for k in z.files})


def tensors(case, device="cpu", dtype=torch.float32):
    """The case's inputs as torch tensors: shared ones by name, per-level ones as a list of dicts (leaves that require grad)."""
    key = torch.from_numpy(case["key"])
    key = key.to(torch.int64) if not key.dtype.is_floating_point else key.to(dtype)
    shared = {"gt": torch.from_numpy(case["gt"]).to(dtype).to(device), "key": key.to(device),
              "target": torch.from_numpy(case["target"]).to(dtype).to(device) if "target" in case else None}
    levels = []
    for l in range(int(case["levels"])):
        levels.append({k: torch.from_numpy(case[f"{k}{l}"]).to(dtype).to(device).requires_grad_(True) for k in DIFF if f"{k}{l}" in case})
    return shared, levels


def _chroma(c):
    s = c.sum(-1) + 1e-5
    return c[:, 0] / s, c[:, 1] / s


def level_terms(albedo, shading, residual, gt, key, rgb=None, target=None, logits=None):
    """The nine terms of one level (absent ones 0) as a vector, in the dtype of the inputs."""
    n = gt.shape[0]
    zero = gt.new_zeros(())
    ar, ag = _chroma(albedo)
    gr, gg = _chroma(gt)
    chroma = ((ar - gr) ** 2).mean() + ((ag - gg) ** 2).mean()
    res = (residual ** 2).mean()
    labels = not key.dtype.is_floating_point
    outer = key.dim() == 2
    flat = key.reshape(n)

    def pairs(count, offset):
        i = torch.arange(count, device=gt.device)
        j = i + offset
        d2 = (gr[i] - gr[j]) ** 2 + (gg[i] - gg[j]) ** 2
        m = (flat[i] == flat[j]).to(gt.dtype) if labels else flat[i] * flat[j]
        dist = ((albedo[i] - albedo[j]) ** 2).sum(-1)
        ds = (shading[i] - shading[j]) ** 2
        e = torch.exp(-60 * d2)
        if outer:                       # the [split, split] broadcast: mean over i of the mask product times mean over j of the rest
            return m.mean() * (e * dist).mean(), m.mean() * (d2 * ds).mean()
        return (e * m * dist).mean(), (d2 * ds if labels else d2 * m * ds).mean()

    split = n // 2
    split2 = split // 2
    sparsity, smooth = pairs(split, n - split)
    far, _ = pairs(split2, split - split2)
    intensity = (gt.mean() - albedo.mean()) ** 2
    image = ((rgb - gt) ** 2).mean() if rgb is not None else zero
    cluster = ((albedo - target) ** 2).mean() if target is not None else zero
    sem = zero
    if logits is not None:
        lab = flat - 1
        keep = lab >= 0
        logp = torch.log_softmax(logits, -1)
        picked = logp[keep].gather(1, lab[keep][:, None])
        sem = -picked.sum() / keep.sum()                 # 0 / 0 = NaN when every ray is void
    return torch.stack([chroma, res, sparsity, smooth, far, intensity, image, cluster, sem])


def present(shared, level):
    return [True] * 7 + [shared["target"] is not None, "logits" in level]


def total_of(terms, weights, shared, levels):
    total = 0
    for t, lv in zip(terms, levels):
        for k, on in enumerate(present(shared, lv)):
            if on:
                total = total + float(weights[k]) * t[k]
    return total


def restate(case, dtype=torch.float64):
    """(terms per level, total, gradients by fixture name) of a fixture case from the restatement."""
    shared, levels = tensors(case, dtype=dtype)
    terms = [level_terms(lv["albedo"], lv["shading"], lv["residual"], shared["gt"], shared["key"], lv["rgb"], shared["target"],
                         lv.get("logits")) for lv in levels]
    total = total_of(terms, case["weights"], shared, levels)
    total.backward()
    grads = {f"g_{k}{l}": v.grad for l, lv in enumerate(levels) for k, v in lv.items()}
    return terms, total.detach(), grads


def assert_terms(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern {got} against {want}"
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    assert (err <= RTOL * np.abs(want[ok])).all(), f"{what}: {got} against {want}"


def assert_gradient(got, want, what):
    got, want = got.detach().double().cpu().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite gradient"
    scale = np.abs(want).max() if want.size else 0.0
    err = np.abs(got - want)
    bound = RTOL * np.abs(want) + GRAD_SCALE * scale
    assert (err <= bound).all(), f"{what}: worst |diff| {err.max():.3e} (scale {scale:.3e}, worst excess {(err - bound).max():.3e})"
