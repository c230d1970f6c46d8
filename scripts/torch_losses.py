"""The trainers' loss terms as plain torch expressions - what a user of the render path runs without csrc/losses.hip, and the
comparison partner of scripts/bench_losses.py and ``scripts/bench_train_step.py --loss intrinsic``.

Same mathematics and the same kind of ops as the reference's compute_intrinsic_loss (object_level/run_nerf_helpers.py:15-86,
SSR/training/training_utils.py:124-207): slices of the two halves and quarters, elementwise chains, one torch.mean per term.
Written a little leaner than the reference (each chroma is computed once, no unused depth weight), so the op count - and the
time - is a lower bound of what the reference's own lines cost."""
import torch


def _chroma(c):
    s = torch.sum(c, dim=-1) + 1e-5
    return c[:, 0] / s, c[:, 1] / s


def intrinsic_terms(albedo, shading, residual, gt, key):
    """(chroma, residual, sparsity, shading, far, intensity); ``key``: float mask [N] / [N,1] or int64 labels [N]."""
    n = albedo.shape[0]
    split = n // 2
    split2 = split // 2
    labels = not key.dtype.is_floating_point
    ar, ag = _chroma(albedo)
    gr, gg = _chroma(gt)
    chroma = torch.mean((ar - gr) ** 2) + torch.mean((ag - gg) ** 2)
    res = torch.mean(residual ** 2)

    def weights(r1, g1, r2, g2, k1, k2):
        d2 = (r1 - r2) ** 2 + (g1 - g2) ** 2
        if labels:
            return torch.exp(-60 * d2) * (k1 == k2).float(), d2
        return torch.exp(-60 * d2) * k1 * k2, d2 * k1 * k2

    w, w2 = weights(gr[:split], gg[:split], gr[-split:], gg[-split:], key[:split], key[-split:])
    sparsity = torch.mean(w * torch.sum((albedo[:split] - albedo[-split:]) ** 2, dim=-1))
    smooth = torch.mean(w2 * (shading[:split] - shading[-split:]) ** 2)
    wf, _ = weights(gr[:split2], gg[:split2], gr[split - split2:split], gg[split - split2:split], key[:split2], key[split - split2:split])
    far = torch.mean(wf * torch.sum((albedo[:split2] - albedo[split - split2:split]) ** 2, dim=-1))
    intensity = (torch.mean(gt) - torch.mean(albedo)) ** 2
    return chroma, res, sparsity, smooth, far, intensity


def step_loss(levels, gt, key, weights, cluster_target=None, semantic=False):
    """sum over the levels of the weighted terms; ``levels``: dicts with albedo, shading, residual, rgb[, logits]."""
    w = lambda name: float(weights.get(name, 1.0))
    total = 0
    for lv in levels:
        six = intrinsic_terms(lv["albedo"], lv["shading"], lv["residual"], gt, key)
        total = total + w("image") * torch.mean((lv["rgb"] - gt) ** 2)
        for name, t in zip(("chroma", "residual", "sparsity", "shading", "far", "intensity"), six):
            total = total + w(name) * t
        if cluster_target is not None:
            total = total + w("cluster") * torch.mean((lv["albedo"] - cluster_target) ** 2)
        if semantic:
            total = total + w("semantic") * torch.nn.functional.cross_entropy(lv["logits"], key - 1, ignore_index=-1)
    return total
