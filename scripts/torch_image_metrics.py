"""The intrinsic-image metrics in eager torch on the GPU, float64: the partner scripts/bench_image_metrics.py measures
``kernels.image_quality`` against, and checks its values with in the same run.  What a user without the kernels would write:
``conv2d`` with the separable 11-tap window for SSIM, ``unfold`` for the LMSE windows, masked sums for the rest."""
import torch
import torch.nn.functional as F


def taps(device):
    i = torch.arange(-5, 6, dtype=torch.float64, device=device)
    w = torch.exp(-0.5 * (i / 1.5) ** 2)
    return w / w.sum()


def _filter(x, w):
    """[N * C, 1, H, W] float64 -> the valid region under the separable window."""
    return F.conv2d(F.conv2d(x, w.view(1, 1, 11, 1)), w.view(1, 1, 1, 11))


def ssim(p, g, valid):
    """p, g: [N, C, H, W] float64; valid: [N, H, W] bool.  [N] float64."""
    n, c, h, w = p.shape
    t = taps(p.device)
    x, y = p.reshape(n * c, 1, h, w), g.reshape(n * c, 1, h, w)
    mx, my = _filter(x, t), _filter(y, t)
    vx, vy, vxy = _filter(x * x, t) - mx * mx, _filter(y * y, t) - my * my, _filter(x * y, t) - mx * my
    m = ((2 * mx * my + 1e-4) * (2 * vxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))
    centre = valid[:, None, 5:h - 5, 5:w - 5]
    m = m.reshape(n, c, h - 10, w - 10)
    return torch.where(centre, m, torch.zeros_like(m)).sum(dim=(1, 2, 3)) / (c * centre.sum(dim=(1, 2, 3)))


def lmse(p, g, valid, k=20, s=10, chunk=20):
    """[N] float64; the windows through ``unfold``, `chunk` images at a time (a 320x240x3 image unfolds to 6.8 MB per operand)."""
    out = []
    for i in range(0, p.shape[0], chunk):
        keep = valid[i:i + chunk, None].to(p.dtype)
        pu = F.unfold(p[i:i + chunk] * keep, k, stride=s)              # [n, C k k, windows]
        gu = F.unfold(g[i:i + chunk] * keep, k, stride=s)
        ku = F.unfold(keep.expand(-1, p.shape[1], -1, -1), k, stride=s)
        spp, spg = (pu * pu).sum(1), (pu * gu).sum(1)
        alpha = torch.where(spp > 1e-5, spg / spp, torch.zeros_like(spp))
        r = (gu - alpha[:, None] * pu) * ku
        out.append((r * r).sum(dim=(1, 2)) / (gu * gu).sum(dim=(1, 2)))
    return torch.cat(out)


def image_metrics(pred, target, mask=None, window_size=20, window_shift=10):
    """{"mse", "psnr", "si_mse", "lmse", "ssim", "dssim"}: [N] float64 device tensors, for [N, H, W, C] float32 inputs without NaNs
    (the masked products above would keep a NaN of an invalid pixel)."""
    p, g = pred.double().permute(0, 3, 1, 2), target.double().permute(0, 3, 1, 2)
    n, c, h, w = p.shape
    valid = torch.ones(n, h, w, dtype=torch.bool, device=p.device) if mask is None else mask > 0
    keep = valid[:, None].to(p.dtype)
    values = c * valid.sum(dim=(1, 2))
    pm, gm = p * keep, g * keep
    spp, spg = (pm * pm).sum(dim=(1, 2, 3)), (pm * gm).sum(dim=(1, 2, 3))
    alpha = torch.where(spp > 1e-5, spg / spp, torch.zeros_like(spp))
    mse = ((gm - pm) ** 2).sum(dim=(1, 2, 3)) / values
    si = ((gm - alpha[:, None, None, None] * pm) ** 2).sum(dim=(1, 2, 3)) / values
    s = ssim(p, g, valid)
    return {"mse": mse, "psnr": -10.0 * torch.log10(mse), "si_mse": si, "lmse": lmse(p, g, valid, window_size, window_shift),
            "ssim": s, "dssim": (1.0 - s) / 2.0}
