"""Shared by test_editing_cpu.py and test_editing_gpu.py: the inputs of the edit kernels (the pattern of test_refresh_gpu's
``_snap_inputs``) and the expectation - the reference's ``update_img`` (gui.py:155-163) restated in torch on the CPU, in fp32 as
the reference evaluates it and in fp64 for the sine mode."""
import math

import numpy as np
import torch

COLS = dict(shading=0, albedo=1, label=4, residual=5)             # [shading | albedo3 | label | residual3 | pad pad], as SNAP_COLS
STRIDE = 10
SCALES = ((1.0, 1.0), (0.37, 1.63), (2.0, 2.0))
CENTER_BEGIN = (0, 4, 8, 12, 12, 17)                               # tests/golden/cluster_lookup.npz: class 3 has no cluster
RECOLOUR = ((0, 1, (255, 16, 0)), (2, 3, (3, 200, 77)), (4, 4, (128, 128, 255)))      # (semantic, class, sliders); one in the last class


def edit_inputs(n, mode, K):
    """[n, STRIDE] fp32 pack and its int64 labels: albedo in [0.02, 0.97], shading in [0, 2], residual in [-0.5, 1.5]; labels walk
    through -1 .. K + 1, one per 8-pixel tile ("uniform") or mixed inside the tiles; pixel 0 is black (a NaN mapped colour),
    pixels 1 / 2 give results below 0 / above 1, pixel 3 has a NaN shading."""
    g = np.random.RandomState(11 * n + len(mode))
    pack = np.zeros((n, STRIDE), np.float32)
    pack[:, 1:4] = g.rand(n, 3) * 0.95 + 0.02
    pack[:, 0] = g.rand(n) * 2.0
    pack[:, 5:8] = g.rand(n, 3) * 2.0 - 0.5
    pack[:, 8:] = g.rand(n, 2)
    if mode == "uniform":
        lab = (np.arange(n) // 8 + 1) % (K + 3) - 1
    else:
        lab = g.randint(-1, K + 2, size=n)
    lab[0] = 0
    pack[0, 1:4] = 0.0
    if n > 3:
        pack[1, 5:8] = -2.0
        pack[2, 5:8] = 2.0
        pack[3, 0] = np.nan
    if mode == "ignore":
        lab[:] = 0
    pack[:, 4] = lab
    return pack, lab.astype(np.int64)


def u8_inputs(n, K, seed=0):
    """The 8-bit planes ``load_all_image`` reads, flat: albedo [n, 3], shading [n], residual [n, 3] uint8, labels [n] in -1 .. K + 1."""
    g = np.random.RandomState(1000 + 13 * n + seed)
    albedo = g.randint(0, 256, size=(n, 3)).astype(np.uint8)
    shading = g.randint(0, 256, size=n).astype(np.uint8)
    residual = g.randint(0, 256, size=(n, 3)).astype(np.uint8)
    lab = g.randint(-1, K + 2, size=n).astype(np.int64)
    lab[0] = 0
    albedo[0] = 0                                                 # black
    return albedo, shading, residual, lab


def unit(u8):
    """gui.py:218: (np.array(img) / 255.).astype(np.float32)"""
    return (np.asarray(u8) / 255.).astype(np.float32)


def u8_pack(albedo, shading, residual, lab):
    """The fp32 pack of u8 planes in COLS' layout."""
    n = shading.shape[0]
    pack = np.zeros((n, STRIDE), np.float32)
    pack[:, 1:4], pack[:, 0], pack[:, 5:8], pack[:, 4] = unit(albedo), unit(shading), unit(residual), lab
    return pack


def expected_slots(lab, dest_class, center_begin=CENTER_BEGIN):
    """center_begin[label] + dest_class where the label's class has a cluster, -1 elsewhere."""
    K = len(center_begin) - 1
    begin = np.asarray(center_begin, np.int64)
    inside = (lab >= 0) & (lab < K)
    safe = np.where(inside, lab, 0)
    has = inside & (begin[safe + 1] > begin[safe])
    return np.where(has, begin[safe] + dest_class, -1).astype(np.int32)


def update_img(albedo, shading, residual, label, albedo_class, rgb_centers, change_shading=False, change_residual=False,
               shading_scale=1.0, residual_scale=1.0, dtype=torch.float32):
    """gui.py:155-163 on flat CPU tensors: albedo / residual [n, 3], shading [n], label and albedo_class [n] int64;
    ``rgb_centers[i]`` = class i's [c, 3] centres or None.  Returns ``(cluster_albedo, img)``.  With ``dtype=torch.float64`` the
    same expressions on the same fp32 inputs, scales and constants rounded to fp32 first: the yardstick of the sine mode."""
    f32 = lambda v: float(np.float32(v))
    albedo, residual = torch.as_tensor(albedo).to(dtype), torch.as_tensor(residual).to(dtype)
    shading = torch.as_tensor(shading).to(dtype)[:, None].repeat(1, 3)                   # np.repeat(shading[..., None], 3, axis=3), :223
    label, albedo_class = torch.as_tensor(label).reshape(-1), torch.as_tensor(albedo_class).reshape(-1)
    cluster_albedo = albedo.clone()
    for i in range(len(rgb_centers)):
        if rgb_centers[i] is None:
            continue
        class_idx = label == i
        cluster_albedo[class_idx] = torch.as_tensor(rgb_centers[i]).to(dtype)[albedo_class[class_idx]]
    pi, half_pi = (math.pi, math.pi / 2) if dtype == torch.float32 else (f32(math.pi), f32(math.pi / 2))
    t_shading = shading ** 2 if change_shading else shading
    t_residual = (torch.sin(residual * pi - half_pi) + 1) / 2 if change_residual else residual
    if dtype == torch.float32:
        img = cluster_albedo * t_shading * shading_scale + t_residual * residual_scale
    else:
        img = cluster_albedo * t_shading * f32(shading_scale) + t_residual * f32(residual_scale)
    return cluster_albedo, img


def to8b(x):
    """to8b (run_nerf_helpers.py:13) on a numpy array in its own precision, NaN -> 0 as the kernels write it."""
    x = np.asarray(x)
    return (255 * np.clip(np.where(np.isnan(x), x.dtype.type(0), x), 0, 1)).astype(np.uint8)


def same_floats(got, want):
    """Bit for bit; a NaN exactly where the expectation has one."""
    got, want = torch.as_tensor(got).cpu().contiguous(), torch.as_tensor(want).cpu().contiguous()
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        return False
    zero = torch.zeros((), dtype=torch.float32)
    return torch.equal(torch.where(nan, zero, got).view(torch.int32), torch.where(nan, zero, want).view(torch.int32))
