"""The trainers' batch assembly as plain host + torch expressions - what an iteration does without csrc/batch.hip, and the comparison
partner of scripts/bench_batches.py and ``scripts/bench_train_step.py --batch inerf``.

The same steps, of the same kind, as the reference's (object_level/run_nerf.py:886-938; SSR/training/trainer.py:627-691 with
SSR/models/rays.py:153-172), host draws and uploads included: the object level picks an image, uploads it and its mask, generates
the rays of the whole frame and builds the [H*W, 2] coordinate grid on the device (the reference runs under a cuda default tensor
type), permutes every pixel index on the host
(np.random.choice(replace=False)), draws the two neighbour offsets with numpy, uploads them and gathers; the SSR trainer draws on the
host and gathers from its device-resident tables."""
import numpy as np
import torch


def frame_rays(H, W, K, c2w):
    """Origins and directions of every pixel of a pinhole frame (the object level's convention: x right, y up, looking down -z),
    on the device of ``c2w``."""
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=c2w.device), torch.linspace(0, H - 1, H, device=c2w.device))
    i, j = i.t(), j.t()
    dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)
    return c2w[:3, -1].expand(rays_d.shape), rays_d


def object_batch(i, images, masks, poses, K, i_train, n_rand, precrop_iters, precrop_frac, device):
    """(batch_rays [2, 2N, 3], target_s [2N, 3], target_m [2N, 1]) of iteration ``i``, all on ``device``, from HOST image / mask /
    pose stacks: the image, the mask, the pose and the two offset arrays are uploaded, everything else is computed on ``device``."""
    H, W = images.shape[1:3]
    img_i = np.random.choice(i_train)
    target = torch.Tensor(images[img_i]).to(device)
    target_mask = torch.Tensor(masks[img_i]).to(device)
    rays_o, rays_d = frame_rays(H, W, K, torch.Tensor(poses[img_i, :3, :4]).to(device))
    if i < precrop_iters:
        dH, dW = int(H // 2 * precrop_frac), int(W // 2 * precrop_frac)
        rows = torch.linspace(H // 2 - dH, H // 2 + dH - 1, 2 * dH, device=device)
        cols = torch.linspace(W // 2 - dW, W // 2 + dW - 1, 2 * dW, device=device)
    else:
        rows, cols = torch.linspace(0, H - 1, H, device=device), torch.linspace(0, W - 1, W, device=device)
    coords = torch.stack(torch.meshgrid(rows, cols), -1).reshape(-1, 2)
    select = coords[np.random.choice(coords.shape[0], size=[n_rand], replace=False)].long()
    off = [torch.from_numpy(np.random.choice([-1, 0, 1], select.shape[0])).to(device) for _ in range(2)]
    nei = select.clone()
    nei[:, 0] = torch.clamp(nei[:, 0] + off[0], 0, H - 1)
    nei[:, 1] = torch.clamp(nei[:, 1] + off[1], 0, W - 1)
    sel = torch.cat((select, nei), 0)
    rays_o, rays_d = rays_o[sel[:, 0], sel[:, 1]], rays_d[sel[:, 0], sel[:, 1]]
    return torch.stack([rays_o, rays_d], 0), target[sel[:, 0], sel[:, 1]], target_mask[sel[:, 0], sel[:, 1]]


def ssr_batch(rays, image, depth, semantic, mask_ids, n_rays):
    """(sampled_rays [2n, 11], gt_rgb, gt_depth, gt_semantic int64, flag) from device-resident tables, draws on the host."""
    n_img, hw = rays.shape[:2]
    h, w = image.shape[1:3]
    index_b = np.random.choice(np.arange(n_img)).reshape((1, 1))
    index_hw = torch.randint(0, hw, (1, n_rays))
    bias_w = torch.from_numpy(np.random.choice([-1, 0, 1], n_rays))
    bias_h = torch.from_numpy(np.random.choice([-1, 0, 1], n_rays))
    nh = torch.clamp(index_hw // w + bias_h, 0, h - 1)
    nw = torch.clamp(index_hw % w + bias_w, 0, w - 1)
    index_hw = torch.cat((index_hw, nh * w + nw), 1)
    sampled = rays[index_b, index_hw, :].reshape(-1, rays.shape[-1]).float()
    rgb = image.reshape(n_img, -1, 3)[index_b, index_hw, :].reshape(-1, 3)
    dep = depth.reshape(n_img, -1)[index_b, index_hw].reshape(-1)
    sem = semantic.reshape(n_img, -1)[index_b, index_hw].reshape(-1).long()
    return sampled, rgb, dep, sem, mask_ids[index_b]
