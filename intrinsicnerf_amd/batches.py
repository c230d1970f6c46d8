"""Training batches assembled on the GPU: pixel draw, rays and targets in one launch (csrc/batch.hip, ``inerf_batch_assemble``).

``ObjectBatcher.next(i)`` replaces run_nerf.py:886-938 - ``img_i``, the whole-image upload, ``get_rays`` of the whole frame, the
``coords`` meshgrid, ``np.random.choice(replace=False)``, ``select_neighbor`` and the gathers - and ``SSRBatcher.next()`` replaces
``SSRTrainer.sample_data`` with ``no_batching=True`` (trainer.py:627-691, rays.py:153-172).  The image / mask / pose stacks are
uploaded once; a batch is then one kernel over device-resident tables.

Indices come from the caller (``indices=``, the reference's draw order; what the exactness tests use) or are drawn in the kernel
from ``(seed, step, ray)`` by integer hashing (tests/_batch_draw.py restates it).  ``next(i)`` draws step ``i``; ``next()`` draws
the step a device-resident counter holds and advances it in the same call, so a ``next()`` captured into a HIP graph
(``torch.cuda.graph``, or inside ``graphs.GraphedTrainStep``'s ``loss_fn``) yields a new batch on every replay.

Out of scope: the object-level ``use_batching`` branch (run_nerf.py:829-883) - it never defines ``target_m``, so the reference's
own loss line fails on it.
"""
import numpy as np
import torch

from . import kernels


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("intrinsicnerf_amd.batches needs a HIP device (no CPU / eager fallback exists)")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"intrinsicnerf_amd.batches runs only on a HIP device, not on {device}")
    return device


def _resident(x, name, device, dtype=None):
    """A host array (numpy, as the reference's loaders return it) is uploaded once; a tensor must already live on the device."""
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError(f"{name} lives on {x.device}: intrinsicnerf_amd runs only on a HIP device (no CPU / eager fallback "
                               "exists); pass the loader's numpy array, or a device tensor")
        return (x if dtype is None else x.to(dtype)).contiguous()
    x = np.ascontiguousarray(x)
    t = torch.from_numpy(x)
    return (t if dtype is None else t.to(dtype)).to(device)


def _index_tensors(indices, device):
    image, pixels, off_row, off_col = indices
    conv = lambda v: (v.to(device=device, dtype=torch.int64) if isinstance(v, torch.Tensor)
                      else torch.as_tensor(np.asarray(v), dtype=torch.int64).to(device)).reshape(-1)
    image = conv(image) if isinstance(image, torch.Tensor) else int(np.asarray(image).reshape(-1)[0])
    return image, conv(pixels), conv(off_row), conv(off_col)


class _Batcher:
    def _init_draw(self, seed, device, image_ids):
        self.seed = int(seed)
        self.device = device
        self.step = torch.zeros(1, dtype=torch.int64, device=device)          # the device step counter of next()
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.image_ids = None if image_ids is None else torch.as_tensor(np.asarray(image_ids), dtype=torch.int64).to(device)
        self.calls = 0                                                        # host mirror: next() calls WITHOUT i issued (not replays; next(i) leaves it alone)

    def _draw(self, i):
        if i is None:
            return dict(seed=self.seed, step_dev=self.step, advance=True, image_ids=self.image_ids)
        return dict(seed=self.seed, step=int(i), image_ids=self.image_ids)

    def reset(self, step=0):
        """Set the device step counter (and the host's count of issued calls)."""
        self.step.fill_(int(step))
        self.calls = int(step)

    def check(self):
        """Read the status word (synchronises): raises if an index was clamped or a cycle walk reached its bound."""
        kernels.check_batch_status(self.status, type(self).__name__)


class ObjectBatcher(_Batcher):
    """``next(i)`` -> ``(batch_rays [2, 2 N_rand, 3], target_s [2 N_rand, 3], target_m [2 N_rand, 1])`` of iteration ``i``
    (run_nerf.py:886-938), the centre crop applied while ``i < precrop_iters``.

    ``images`` [n, H, W, 3], ``masks`` [n, H, W, 1] (or [n, H, W]; None: no ``target_m``), ``poses`` [n, >=3, >=4]: numpy arrays
    as the loaders return them (uploaded once, as fp32) or device tensors.  ``K``: the 3x3 intrinsics.  ``i_train``: the ids
    ``np.random.choice(i_train)`` draws from.  ``next(i, indices=(image, pixels, off_row, off_col))`` takes the reference's own
    draws: ``pixels`` = ``select_inds`` (indices into the current window), ``off_row`` = ``bias_x``, ``off_col`` = ``bias_y``.
    ``next()`` without ``i`` draws from the device step counter and advances it (capturable); the window is then decided by the
    number of no-argument ``next()`` calls issued so far, so a captured graph keeps the window it was captured with."""

    def __init__(self, images, masks, poses, K, i_train, N_rand, precrop_iters=0, precrop_frac=0.5, seed=0, device=None):
        device = _device(device if device is not None else (images.device if isinstance(images, torch.Tensor) else None))
        self.images = _resident(images, "images", device, torch.float32)
        if self.images.dim() != 4 or self.images.shape[-1] != 3:
            raise ValueError(f"images has shape {tuple(self.images.shape)}, expected [n, H, W, 3]")
        n, self.H, self.W = (int(s) for s in self.images.shape[:3])
        self.masks = None
        if masks is not None:
            self.masks = _resident(masks, "masks", device, torch.float32).reshape(n, self.H, self.W, 1)
        poses = _resident(poses, "poses", device, torch.float32)
        self.poses = poses[:, :3, :4].contiguous()                            # run_nerf.py:897
        K = np.asarray(K, dtype=np.float64)
        self.intrinsics = (K[0][0], K[1][1], K[0][2], K[1][2])                # get_rays, run_nerf_helpers.py:359-368
        self.N_rand, self.precrop_iters, self.precrop_frac = int(N_rand), int(precrop_iters), float(precrop_frac)
        self._init_draw(seed, device, i_train)

    def window(self, i):
        """(row0, col0, rows, cols) of iteration ``i``: run_nerf.py:902-913."""
        if i < self.precrop_iters:
            dH, dW = int(self.H // 2 * self.precrop_frac), int(self.W // 2 * self.precrop_frac)
            return self.H // 2 - dH, self.W // 2 - dW, 2 * dH, 2 * dW
        return 0, 0, self.H, self.W

    def next(self, i=None, indices=None, return_indices=False):
        window = self.window(self.calls if i is None else int(i))
        if i is None:
            self.calls += 1
        if indices is not None:
            indices = _index_tensors(indices, self.device)
            n = int(indices[1].shape[0])
            draw = None
        else:
            n, draw = self.N_rand, self._draw(i)
        return kernels.batch_object(self.images, self.masks, self.poses, self.intrinsics, window, n, indices=indices, draw=draw,
                                    status=self.status, return_indices=return_indices)


class SSRBatcher(_Batcher):
    """``next()`` -> what ``SSRTrainer.sample_data(no_batching=True)`` returns (trainer.py:627-691): ``(sampled_rays [2n, 11],
    gt_rgb [2n, 3], gt_depth [2n], gt_semantic [2n] int64, flag)`` with ``enable_semantic``, else ``(sampled_rays, gt_rgb)``.

    ``image`` [n_img, H, W, 3] fp32 | fp64, ``depth`` [n_img, H, W] fp32 | fp64, ``semantic`` [n_img, H, W] integer - the trainer's
    device-resident tables (numpy arrays are uploaded once, in their own dtype).  Rays: the trainer's table ``rays``
    [n_img, H*W, 11], or ``camera`` = dict(poses, fx, fy, cx, cy, near, far, opengl), from which the same rows are computed.
    ``mask_ids`` [n_img]: the per-image availability of semantic labels; ``flag`` is ``mask_ids[image]`` as a device fp64 [1, 1]
    (1 without ``mask_ids``).  ``next(i, indices=(image, pixels, off_row, off_col))``: ``pixels`` flat ``h * W + w``,
    ``off_row`` = ``bias_h``, ``off_col`` = ``bias_w``."""

    def __init__(self, image, depth=None, semantic=None, n_rays=1024, rays=None, camera=None, mask_ids=None, enable_semantic=True,
                 seed=0, device=None):
        device = _device(device if device is not None else (image.device if isinstance(image, torch.Tensor) else None))
        self.image = _resident(image, "image", device)
        self.enable_semantic = bool(enable_semantic)
        self.depth = _resident(depth, "depth", device) if (depth is not None and self.enable_semantic) else None
        self.semantic = _resident(semantic, "semantic", device) if (semantic is not None and self.enable_semantic) else None
        self.mask_ids = _resident(mask_ids, "mask_ids", device, torch.float64) if (mask_ids is not None and self.enable_semantic) else None
        self.rays = _resident(rays, "rays", device, torch.float32) if rays is not None else None
        self.camera = None
        if camera is not None:
            self.camera = dict(camera, poses=_resident(camera["poses"], "camera['poses']", device, torch.float32))
        self.n_rays = int(n_rays)
        self._init_draw(seed, device, None)

    def next(self, i=None, indices=None, return_indices=False):
        if i is None:
            self.calls += 1
        if indices is not None:
            indices = _index_tensors(indices, self.device)
            n, draw = int(indices[1].shape[0]), None
        else:
            n, draw = self.n_rays, self._draw(i)
        out = kernels.batch_ssr(self.image, self.depth, self.semantic, n, rays=self.rays, camera=self.camera, avail=self.mask_ids,
                                indices=indices, draw=draw, status=self.status, return_indices=return_indices)
        rays, rgb, depth, sem, avail = out[:5]
        if self.enable_semantic:
            flag = avail.reshape(1, 1) if avail is not None else 1
            res = (rays, rgb, depth, sem, flag)
        else:
            res = (rays, rgb)
        return res + (out[5],) if return_indices else res
