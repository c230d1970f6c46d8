"""The reference's edit engine as plain torch expressions - what a slider tick does without csrc/edit.hip, and the comparison
partner of scripts/bench_editing.py.

The same steps, of the same kind, as gui.py's: ``load_all_image`` (:185-256) uploads every frame as fp32 - albedo, shading
repeated to three channels, residual - and the labels as int64; ``cluster_img`` (:268-281) keeps ``dest_class`` of every pixel
(here through this package's lookup: it is start-up, not the tick); ``update_img`` (:139-182) then runs, per tick and frame, one
boolean-mask gather and one scatter per semantic class that has a cluster, the compose line, a blocking ``.cpu()`` and ``to8b``
on the host (``numpy_to_photo``, :258-262)."""
import math

import numpy as np
import torch


class TorchEditor:
    def __init__(self, manager, albedo, shading, residual, label, device):
        """``albedo`` [F, H, W, 3], ``shading`` [F, H, W], ``residual`` [F, H, W, 3] uint8 and ``label`` [F, H, W] integers, as the
        PNG files hold them."""
        from intrinsicnerf_amd import cluster
        unit = lambda a: (np.asarray(a) / 255.).astype(np.float32)
        self.albedos_gpu = torch.from_numpy(unit(albedo)).to(device)
        self.shadings_gpu = torch.from_numpy(np.repeat(unit(shading)[..., None], 3, axis=3)).to(device)
        self.residuals_gpu = torch.from_numpy(unit(residual)).to(device)
        self.labels_gpu = torch.from_numpy(np.asarray(label).astype(np.int64)[..., None]).to(device)
        shape = self.labels_gpu.shape
        self.cluster_albedo_class = cluster.dest_class(manager, self.albedos_gpu.reshape(-1, 3), self.labels_gpu.reshape(-1, 1)).reshape(shape)
        self.ori_rgb_centers = [None if c is None else torch.as_tensor(cluster._field(c, "rgb_centers")).to(device).clone()
                                for c in list(manager.clusters)[:manager.class_num]]
        self.reset()

    def reset(self):
        self.rgb_centers = [None if c is None else c.clone() for c in self.ori_rgb_centers]
        self.global_shading_scale = self.global_residual_scale = 1.0
        self.global_change_shading = self.global_change_residual = False

    def update_color(self, semantic_idx, class_idx, red, green, blue):
        self.rgb_centers[semantic_idx][class_idx, 0] = float(red) / 255.0
        self.rgb_centers[semantic_idx][class_idx, 1] = float(green) / 255.0
        self.rgb_centers[semantic_idx][class_idx, 2] = float(blue) / 255.0

    def t_shading(self, s):
        return s ** 2 if self.global_change_shading else s

    def t_residual(self, r):
        return (torch.sin(r * math.pi - math.pi / 2) + 1) / 2 if self.global_change_residual else r

    def compose(self, idx):
        """The device part of ``update_img``: the float image of frame ``idx``, left on the device."""
        cluster_albedo = self.albedos_gpu[idx].clone()
        for i in range(len(self.rgb_centers)):
            if self.rgb_centers[i] is None:
                continue
            class_idx = torch.squeeze(self.labels_gpu[idx] == i)
            albedo_class = self.cluster_albedo_class[idx][class_idx]
            cluster_albedo[class_idx] = torch.squeeze(self.rgb_centers[i][albedo_class])
        return (cluster_albedo * self.t_shading(self.shadings_gpu[idx]) * self.global_shading_scale
                + self.t_residual(self.residuals_gpu[idx]) * self.global_residual_scale)

    def update_img(self, idx):
        """One tick: the shown 8-bit image of frame ``idx`` on the host."""
        img = self.compose(idx).cpu().numpy()
        return (255 * np.clip(img, 0, 1)).astype(np.uint8)
