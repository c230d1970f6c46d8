"""Drop-in front-end for the scene-level code base (``SSR/`` + ``train_SSR_main.py``).

Mirrors, with identical names / argument meaning / returned keys (citations relative to
``/root/reference/SSR``):
  Semantic_NeRF            models/semantic_nerf.py:74-181     get_embedder   models/semantic_nerf.py:50-65
  run_network              models/model_utils.py:19-35        raw2outputs    models/model_utils.py:39-116
  sample_pdf               models/rays.py:176-220             create_rays    models/rays.py:223-256
  batchify_rays            training/training_utils.py:5-17
  SSRRenderMixin.render_rays / volumetric_rendering / create_ssr
                           training/trainer.py:693-715 / 717-808 / 811-846
``SSRTrainer`` keeps its data loading, losses and logging; it only has to inherit the mixin (or
assign the three methods) - see INTEGRATION.md.  All arithmetic runs in ``libinerf.so``; the control
path shared with ``object_level.py`` - fusability, the chunk loop with its f16 range fallback, the
staged pass of a training step - is ``render_core.py``.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _capi, kernels, render_core
from .object_level import Embedder
from .render_core import _fusable, _train_desc, _training_path_notice, _unfused_notice, _wants_grad
from .losses import compute_intrinsic_loss_ssr as compute_intrinsic_loss, ssr_step_loss  # noqa: F401  (training_utils.py:179-207, trainer.py:923-988)

__all__ = ["get_embedder", "Semantic_NeRF", "run_network", "raw2outputs", "sample_pdf", "create_rays",
           "get_rays_camera", "get_rays_world", "batchify_rays", "SSRRenderMixin", "SSRRenderer",
           "compute_intrinsic_loss", "ssr_step_loss"]


def get_embedder(multires, i=0, scalar_factor=1):
    """(embed_fn, out_dim); the input is divided by ``scalar_factor`` first - semantic_nerf.py:50-65."""
    if i == -1:
        return nn.Identity(), 3
    e = Embedder(multires, scalar_factor=scalar_factor)
    return e, e.out_dim


def fc_block(in_f, out_f):
    return nn.Sequential(nn.Linear(in_f, out_f), nn.ReLU(out_f))


class Semantic_NeRF(nn.Module):
    """Intrinsic NeRF + position-only semantic head, reference parameter names (semantic_nerf.py:98-118).

    ``semantic_linear.0.0`` / ``semantic_linear.1``, ``residual_linear``, ``albedo_linear1/2``,
    ``shading_linear1/2``.  As for the object-level module, ``forward`` defines the network in torch
    ops for holders of an embedded tensor; the render path uses the fused kernel instead.
    """

    def __init__(self, enable_semantic, num_semantic_classes, D=8, W=256, input_ch=3, input_ch_views=3, output_ch=4,
                 skips=[4], use_viewdirs=False):
        super().__init__()
        self.D, self.W = D, W
        self.input_ch, self.input_ch_views = input_ch, input_ch_views
        self.skips = list(skips)
        self.use_viewdirs = use_viewdirs
        self.enable_semantic = enable_semantic
        self.num_semantic_classes = num_semantic_classes if enable_semantic else 0
        self.pts_linears = nn.ModuleList(
            [nn.Linear(input_ch, W)] +
            [nn.Linear(W + input_ch, W) if i in self.skips else nn.Linear(W, W) for i in range(D - 1)])
        self.views_linears = nn.ModuleList([nn.Linear(input_ch_views + W, W // 2)])
        if use_viewdirs:
            self.feature_linear = nn.Linear(W, W)
            self.alpha_linear = nn.Linear(W, 1)
            if enable_semantic:
                self.semantic_linear = nn.Sequential(fc_block(W, W // 2), nn.Linear(W // 2, num_semantic_classes))
            self.residual_linear = nn.Linear(W // 2, 3)
            self.albedo_linear1 = nn.Linear(W, W // 2)
            self.albedo_linear2 = nn.Linear(W // 2, 3)
            self.shading_linear1 = nn.Linear(W, W // 2)
            self.shading_linear2 = nn.Linear(W // 2, 1)
        else:
            self.output_linear = nn.Linear(W, output_ch)

    def fused_desc(self):
        if not (self.use_viewdirs and self.D == 8 and self.W == 256 and self.skips == [4]):
            return None
        l_xyz, rx = divmod(self.input_ch - 3, 6)
        l_dir, rd = divmod(self.input_ch_views - 3, 6)
        if rx or rd or not (0 <= l_xyz <= 10 and 0 <= l_dir <= 4) or self.num_semantic_classes > _capi.MAX_CLASSES:
            return None
        return _capi.net_desc(_capi.VARIANT_SSR, self.num_semantic_classes, l_xyz, l_dir, 1.0)

    def forward(self, x, show_endpoint=False):
        pts, views = torch.split(x, [self.input_ch, self.input_ch_views], dim=-1)
        h = pts
        for i, layer in enumerate(self.pts_linears):
            h = F.relu(layer(h))
            if i in self.skips:
                h = torch.cat([pts, h], -1)
        if not self.use_viewdirs:
            out = self.output_linear(h)
            return out
        sigma = self.alpha_linear(h)
        sem = self.semantic_linear(h) if self.enable_semantic else None
        albedo = torch.sigmoid(self.albedo_linear2(F.relu(self.albedo_linear1(h))))
        shading = torch.sigmoid(self.shading_linear2(F.relu(self.shading_linear1(h))))
        v = torch.cat([self.feature_linear(h), views], -1)
        for layer in self.views_linears:
            v = F.relu(layer(v))
        residual = torch.sigmoid(self.residual_linear(v))
        rgb = albedo * shading + residual
        parts = [rgb, sigma, albedo, shading, residual] + ([sem] if sem is not None else [])
        if show_endpoint:
            parts.append(v)
        return torch.cat(parts, -1)


def run_network(inputs, viewdirs, fn, embed_fn, embeddirs_fn, netchunk=1024 * 64, show_endpoint=False):
    """Encode + apply the network - model_utils.py:19-35.  ``fn`` is a Semantic_NeRF (fused HIP launch) or
    any callable on the embedded tensor (called as the reference does).  ``show_endpoint`` is what the
    reference expresses as ``lambda x: net(x, self.endpoint_feat)`` (trainer.py:770)."""
    return render_core.run_network(inputs, viewdirs, fn, embed_fn, embeddirs_fn, netchunk, endpoint=show_endpoint,
                                   foreign=(lambda x: fn(x, True)) if show_endpoint else None)          # trainer.py:770


def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=False, enable_semantic=True, num_sem_class=0,
                endpoint_feat=False):
    """Compositing incl. semantic logits / endpoint feature - model_utils.py:39-116.

    Returns ``(rgb, disp, acc, weights, depth, sem, feat, albedo, shading, residual)``; ``sem`` / ``feat``
    are ``torch.tensor(0)`` when disabled, as in the reference.
    """
    if enable_semantic:
        assert num_sem_class > 0
    noise = torch.randn(raw[..., 3].shape, device=raw.device) * raw_noise_std if raw_noise_std > 0. else None
    o = kernels.composite(raw.float(), z_vals.float(), rays_d.float(), noise, white_bkgd,
                          n_classes=num_sem_class if enable_semantic else 0, feat_dim=128 if endpoint_feat else 0)
    sem = o["sem"] if enable_semantic else torch.tensor(0)
    feat = o["feat"] if endpoint_feat else torch.tensor(0)
    return o["rgb"], o["disp"], o["acc"], o["weights"], o["depth"], sem, feat, o["albedo"], o["shading"], o["residual"]


def sample_pdf(bins, weights, N_samples, det=False):
    """Inverse-CDF sampling - rays.py:176-220."""
    b2 = torch.reshape(bins, [-1, bins.shape[-1]]).float()
    w2 = torch.reshape(weights, [-1, weights.shape[-1]]).float()
    if det:
        u = torch.linspace(0., 1., steps=N_samples, device=bins.device)
    else:
        u = torch.rand(b2.shape[0], N_samples, device=bins.device)
    return torch.reshape(kernels.sample_pdf(b2, w2, u, N_samples), list(bins.shape[:-1]) + [N_samples])


# ----------------------------------------------------------------------------------------------
# ray generation (input producer; rays.py:27-67,223-256)
# ----------------------------------------------------------------------------------------------
def get_rays_camera(B, H, W, fx, fy, cx, cy, depth_type="z", convention="opencv"):
    assert depth_type in ("z", "euclidean")
    j, i = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    i = i.float()[None].expand(B, H, W)
    j = j.float()[None].expand(B, H, W)
    if convention == "opencv":
        dirs = torch.stack(((i - cx) / fx, (j - cy) / fy, torch.ones(B, H, W)), dim=3)
    elif convention == "opengl":
        dirs = torch.stack(((i - cx) / fx, -(j - cy) / fy, -torch.ones(B, H, W)), dim=3)
    else:
        raise AssertionError(convention)
    if depth_type == "euclidean":
        dirs = dirs * (1. / torch.norm(dirs, dim=3, keepdim=True))
    return dirs


def get_rays_world(T_WC, dirs_C):
    R_WC = T_WC[:, :3, :3]
    dirs_W = torch.matmul(R_WC[:, None, ...], dirs_C[..., None]).squeeze(-1)
    origins = torch.broadcast_tensors(T_WC[:, :3, -1][:, None, :], dirs_W)[0]
    return origins, dirs_W


def create_rays(num_rays, Ts_c2w, height, width, fx, fy, cx, cy, near, far, c2w_staticcam=None, depth_type="z",
                use_viewdirs=True, convention="opencv"):
    """[num_images, H*W, 11] ray batch ``[o3, d3, near, far, viewdir3]`` - rays.py:223-256.

    Poses on a HIP device (and depth_type "z", view directions on - every shipped config): one ``inerf_gen_rays`` launch
    that reproduces the reference's CPU bits; CPU poses (what trainer.py:608-624 passes) take the torch expressions below,
    which ARE the reference's."""
    if (isinstance(Ts_c2w, torch.Tensor) and Ts_c2w.is_cuda and depth_type == "z" and use_viewdirs
            and (c2w_staticcam is None or (isinstance(c2w_staticcam, torch.Tensor) and c2w_staticcam.is_cuda))):
        if Ts_c2w.shape[0] != num_rays:
            raise ValueError(f"create_rays: {num_rays} images but {Ts_c2w.shape[0]} poses")
        rays = kernels.gen_rays(Ts_c2w.float(), height, width, fx, fy, cx, cy, near, far, convention == "opengl",
                                None if c2w_staticcam is None else c2w_staticcam.float())
        return rays.reshape(num_rays, height * width, -1)
    dirs_C = get_rays_camera(num_rays, height, width, fx, fy, cx, cy, depth_type=depth_type,
                             convention=convention).view(num_rays, -1, 3).to(Ts_c2w.device)
    rays_o, rays_d = get_rays_world(Ts_c2w, dirs_C)
    if use_viewdirs:
        viewdirs = rays_d
        if c2w_staticcam is not None:
            rays_o, rays_d = get_rays_world(c2w_staticcam, dirs_C)
        viewdirs = viewdirs / torch.norm(viewdirs, dim=-1, keepdim=True).float()
    near, far = near * torch.ones_like(rays_d[..., :1]), far * torch.ones_like(rays_d[..., :1])
    rays = torch.cat([rays_o, rays_d, near, far], -1)
    if use_viewdirs:
        rays = torch.cat([rays, viewdirs], -1)
    return rays


def batchify_rays(render_fn, rays_flat, chunk=1024 * 32, coalesce_to=None, with_ray_base=False):
    """training_utils.py:5-17 on render_core.render_chunks: the chunks' f16 range words are read together after the
    last chunk (one host synchronisation per frame) and only the chunks that left the range are rendered again in exact
    fp32.  ``coalesce_to`` (SSRRenderMixin.render_rays, eval-mode frames whose result cannot depend on the chunk boundaries):
    rays per call instead of ``chunk``; the launches keep one f16 range word per ``chunk`` rays, so a chunk that leaves the range is still the
    only one rendered again.  ``with_ray_base``: ``render_fn`` is also given every chunk's first global ray index (``ray_base=``), the base
    of its training draws (SSRRenderMixin.draws)."""
    def piece(i, count):
        return render_fn(rays_flat[i:i + count], ray_base=i) if with_ray_base else render_fn(rays_flat[i:i + count])

    return render_core.render_chunks(piece, rays_flat.shape[0], chunk, max(chunk, coalesce_to or 0), "render_rays")


# ----------------------------------------------------------------------------------------------
# the trainer's render methods
# ----------------------------------------------------------------------------------------------
class SSRRenderMixin:
    """``render_rays`` / ``volumetric_rendering`` / ``create_ssr`` of SSRTrainer (trainer.py:693-846).

    Reads the same attributes the reference methods read: ``N_samples, N_importance, perturb,
    training, raw_noise_std, white_bkgd, enable_semantic, num_valid_semantic_class, endpoint_feat,
    netchunk, chunk, ssr_net_coarse, ssr_net_fine, embed_fn, embeddirs_fn``.  Two optional extras:
    ``return_raw`` (default True, as the reference always returns raw_coarse / raw_fine - ~3 GB per
    320x240 frame; set False to skip materialising them for the caller) and ``check_numerics``
    (default True: the reference's ungated nan/inf print, trainer.py:803-806, one device sync per key).
    """

    return_raw = True
    check_numerics = True
    cluster_refresh = None        # a refresh.ClusterRefresh: render_path(update_cluster=True) keeps its sample set, fit and c / edit images on the device
    frame_products = None         # a frames.FrameProducts: render_path takes every 8- / 16-bit image - the jet maps of depth and entropy included, no imgviz - from csrc/frame_vis.hip
    frame_evaluator = None        # an evaluation.FrameEvaluator: render_path takes the label / entropy maps from csrc/eval.hip and accumulates the metrics of registered frame sets
    # a draws.DrawState: in training mode the jitter, the per-ray u (perturb > 0) and the density noise (raw_noise_std > 0) are drawn inside
    # the kernels as a function of (seed, step, stream, global ray index, sample) - the same bits for any `chunk`; None: torch's generator
    draws = None

    def render_rays(self, flat_rays):
        ray_shape = flat_rays.shape
        loop = (self.volumetric_rendering, flat_rays, self.chunk, self._coalesced(flat_rays))
        if self.draws is not None and bool(self.training) and (self.perturb > 0. or self.raw_noise_std > 0.):
            # (eval-mode frames and renders that draw nothing leave the step alone: it counts drawing renders)
            all_ret = render_core.advance_after(self.draws, batchify_rays, *loop, with_ray_base=True)
        else:
            all_ret = batchify_rays(*loop)      # one host synchronisation per frame
        for k in all_ret:
            all_ret[k] = torch.reshape(all_ret[k], list(ray_shape[:-1]) + list(all_ret[k].shape[1:]))
        return all_ret

    def render_path(self, rays, save_dir=None, update_cluster=False, b_f=0.5):
        """Render the frames ``rays[i]`` ([n_images, H*W, 11]) - trainer.py:1221-1456; returns the reference's 12-tuple
        ``(rgbs, disps, deps, vis_deps, sems, vis_sems, entropys, vis_entropys, albedos, shadings, residuals,
        cluster_manager)``.

        Per frame the label map (argmax of the softmax, :1244) and the entropy map (:1245) are computed on the device, all
        maps travel to the host as one pinned asynchronous copy that overlaps the next frame's kernels
        (frames.FrameStreamer) - the reference issues ~10 blocking ``.cpu()`` calls per frame.  The visualisations are
        the trainer's own business: ``vis_deps`` / ``vis_entropys`` need ``imgviz.depth2rgb`` (None when imgviz is not
        importable), ``vis_sems`` reads ``self.valid_colour_map`` (None without it).  Reads ``H_scaled, W_scaled, near,
        far`` like the reference.  ``update_cluster`` needs ``self.cluster_manager_factory`` (the reference's
        ``Cluster_Manager``: its mean-shift fitting is training control plane, not rebuilt here) - or ``self.cluster_refresh`` (a
        ``refresh.ClusterRefresh``; opt-in): the sample set, the fit and the ``c*`` / ``edit*`` images then stay on the device
        (csrc/refresh.hip), with the same returned values and files.  ``self.frame_evaluator`` (an ``evaluation.FrameEvaluator``;
        opt-in): the two semantic maps come from one launch of csrc/eval.hip instead of the six torch expressions, and the metrics of
        a frame set registered with it are accumulated in that launch; the returned tuple and the files keep shapes and dtypes.
        ``self.frame_products`` (a ``frames.FrameProducts``; opt-in): the 8-bit rgb / albedo / shading / residual / entropy images, the
        16-bit disp / depth images, ``label``, ``vis_label``, ``vis_depth`` and ``vis_entropy`` are made on the device in one launch per
        frame (csrc/frame_vis.hip) and travel as bytes next to the float maps; the files are written from them and ``sems``,
        ``vis_deps``, ``vis_sems``, ``vis_entropys`` returned from them - ``vis_deps`` / ``vis_entropys`` then need no imgviz
        (``frames.depth2rgb``'s rule: jet over [near, far], and over the entropy map's own range)."""
        import os
        import numpy as np
        from . import frames
        H, W = int(self.H_scaled), int(self.W_scaled)
        try:
            from imgviz import depth2rgb
        except ImportError:
            depth2rgb = None
        lvl = "fine" if self.N_importance > 0 else "coarse"
        keys = [f"{k}_{lvl}" for k in ("rgb", "disp", "depth", "albedo", "shading", "residual")]
        if self.enable_semantic:
            keys += ["sem_label", "sem_entropy"]
        cmap = getattr(self, "valid_colour_map", None)
        if cmap is not None:      # the trainer keeps it on the GPU (trainer.py:262,449,588: valid_colour_map.cuda()); indexed on the host here
            cmap = cmap.detach().cpu().numpy() if isinstance(cmap, torch.Tensor) else np.asarray(cmap)
        if save_dir is not None:
            assert os.path.exists(save_dir)
        acc = {k: [] for k in ("rgb", "disp", "dep", "vis_dep", "albedo", "shading", "residual", "sem", "vis_sem", "ent", "vis_ent")}
        sample_pixels, sample_labels = [], []
        widths = None

        def finish(i, frame):
            m = frames.unpack_frame(frame, widths, keys, (H, W))
            img = products.images(i) if products is not None else None          # the frame's device-made planes
            acc["rgb"].append(m[f"rgb_{lvl}"]); acc["disp"].append(m[f"disp_{lvl}"]); acc["albedo"].append(m[f"albedo_{lvl}"])
            acc["shading"].append(m[f"shading_{lvl}"]); acc["residual"].append(m[f"residual_{lvl}"]); acc["dep"].append(m[f"depth_{lvl}"])
            if img is not None:
                acc["vis_dep"].append(img["vis_depth"])
            elif depth2rgb is not None:
                acc["vis_dep"].append(depth2rgb(acc["dep"][-1], min_value=self.near, max_value=self.far))
            if self.enable_semantic and img is not None:
                acc["sem"].append(img["label"]); acc["ent"].append(m["sem_entropy"])
                if cmap is not None:
                    acc["vis_sem"].append(img["vis_label"])
                acc["vis_ent"].append(img["vis_entropy"])
            elif self.enable_semantic:
                label = m["sem_label"].astype(np.uint8)
                acc["sem"].append(label); acc["ent"].append(m["sem_entropy"])
                if cmap is not None:
                    acc["vis_sem"].append(cmap[label.astype(np.int64)].astype(np.uint8))
                if depth2rgb is not None:
                    acc["vis_ent"].append(depth2rgb(acc["ent"][-1]))
            if update_cluster and not on_device:
                sample_pixels.append(acc["albedo"][-1][::2, ::2, :].reshape(-1, 3))
                sample_labels.append(acc["sem"][-1][::2, ::2].reshape(-1, 1))
            if save_dir is not None:
                w = lambda name, img: frames.write_png(os.path.join(save_dir, name.format(i)), img)
                if img is not None and getattr(products, "encode", False):      # the files were encoded on the device: same names, same set
                    for name, data in products.files(i).items():
                        with open(os.path.join(save_dir, "{}_{:03d}.png".format(name, i)), "wb") as fh:
                            fh.write(data)
                    return
                if img is not None:
                    for name in ("rgb", "albedo", "shading", "residual", "disp", "depth"):
                        w(name + "_{:03d}.png", img[name])
                else:
                    w("rgb_{:03d}.png", frames.to8b(acc["rgb"][-1])); w("albedo_{:03d}.png", frames.to8b(acc["albedo"][-1]))
                    w("shading_{:03d}.png", frames.to8b(acc["shading"][-1])); w("residual_{:03d}.png", frames.to8b(acc["residual"][-1]))
                    w("disp_{:03d}.png", acc["disp"][-1].astype(np.uint16)); w("depth_{:03d}.png", (acc["dep"][-1] * 1000).astype(np.uint16))
                if acc["vis_dep"]:
                    w("vis_depth_{:03d}.png", acc["vis_dep"][-1])
                if self.enable_semantic:
                    w("label_{:03d}.png", acc["sem"][-1]); w("entropy_{:03d}.png", img["entropy"] if img is not None else frames.to8b(acc["ent"][-1]))
                    if acc["vis_sem"]:
                        w("vis_label_{:03d}.png", acc["vis_sem"][-1])
                    if acc["vis_ent"]:
                        w("vis_entropy_{:03d}.png", acc["vis_ent"][-1])

        refresh = getattr(self, "cluster_refresh", None)
        on_device = bool(update_cluster) and refresh is not None
        class_num = (1 if getattr(self, "no_semantic_tree", False) else self.num_valid_semantic_class) if on_device else None
        streamer, in_flight = None, []
        evaluator = getattr(self, "frame_evaluator", None)
        if evaluator is not None:
            evaluator.begin(rays)
        products = getattr(self, "frame_products", None)
        for i in range(len(rays)):
            out = self.render_rays(rays[i])
            maps = {k: out[k].detach() for k in keys if k in out}
            if evaluator is not None:
                # one launch: both maps and, for a registered frame set, the confusion table and the depth / rgb sums
                label, entropy = evaluator.add_frame(i, logits=out[f"sem_logits_{lvl}"].detach() if self.enable_semantic else None,
                                                     depth=maps[f"depth_{lvl}"], rgb=maps[f"rgb_{lvl}"])
                if self.enable_semantic:
                    maps["sem_label"], maps["sem_entropy"] = label, entropy
            elif self.enable_semantic:
                logits = out[f"sem_logits_{lvl}"].detach()
                logp = F.log_softmax(logits, dim=-1)
                maps["sem_label"] = torch.argmax(F.softmax(logits, dim=-1), dim=-1).float()         # < 2^24: exact in fp32
                maps["sem_entropy"] = torch.sum(-logp * F.softmax(logits, dim=-1), dim=-1)
            pack, widths = frames.pack_maps(maps, keys)
            if on_device:
                if not pack.is_cuda:
                    raise RuntimeError(f"render_path with cluster_refresh: the rendered maps live on {pack.device}; the refresh pass runs "
                                       "only on a HIP device (no CPU / eager fallback exists)")
                if i == 0:
                    refresh.begin(len(rays), H, W, class_num, pack.device)
                refresh.add_frame(i, pack, widths, keys)
            if products is not None:
                if not pack.is_cuda:
                    raise RuntimeError(f"render_path with frame_products: the rendered maps live on {pack.device}; the frame images are "
                                       "made only on a HIP device (no CPU / eager fallback exists)")
                if i == 0:
                    plist = [(k, "to8b", f"{k}_{lvl}") for k in ("rgb", "albedo", "shading", "residual")]
                    plist += [("disp", "u16", f"disp_{lvl}", 1.0), ("depth", "u16", f"depth_{lvl}", 1000.0),      # trainer.py:1344-1345
                              ("vis_depth", "jet", f"depth_{lvl}", (float(self.near), float(self.far)))]            # trainer.py:1314
                    if self.enable_semantic:
                        plist += [("label", "u8_cast", "sem_label"), ("entropy", "to8b", "sem_entropy"),
                                  ("vis_entropy", "jet", "sem_entropy", None)]                                       # trainer.py:1321: its own range
                        if cmap is not None:
                            plist.append(("vis_label", "palette", "sem_label"))                                     # trainer.py:1269, 1294
                    products.begin(plist, keys, widths, (H, W), pack.device, palette=cmap)
                products.add_frame(i, pack)
            if pack.is_cuda:
                if streamer is None:
                    streamer = frames.FrameStreamer(pack.device)
                done = streamer.push(pack)
                in_flight.append(i)
                if done is not None:
                    finish(in_flight.pop(0), done)
            else:
                finish(i, pack.numpy())
        if streamer is not None:
            for frame in streamer.drain():
                finish(in_flight.pop(0), frame)
        if products is not None and getattr(products, "movies", None):
            products.close_movies()
        st = lambda name: np.stack(acc[name], 0) if acc[name] else None
        cluster_manager = None
        if on_device:
            # the sample table was filled frame by frame; the fit reads it where it is, and every kept pack becomes its two 8-bit images
            cluster_manager = refresh.finish(b_f, host=lambda i: (acc["albedo"][i], acc["sem"][i] if class_num > 1 else None,
                                                                  acc["shading"][i], acc["residual"][i]))
            if save_dir is not None:
                for i in range(len(acc["albedo"])):
                    c, edit = refresh.snap(i)
                    frames.write_png(os.path.join(save_dir, "c{:03d}.png".format(i)), c)
                    frames.write_png(os.path.join(save_dir, "edit{:03d}.png".format(i)), edit)
        elif update_cluster:
            factory = getattr(self, "cluster_manager_factory", None)
            if factory is None:
                raise NotImplementedError("render_path(update_cluster=True) fits mean-shift clusters (Cluster_Manager.update_center, "
                                          "SSR/training/cluster.py:101-182); set self.cluster_manager_factory to that class")
            cluster_manager = factory(class_num=1 if getattr(self, "no_semantic_tree", False) else self.num_valid_semantic_class)
            cluster_manager.update_center(np.stack(sample_labels, 0), np.stack(sample_pixels, 0), band_factor=b_f)
            # trainer.py:1425-1440: every rendered albedo snapped to its cluster centres (c*.png) and the image re-composed from
            # the clustered albedo (edit*.png); manager.dest_color is the reference's method (cluster.dest_color: the HIP lookup)
            dev = rays[0].device if isinstance(rays[0], torch.Tensor) else torch.device("cpu")
            for i, albedo in enumerate(acc["albedo"]):
                pixel = torch.from_numpy(albedo).reshape(-1, 3).to(dev)
                label = torch.from_numpy(acc["sem"][i]).reshape(-1, 1).to(dev)
                result = cluster_manager.dest_color(pixel, label).reshape(albedo.shape).cpu().numpy()
                if save_dir is not None:
                    frames.write_png(os.path.join(save_dir, "c{:03d}.png".format(i)), frames.to8b(result))
                    edit = (result.reshape(-1, 3) * acc["shading"][i].reshape(-1, 1) + acc["residual"][i].reshape(-1, 3)).reshape(result.shape)
                    frames.write_png(os.path.join(save_dir, "edit{:03d}.png".format(i)), frames.to8b(edit))
        return (st("rgb"), st("disp"), st("dep"), st("vis_dep"), st("sem"), st("vis_sem"), st("ent"), st("vis_ent"),
                st("albedo"), st("shading"), st("residual"), cluster_manager)

    def occupancy_grid(self, extents, transform, grid_dim=256, occ_range=(-1., 1.)):
        """``occ[grid_dim, grid_dim, grid_dim]`` (device) of the fine network on the lattice inside the scene's oriented bounding box -
        extract_colour_mesh.py:149-185 up to the array handed to marching cubes: ``extents`` / ``transform`` as
        trimesh.bounds.oriented_bounds gives them (transform = the inverse of its to-origin matrix), voxel size
        ``(far - near) / N_importance`` (:178).  One ``inerf_occupancy_grid`` launch (geometry.occupancy_grid)."""
        from . import geometry
        return geometry.occupancy_grid(self.ssr_net_fine, self.embed_fn, occ_range, extents, transform, grid_dim,
                                       (self.far - self.near) / self.N_importance, embeddirs_fn=self.embeddirs_fn)

    def vertex_colours(self, vertices, normals, near_t=2.0, sem=False, colour_map=None, chunk=None):
        """``uint8 [V, 3]`` (numpy) colours of the mesh vertices - extract_colour_mesh.py:232-257: one ray per vertex against its normal
        (near 0.1, far 10.0 as :233-234 hard-code them, ``near_t`` = args.near_t), rendered in eval mode, then ``to8b(rgb_fine)`` or, with
        ``sem``, ``colour_map[label]`` (default: ``self.valid_colour_map``).  geometry.vertex_colours on ``self.render_rays`` with
        ``return_raw`` and ``check_numerics`` off for the pass: rays, render and colours stay on the device, three bytes per vertex
        are copied to the host, once.  The trainer must be in eval mode (the reference sets ``training = False`` first, :129)."""
        from . import geometry
        if bool(self.training):
            raise RuntimeError("vertex_colours renders in eval mode: set training = False first (extract_colour_mesh.py:129)")
        if colour_map is None:
            colour_map = getattr(self, "valid_colour_map", None)
        saved = self.return_raw, self.check_numerics
        self.return_raw = self.check_numerics = False
        try:
            return geometry.vertex_colours(self.render_rays, vertices, normals, near=0.1, far=10.0, near_t=near_t, sem=sem,
                                           colour_map=colour_map if sem else None, chunk=chunk)
        finally:
            self.return_raw, self.check_numerics = saved

    def extract_colour_mesh(self, extents, transform, grid_dim=256, level=0.45, near_t=2.0, sem=False, colour_map=None, save_path=None,
                            min_num_cluster=400, keep_single_cluster=False, occ_range=(-1., 1.)):
        """extract_colour_mesh.py:149-266 in one call: the occupancy of the fine network on the lattice of the oriented bounding box,
        marching cubes at ``level`` (0.45 as :134), scene coordinates, vertex normals, ``clean_mesh`` (geometry.extract_mesh: all on the
        device), then ``vertex_colours`` and, with ``save_path``, the coloured PLY (geometry.write_ply).  Returns ``(vertices float64
        [V, 3], faces int32 [F, 3], normals float64 [V, 3]`` - device tensors - ``, colours uint8 [V, 3]`` - numpy``)``."""
        from . import geometry
        vertices, faces, normals = geometry.extract_mesh(self.ssr_net_fine, self.embed_fn, extents, transform, grid_dim,
                                                         (self.far - self.near) / self.N_importance, level, occ_range=occ_range,
                                                         min_num_cluster=min_num_cluster, keep_single_cluster=keep_single_cluster,
                                                         embeddirs_fn=self.embeddirs_fn)
        colours = self.vertex_colours(vertices, normals, near_t=near_t, sem=sem, colour_map=colour_map)
        if save_path is not None:
            geometry.write_ply(save_path, vertices, faces, colours=colours, normals=normals)
        return vertices, faces, normals, colours

    def _coalesced(self, flat_rays):
        """``self.chunk``, or the larger number of rays per ``volumetric_rendering`` call that gives the same frame
        (kernels.coalesced_chunk; results are bit-identical for any chunking): only when no random number is drawn per chunk (eval
        mode, or ``perturb == 0`` and ``raw_noise_std == 0``), ``raw_*`` is not returned, nothing records autograd and both networks
        take the fused kernels."""
        training = bool(self.training)
        if (self.return_raw or (training and (self.perturb > 0. or self.raw_noise_std > 0.)) or not flat_rays.is_cuda
                or flat_rays.shape[-1] <= 8 or flat_rays.shape[0] <= self.chunk or _wants_grad(self.ssr_net_coarse, self.ssr_net_fine)):
            return None
        if _fusable(self.ssr_net_coarse, self.embed_fn, self.embeddirs_fn) is None or (
                self.N_importance > 0 and _fusable(self.ssr_net_fine, self.embed_fn, self.embeddirs_fn) is None):
            return None
        c = int(self.num_valid_semantic_class) if self.enable_semantic else 0
        channels = _capi.BASE_CHANNELS + c + (_capi.ENDPOINT_DIM if (self.endpoint_feat and self.N_importance > 0) else 0)
        return kernels.coalesced_chunk(flat_rays.shape[0], self.chunk, self.N_samples, self.N_importance, channels, flat_rays.device)

    def volumetric_rendering(self, ray_batch, ray_base=None):
        """trainer.py:717-808 for one ray batch.  With ``self.draws``: ``ray_base`` is the global index of the batch's first ray (given
        by render_rays' chunk loop, which advances the step); None: this call is the whole batch (base 0) and advances the step itself."""
        ray_batch = ray_batch.float()
        n, dev = ray_batch.shape[0], ray_batch.device
        draws, base = self.draws, 0 if ray_base is None else int(ray_base)
        if ray_batch.shape[-1] <= 8:
            raise NotImplementedError("volumetric_rendering needs view directions (use_viewdirs: true in every config)")
        desc = _fusable(self.ssr_net_coarse, self.embed_fn, self.embeddirs_fn)
        if desc is not None and self.N_importance > 0 and _fusable(self.ssr_net_fine, self.embed_fn, self.embeddirs_fn) is None:
            desc = None
        if desc is None:
            # The reference builds whatever netdepth / netwidth the YAML says (trainer.py:811-846) and calls it
            # (model_utils.py:19-35).  Outside the fused kernels' architecture (D=8, W=256, skips=[4], multires<=10,
            # multires_views<=4) the path runs STAGED, like object_level.render_rays does for a user-supplied network:
            # sampling and compositing on the HIP kernels (with their HIP backward), the networks through their own forward.
            _unfused_notice("volumetric_rendering")
        training = bool(self.training)
        t_vals = torch.linspace(0., 1., steps=self.N_samples, device=dev)
        # RNG draws in the reference's order: t_rand (:744), coarse noise (model_utils.py:70), u (rays.py:197), fine noise
        std = self.raw_noise_std if training else 0
        drawn_perturb = draws is not None and self.perturb > 0. and training
        drawn_noise = draws is not None and std > 0.
        t_rand = torch.rand(n, self.N_samples, device=dev) if (self.perturb > 0. and training and not drawn_perturb) else None
        noise_c = torch.randn(n, self.N_samples, device=dev) * std if (std > 0. and not drawn_noise) else None
        u = noise_f = None
        if self.N_importance > 0:
            det = (self.perturb == 0.) or (not training)
            if not drawn_perturb:
                u = (torch.linspace(0., 1., steps=self.N_importance, device=dev) if det
                     else torch.rand(n, self.N_importance, device=dev))
            noise_f = torch.randn(n, self.N_samples + self.N_importance, device=dev) * std if (std > 0. and not drawn_noise) else None
        ep = bool(self.endpoint_feat) and self.N_importance > 0
        # the drawn forms: (jitter / u, coarse noise, fine noise) for the staged path, one inerf_draw_args for the fused one
        dr = None
        if drawn_perturb or drawn_noise:
            dr = {"perturb": draws.args(base) if drawn_perturb else None,
                  "noise_c": draws.args(base, std) if drawn_noise else None,
                  "noise_f": draws.args(base, std, fine=True) if drawn_noise else None,
                  "fused": draws.args(base, std if drawn_noise else 0., perturb=drawn_perturb)}

        train_desc = None
        if desc is not None and _wants_grad(self.ssr_net_coarse, self.ssr_net_fine):
            _training_path_notice("volumetric_rendering")
            train_desc, desc = _train_desc(desc), None
        if desc is not None:
            o = render_core.render_fused(desc, self.ssr_net_coarse, self.ssr_net_fine, "volumetric_rendering", ray_batch, self.N_samples,
                                         self.N_importance, t_vals, u, t_rand, noise_c, noise_f, white_bkgd=self.white_bkgd, endpoint=ep,
                                         want_raw_coarse=self.return_raw, want_raw_fine=self.return_raw,
                                         want_sem=bool(self.enable_semantic), draw=None if dr is None else dr["fused"])
        else:       # stage by stage (render_core.staged_pass); a training step reads both networks' f16 range words once
            foreign = lambda pts, viewdirs, fn, endpoint: run_network(pts, viewdirs, fn, self.embed_fn, self.embeddirs_fn, self.netchunk,
                                                                      show_endpoint=endpoint)
            o = render_core.training_step(
                lambda td: render_core.staged_pass(ray_batch, t_vals, (t_rand, noise_c, u, noise_f), dr,
                                                   (self.ssr_net_coarse, self.ssr_net_fine),
                                                   render_core.make_query(td, ray_batch, (self.embed_fn, self.embeddirs_fn), foreign),
                                                   self.N_importance, self.white_bkgd,
                                                   n_classes=self.num_valid_semantic_class if self.enable_semantic else 0, endpoint=ep),
                train_desc, "volumetric_rendering")
        ret = {}
        if self.return_raw:
            ret["raw_coarse"] = o["raw_coarse"]
        for k in ("rgb", "disp", "acc", "depth", "albedo", "shading", "residual"):
            ret[k + "_coarse"] = o[k + "_coarse"]
        if self.enable_semantic:
            ret["sem_logits_coarse"] = o["sem_coarse"]
        if self.N_importance > 0:
            for k in ("rgb", "disp", "acc", "depth", "albedo", "shading", "residual"):
                ret[k + "_fine"] = o[k + "_fine"]
            if self.enable_semantic:
                ret["sem_logits_fine"] = o["sem_fine"]
            ret["z_std"] = o["z_std"]
            if self.return_raw:
                ret["raw_fine"] = o["raw_fine"]
            if ep:
                ret["feat_map_fine"] = o["feat_fine"]
        if self.check_numerics:
            render_core.report_non_finite(ret)
        if dr is not None and ray_base is None:
            draws.advance()
        return ret

    def sample_data(self, step, rays, h, w, no_batching=True, mode="train"):
        """``SSRTrainer.sample_data`` (trainer.py:627-691).  With ``no_batching`` the draws are the reference's own
        ``sampling_index`` (a seeded run selects the reference's pixels) and every gather is ONE launch of
        ``inerf_batch_assemble``; returns the reference's 5-tuple (2-tuple without ``enable_semantic``), the availability flag
        being ``mask_ids[index_batch]`` as the reference forms it.  ``no_batching=False`` keeps the reference's torch lines.
        A holder that is not the reference's trainer may carry its own draw function as the INSTANCE attribute ``sampling_index``
        (same signature; set on a class it would have to be a ``staticmethod``)."""
        num_img, num_ray, ray_dim = rays.shape
        assert num_ray == h * w
        total_ray_num = num_img * h * w
        if mode == "train":
            image, sample_num = self.train_image, self.num_train
            depth, semantic = (self.train_depth, self.train_semantic) if self.enable_semantic else (None, None)
        elif mode == "test":
            image, sample_num = self.test_image, self.num_test
            depth, semantic = (self.test_depth, self.test_semantic) if self.enable_semantic else (None, None)
        else:
            assert False
        sematic_available_flag = 1
        if no_batching:
            draw = getattr(self, "sampling_index", None)
            if draw is None:
                import sys
                mod = sys.modules.get("SSR.models.rays")
                if mod is None:
                    raise RuntimeError("sample_data draws with the reference's sampling_index: import SSR.models.rays (the launcher "
                                       "does) or set `sampling_index` on the trainer")
                draw = mod.sampling_index
            index_batch, index_hw = draw(self.n_rays, num_img, h, w)
            # [1, 2n]: the n drawn pixels, then their clamped neighbours.  The kernel takes the pixel and the two offsets and clamps
            # itself; after the clamp the offsets are what is left of the reference's bias_h / bias_w, so the rows are the same.
            n = index_hw.shape[1] // 2
            sel, nei = index_hw[0, :n], index_hw[0, n:]
            packed = torch.stack([sel, torch.div(nei, w, rounding_mode="floor") - torch.div(sel, w, rounding_mode="floor"),
                                  nei % w - sel % w]).to(device=rays.device, dtype=torch.int64)          # one upload
            image_index = int(np.asarray(index_batch).reshape(-1)[0])
            out = kernels.batch_ssr(image.reshape(sample_num, h, w, 3), None if depth is None else depth.reshape(sample_num, h, w),
                                    None if semantic is None else semantic.reshape(sample_num, h, w), n, rays=rays,
                                    indices=(image_index, packed[0], packed[1], packed[2]))
            flat_sampled_rays, gt_image, gt_depth, gt_semantic = out[:4]
            if self.enable_semantic:
                sematic_available_flag = self.mask_ids[index_batch]
        else:
            index_hw = self.rand_idx[self.i_batch:self.i_batch + self.n_rays]
            flat_sampled_rays = rays.reshape([-1, ray_dim]).float()[index_hw, :]
            gt_image = image.reshape(-1, 3)[index_hw, :]
            if self.enable_semantic:
                gt_depth = depth.reshape(-1)[index_hw]
                gt_semantic = semantic.reshape(-1)[index_hw].cuda()
            self.i_batch += self.n_rays
            if self.i_batch >= total_ray_num:
                print("Shuffle data after an epoch!")
                self.rand_idx = torch.randperm(total_ray_num)
                self.i_batch = 0
        if self.enable_semantic:
            return flat_sampled_rays, gt_image, gt_depth, gt_semantic.long(), sematic_available_flag
        return flat_sampled_rays, gt_image

    def create_ssr(self):
        """Build coarse + fine Semantic_NeRF and the encoders - trainer.py:811-846 (optimiser included)."""
        r, m = self.config["render"], self.config["model"]
        embed_fn, input_ch = get_embedder(r["multires"], r["i_embed"], scalar_factor=10)
        embeddirs_fn, input_ch_views = (get_embedder(r["multires_views"], r["i_embed"], scalar_factor=1)
                                        if r["use_viewdirs"] else (None, 0))
        output_ch = 5 if self.N_importance > 0 else 4
        mk = lambda d, w: Semantic_NeRF(enable_semantic=self.enable_semantic,
                                        num_semantic_classes=self.num_valid_semantic_class, D=d, W=w, input_ch=input_ch,
                                        output_ch=output_ch, skips=[4], input_ch_views=input_ch_views,
                                        use_viewdirs=r["use_viewdirs"]).cuda()
        model = mk(m["netdepth"], m["netwidth"])
        grad_vars = list(model.parameters())
        model_fine = None
        if self.N_importance > 0:
            model_fine = mk(m["netdepth_fine"], m["netwidth_fine"])
            grad_vars += list(model_fine.parameters())
        self.ssr_net_coarse, self.ssr_net_fine = model, model_fine
        self.embed_fn, self.embeddirs_fn = embed_fn, embeddirs_fn
        self.optimizer = torch.optim.Adam(params=grad_vars, lr=getattr(self, "lrate", 5e-4))


class SSRRenderer(SSRRenderMixin):
    """Stand-alone holder of the attributes the mixin reads (for rendering without the trainer)."""

    def __init__(self, num_classes, N_samples=64, N_importance=128, multires=10, multires_views=4, white_bkgd=False,
                 enable_semantic=True, endpoint_feat=False, chunk=1024 * 32, netchunk=1024 * 32, perturb=1.,
                 raw_noise_std=1., device="cuda"):
        self.N_samples, self.N_importance = N_samples, N_importance
        self.perturb, self.raw_noise_std, self.white_bkgd = perturb, raw_noise_std, white_bkgd
        self.enable_semantic, self.num_valid_semantic_class = enable_semantic, num_classes
        self.endpoint_feat, self.chunk, self.netchunk = endpoint_feat, chunk, netchunk
        self.training = False
        self.embed_fn, ch = get_embedder(multires, 0, scalar_factor=10)
        self.embeddirs_fn, chv = get_embedder(multires_views, 0, scalar_factor=1)
        mk = lambda: Semantic_NeRF(enable_semantic, num_classes, D=8, W=256, input_ch=ch, output_ch=5, skips=[4],
                                   input_ch_views=chv, use_viewdirs=True).to(device)
        self.ssr_net_coarse = mk()
        self.ssr_net_fine = mk() if N_importance > 0 else None
