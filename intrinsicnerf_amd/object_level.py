"""Drop-in front-end for the object-level code base (``object_level/run_nerf.py`` + ``run_nerf_helpers.py``).

Same function names, argument meaning, return structure and error behaviour as the reference, so
that ``run_nerf.py`` keeps working when it imports these instead of its own definitions
(INTEGRATION.md).  The arithmetic is done by ``libinerf.so`` (hand-written HIP for gfx950); this
file is plumbing: shape handling, RNG draws in the reference's order, dict assembly.  The control
path it shares with ``ssr.py`` - fusability, the chunk loop with its f16 range fallback, the staged
pass of a training step - is ``render_core.py``.

Reference lines (relative to ``/root/reference/object_level``):
  render          run_nerf.py:74-139        batchify_rays   run_nerf.py:59-71
  render_rays     run_nerf.py:415-528       run_network     run_nerf.py:42-56
  raw2outputs     run_nerf.py:359-412       sample_pdf      run_nerf_helpers.py:402-445
  NeRF            run_nerf_helpers.py:247   get_embedder    run_nerf_helpers.py:228-243
  get_rays        run_nerf_helpers.py:359   ndc_rays        run_nerf_helpers.py:381-399
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _capi, kernels, render_core
from .render_core import (FP32_LAYERS_NOTE, _fusable, _layered_spec, _run_network_torch, _train_desc, _train_query,  # noqa: F401
                          _training_path_notice, _unfused_notice, _wants_grad)       # (they live in render_core.py; importable from here as before)
from .losses import compute_intrinsic_loss, object_step_loss  # noqa: F401  (run_nerf_helpers.py:59-86, run_nerf.py:976-1013 on csrc/losses.hip)

__all__ = ["Embedder", "get_embedder", "NeRF", "NetworkQuery", "run_network", "raw2outputs", "sample_pdf",
           "render_rays", "batchify_rays", "render", "render_path", "get_rays", "get_rays_np", "ndc_rays", "create_nerf", "to8b",
           "compute_intrinsic_loss", "object_step_loss"]


# ----------------------------------------------------------------------------------------------
# encoder + model (host-side mirrors; the hot path reads only their hyper-parameters and weights)
# ----------------------------------------------------------------------------------------------
class Embedder:
    """Frequency encoder description (run_nerf_helpers.py:195-225).

    In the fused path only ``n_freqs`` / ``scalar_factor`` are read - the encoding itself happens
    inside the MLP kernel.  Calling the object evaluates the same encoding with torch ops (used by
    code that wants the embedding itself, e.g. a user-supplied network).
    """

    def __init__(self, n_freqs, input_dims=3, scalar_factor=1.0):
        self.n_freqs = int(n_freqs)
        self.input_dims = input_dims
        self.scalar_factor = float(scalar_factor)
        self.out_dim = input_dims * (1 + 2 * self.n_freqs)

    def __call__(self, x):
        if self.scalar_factor != 1.0:
            x = x / self.scalar_factor
        bands = [x]
        for k in range(self.n_freqs):
            bands += [torch.sin(x * float(2 ** k)), torch.cos(x * float(2 ** k))]
        return torch.cat(bands, -1)

    embed = __call__


def get_embedder(multires, i=0):
    """(embed_fn, out_dim) - run_nerf_helpers.py:228-243.  ``i == -1`` means no encoding."""
    if i == -1:
        return nn.Identity(), 3
    e = Embedder(multires)
    return e, e.out_dim


class NeRF(nn.Module):
    """Intrinsic NeRF MLP with the reference's parameter names and shapes (run_nerf_helpers.py:247-325).

    ``pts_linears.0-7``, ``views_linears.0``, ``feature_linear``, ``alpha_linear``, ``shading_linear``
    (the RESIDUAL head), ``albedo_linear1/2``, ``test_linear1/2`` (the SHADING head): checkpoints
    written by the reference load unchanged.  ``forward`` is the definition of the network in torch
    ops for callers that hold an already-embedded tensor; ``render_rays`` / ``run_network`` never call
    it - they hand the module's weights to the fused HIP kernel.
    """

    def __init__(self, D=8, W=256, input_ch=3, input_ch_views=3, output_ch=4, skips=[4], use_viewdirs=False):
        super().__init__()
        self.D, self.W = D, W
        self.input_ch, self.input_ch_views = input_ch, input_ch_views
        self.skips = list(skips)
        self.use_viewdirs = use_viewdirs
        self.pts_linears = nn.ModuleList(
            [nn.Linear(input_ch, W)] +
            [nn.Linear(W + input_ch, W) if i in self.skips else nn.Linear(W, W) for i in range(D - 1)])
        self.views_linears = nn.ModuleList([nn.Linear(input_ch_views + W, W // 2)])
        if use_viewdirs:
            self.feature_linear = nn.Linear(W, W)
            self.alpha_linear = nn.Linear(W, 1)
            self.shading_linear = nn.Linear(W // 2, 3)
            self.albedo_linear1 = nn.Linear(W, W // 2)
            self.albedo_linear2 = nn.Linear(W // 2, 3)
            self.test_linear1 = nn.Linear(W, W // 2)
            self.test_linear2 = nn.Linear(W // 2, 1)
        else:
            self.output_linear = nn.Linear(W, output_ch)

    def fused_desc(self):
        """C-ABI description if the fused kernel supports this architecture, else None."""
        if not (self.use_viewdirs and self.D == 8 and self.W == 256 and self.skips == [4]):
            return None
        l_xyz, rx = divmod(self.input_ch - 3, 6)
        l_dir, rd = divmod(self.input_ch_views - 3, 6)
        if rx or rd or not (0 <= l_xyz <= 10 and 0 <= l_dir <= 4):
            return None
        return _capi.net_desc(_capi.VARIANT_OBJECT, 0, l_xyz, l_dir, 1.0)

    def forward(self, x):
        pts, views = torch.split(x, [self.input_ch, self.input_ch_views], dim=-1)
        h = pts
        for i, layer in enumerate(self.pts_linears):
            h = F.relu(layer(h))
            if i in self.skips:
                h = torch.cat([pts, h], -1)
        if not self.use_viewdirs:
            return self.output_linear(h)
        sigma = self.alpha_linear(h)
        albedo = torch.sigmoid(self.albedo_linear2(F.relu(self.albedo_linear1(h))))
        shading = torch.sigmoid(self.test_linear2(F.relu(self.test_linear1(h))))
        v = torch.cat([self.feature_linear(h), views], -1)
        for layer in self.views_linears:
            v = F.relu(layer(v))
        residual = torch.sigmoid(self.shading_linear(v))
        rgb = albedo * shading + residual
        return torch.cat([rgb, sigma, albedo, shading, residual], -1)


class NetworkQuery:
    """The ``network_query_fn`` closure of create_nerf (run_nerf.py:298-301) as an inspectable object."""

    def __init__(self, embed_fn, embeddirs_fn, netchunk=1024 * 64):
        self.embed_fn, self.embeddirs_fn, self.netchunk = embed_fn, embeddirs_fn, netchunk

    def __call__(self, inputs, viewdirs, network_fn):
        return run_network(inputs, viewdirs, network_fn, self.embed_fn, self.embeddirs_fn, self.netchunk)


def _as_network_query(q):
    """``q`` as a NetworkQuery if it is one - or if it is, structurally, the closure the reference's create_nerf builds
    (run_nerf.py:298-301):

        lambda inputs, viewdirs, network_fn: run_network(inputs, viewdirs, network_fn, embed_fn=embed_fn,
                                                         embeddirs_fn=embeddirs_fn, netchunk=args.netchunk)

    i.e. a 3-argument function whose only global is THIS package's ``run_network`` and whose closure holds ``embed_fn``
    and ``embeddirs_fn``.  A run_nerf.py that merely imports this module's symbols therefore takes the fused path with
    its create_nerf untouched.  Anything else returns None and is called as given (the staged path)."""
    if isinstance(q, NetworkQuery):
        return q
    code, cells, glob = getattr(q, "__code__", None), getattr(q, "__closure__", None), getattr(q, "__globals__", None)
    if code is None or cells is None or glob is None or code.co_argcount != 3 or code.co_kwonlyargcount:
        return None
    if not set(code.co_names) <= {"run_network", "netchunk"} or "run_network" not in code.co_names:
        return None
    target = glob.get("run_network")
    if target is None or getattr(target, "__module__", "").split(".")[0] != __name__.split(".")[0] or target.__name__ != "run_network":
        return None
    free = dict(zip(code.co_freevars, cells))
    try:
        embed_fn, embeddirs_fn = free["embed_fn"].cell_contents, free["embeddirs_fn"].cell_contents
    except (KeyError, ValueError):
        return None
    if not isinstance(embed_fn, Embedder) or not isinstance(embeddirs_fn, Embedder):
        return None
    return NetworkQuery(embed_fn, embeddirs_fn)


def run_network(inputs, viewdirs, fn, embed_fn, embeddirs_fn, netchunk=1024 * 64):
    """Encode ``inputs[..., 3]`` (+ ``viewdirs[N, 3]``) and apply network ``fn`` - run_nerf.py:42-56.

    With this package's NeRF + Embedder the whole thing is one fused HIP launch (``netchunk`` only
    bounded the reference's activation memory and does not affect results).  Any other ``fn`` is
    called like the reference does, on the torch-evaluated embedding.
    """
    return render_core.run_network(inputs, viewdirs, fn, embed_fn, embeddirs_fn, netchunk, endpoint=False)


def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=False, pytest=False):
    """Alpha compositing - run_nerf.py:359-412.

    Returns ``(rgb_map, disp_map, acc_map, weights, depth_map, albedo_map, shading_map, residual_map)``.
    """
    noise = None
    if raw_noise_std > 0.:
        noise = torch.randn(raw[..., 3].shape, device=raw.device) * raw_noise_std
        if pytest:
            np.random.seed(0)
            noise = torch.Tensor(np.random.rand(*list(raw[..., 3].shape)) * raw_noise_std).to(raw.device)
    o = kernels.composite(raw.float(), z_vals.float(), rays_d.float(), noise, white_bkgd)
    return o["rgb"], o["disp"], o["acc"], o["weights"], o["depth"], o["albedo"], o["shading"], o["residual"]


def _draw_u(n_rays, n_samples, det, pytest, device):
    """The ``u`` of sample_pdf (run_nerf_helpers.py:409-425): shared linspace when deterministic."""
    if pytest:
        np.random.seed(0)
        if det:
            return torch.Tensor(np.linspace(0., 1., n_samples)).to(device)
        return torch.Tensor(np.random.rand(n_rays, n_samples)).to(device)
    if det:
        return torch.linspace(0., 1., steps=n_samples, device=device)
    return torch.rand(n_rays, n_samples, device=device)


def sample_pdf(bins, weights, N_samples, det=False, pytest=False):
    """Hierarchical sampling - run_nerf_helpers.py:402-445.  ``bins[N,B]``, ``weights[N,B-1]`` -> ``[N,N_samples]``."""
    lead = bins.shape[:-1]
    b2 = torch.reshape(bins, [-1, bins.shape[-1]]).float()
    w2 = torch.reshape(weights, [-1, weights.shape[-1]]).float()
    u = _draw_u(b2.shape[0], N_samples, det, pytest, bins.device)
    return torch.reshape(kernels.sample_pdf(b2, w2, u, N_samples), list(lead) + [N_samples])


_RET_MAP = (("rgb_map", "rgb"), ("disp_map", "disp"), ("acc_map", "acc"), ("albedo_map", "albedo"),
            ("shading_map", "shading"), ("residual_map", "residual"))
_RET_0 = (("rgb0", "rgb"), ("disp0", "disp"), ("acc0", "acc"), ("albedo0", "albedo"), ("shading0", "shading"),
          ("residual0", "residual"))


def render_rays(ray_batch, network_fn, network_query_fn, N_samples, retraw=False, lindisp=False, perturb=0.,
                N_importance=0, network_fine=None, white_bkgd=False, raw_noise_std=0., verbose=False, pytest=False, draws=None,
                ray_base=None):
    """Volumetric rendering of one ray batch - run_nerf.py:415-528 (same dict keys, same RNG draw order).

    ``draws`` (a ``draws.DrawState``; default None = torch's generator, as before): whatever the reference draws - the jitter and the
    per-ray u when ``perturb > 0``, the density noise when ``raw_noise_std > 0`` - is drawn inside the kernels as a function of
    (seed, step, stream, ``ray_base`` + ray, sample), so the result does not depend on how the rays were chunked.  ``ray_base``: global
    index of this batch's first ray - given by a chunk loop, which then also advances the step; None: this call is the whole
    batch (base 0) and advances the step itself.  A call that draws nothing (``perturb == 0`` and ``raw_noise_std == 0``) leaves the step
    alone: the step counts drawing renders, so eval renders between training steps do not shift the training draws."""
    ray_batch = ray_batch.float()
    n = ray_batch.shape[0]
    dev = ray_batch.device
    if draws is not None and pytest:
        raise ValueError("render_rays: pytest=True replaces the random tensors by numpy's; it cannot be combined with draws")
    drawn_perturb = draws is not None and perturb > 0.
    drawn_noise = draws is not None and raw_noise_std > 0.
    base = 0 if ray_base is None else int(ray_base)
    if ray_batch.shape[-1] <= 8:
        raise NotImplementedError("render_rays without view directions: the 11-channel intrinsic network needs "
                                  "use_viewdirs=True (run_nerf_helpers.py:281-282 is unused by every config)")
    desc = None
    nq = _as_network_query(network_query_fn)
    if nq is not None:
        desc = _fusable(network_fn, nq.embed_fn, nq.embeddirs_fn)
        if desc is not None and network_fine is not None and _fusable(network_fine, nq.embed_fn, nq.embeddirs_fn) is None:
            desc = None
    # random inputs, drawn in the reference's order: t_rand (:478), coarse noise (:387), u (helpers:414), fine noise
    t_vals = torch.linspace(0., 1., steps=N_samples, device=dev)
    t_rand = None
    if perturb > 0. and not drawn_perturb:
        t_rand = torch.rand(n, N_samples, device=dev)
        if pytest:
            np.random.seed(0)
            t_rand = torch.Tensor(np.random.rand(n, N_samples)).to(dev)

    def noise(s):
        if not raw_noise_std > 0. or drawn_noise:
            return None
        nz = torch.randn(n, s, device=dev) * raw_noise_std
        if pytest:
            np.random.seed(0)
            nz = torch.Tensor(np.random.rand(n, s) * raw_noise_std).to(dev)
        return nz

    noise_c = noise(N_samples)
    u = _draw_u(n, N_importance, perturb == 0., pytest, dev) if (N_importance > 0 and not drawn_perturb) else None
    noise_f = noise(N_samples + N_importance) if N_importance > 0 else None
    fine_net = network_fine if network_fine is not None else network_fn
    train_desc = None
    if desc is not None and _wants_grad(network_fn, network_fine):
        _training_path_notice("render_rays")
        train_desc, desc = _train_desc(desc), None
    if desc is not None:
        draw = draws.args(base, raw_noise_std if drawn_noise else 0., perturb=True if drawn_perturb else False) if (
            drawn_perturb or drawn_noise) else None
        o = render_core.render_fused(desc, network_fn, fine_net, "render_rays", ray_batch, N_samples, N_importance, t_vals, u, t_rand,
                                     noise_c, noise_f, white_bkgd=white_bkgd, lindisp=lindisp,
                                     want_raw_coarse=retraw and N_importance == 0, want_raw_fine=retraw, draw=draw)
    else:
        # a network outside the fused architecture, a user-supplied one, or a training step: the stages run on the HIP kernels
        # (compositing differentiably); the network through kernels.mlp_train, the fp32 layer kernels (layered.py) or - a foreign
        # callable or query function - as the reference calls it
        dr = {"perturb": draws.args(base) if drawn_perturb else None,
              "noise_c": draws.args(base, raw_noise_std) if drawn_noise else None,
              "noise_f": draws.args(base, raw_noise_std, fine=True) if drawn_noise else None}
        encoders = (nq.embed_fn, nq.embeddirs_fn) if nq is not None else None
        foreign = lambda pts, viewdirs, fn, endpoint: network_query_fn(pts, viewdirs, fn)
        o = render_core.training_step(
            lambda td: render_core.staged_pass(ray_batch, t_vals, (t_rand, noise_c, u, noise_f), dr, (network_fn, fine_net),
                                               render_core.make_query(td, ray_batch, encoders, foreign), N_importance, white_bkgd,
                                               lindisp),
            train_desc, "render_rays")
    lvl = "fine" if N_importance > 0 else "coarse"
    ret = {rk: o[f"{ok}_{lvl}"] for rk, ok in _RET_MAP}
    if retraw:
        ret["raw"] = o["raw_" + lvl]
    if N_importance > 0:
        for rk, ok in _RET_0:
            ret[rk] = o[ok + "_coarse"]
        ret["z_std"] = o["z_std"]
    if verbose:       # the reference's DEBUG nan/inf scan (run_nerf.py:524-526)
        render_core.report_non_finite(ret)
    if (drawn_perturb or drawn_noise) and ray_base is None:      # the whole batch was this one call: the next call draws at the next step
        draws.advance()
    return ret


def _coalesced(rays_flat, chunk, kwargs):
    """``chunk``, or the larger number of rays per ``render_rays`` call that gives the same result (kernels.coalesced_chunk): only for
    eval-mode calls of the fused path - no random draw (``perturb == 0``, ``raw_noise_std == 0``), no ``retraw``, no autograd."""
    if (kwargs.get("retraw") or kwargs.get("perturb", 0.) > 0. or kwargs.get("raw_noise_std", 0.) > 0. or kwargs.get("verbose")
            or not rays_flat.is_cuda or rays_flat.shape[-1] <= 8 or rays_flat.shape[0] <= chunk):
        return chunk
    net, fine = kwargs.get("network_fn"), kwargs.get("network_fine")
    nq = _as_network_query(kwargs.get("network_query_fn"))
    if nq is None or _fusable(net, nq.embed_fn, nq.embeddirs_fn) is None or _wants_grad(net, fine):
        return chunk
    if fine is not None and _fusable(fine, nq.embed_fn, nq.embeddirs_fn) is None:
        return chunk
    return kernels.coalesced_chunk(rays_flat.shape[0], chunk, kwargs.get("N_samples", 0), kwargs.get("N_importance", 0),
                                   _capi.BASE_CHANNELS, rays_flat.device)


def batchify_rays(rays_flat, chunk=1024 * 32, **kwargs):
    """Render rays in chunks - run_nerf.py:59-71.  Results do not depend on ``chunk`` - so eval-mode frames of the fused path
    are rendered in FEWER, larger launches than ``chunk`` asks for (``_coalesced``; ``INERF_COALESCE_BYTES=0`` keeps the caller's).

    The loop is render_core.render_chunks: the f16 range words are read ONCE per call, and the chunks that left the range - and
    only those - are rendered again with the exact fp32 kernel.  With ``draws`` every chunk draws at the same step with its first
    global ray index as base; the step advances once, after the last chunk (render_core.advance_after)."""
    draws = kwargs.get("draws")
    if draws is not None and (kwargs.get("perturb", 0.) > 0. or kwargs.get("raw_noise_std", 0.) > 0.):
        # (a caller that renders a band of a larger batch passes the band's start as ray_base)
        return render_core.advance_after(draws, _batchify_rays, rays_flat, chunk, kwargs)
    return _batchify_rays(rays_flat, chunk, kwargs)


def _batchify_rays(rays_flat, chunk, kwargs):
    kwargs = dict(kwargs)
    base0 = int(kwargs.pop("ray_base", None) or 0)
    based = (lambda i: {"ray_base": base0 + i}) if kwargs.get("draws") is not None else (lambda i: {})
    # (render_rays is looked up when a piece is rendered: callers and tests wrap the module's function)
    return render_core.render_chunks(lambda i, count: render_rays(rays_flat[i:i + count], **kwargs, **based(i)),
                                     rays_flat.shape[0], chunk, _coalesced(rays_flat, chunk, kwargs), "render")

def render(H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1., use_viewdirs=False,
           c2w_staticcam=None, **kwargs):
    """Render an image or a ray batch - run_nerf.py:74-139.

    Returns ``[rgb_map, disp_map, acc_map, albedo_map, shading_map, residual_map, extras]``.

    With ``use_viewdirs``, the ``[N, 11]`` batch handed to ``batchify_rays`` on a HIP device comes out of ONE launch with the bits
    the lines below give on the reference's CPU path: a device pose (``ndc`` on or off, static camera allowed) through
    ``inerf_gen_rays[_ndc]``, given fp32 device rays without autograd with ``ndc=True`` (no static camera) through
    ``inerf_assemble_rays``.  Everything else - CPU tensors, other dtypes, rays that require grad, given rays with a static
    camera or with ``ndc=False``, ``use_viewdirs=False`` - is the reference's torch lines.
    """
    k_extract = ["rgb_map", "disp_map", "acc_map", "albedo_map", "shading_map", "residual_map"]
    batch = sh = None
    if (c2w is not None and use_viewdirs and isinstance(c2w, torch.Tensor) and c2w.is_cuda
            and (c2w_staticcam is None or (isinstance(c2w_staticcam, torch.Tensor) and c2w_staticcam.is_cuda))):
        # pose -> [H*W, 11] ray batch in one launch (inerf_gen_rays / inerf_gen_rays_ndc): the same bits as the lines below give
        # on the reference's CPU path, on every device (torch's own reductions carry no such promise across devices)
        batch = kernels.gen_rays(c2w.float(), H, W, K[0][0], K[1][1], K[0][2], K[1][2], near, far, True,
                                 None if c2w_staticcam is None else c2w_staticcam.float(),
                                 ndc=_ndc_coefficients(H, W, K[0][0], 1.) if ndc else None)
        sh = (H, W, 3)
    elif c2w is None and use_viewdirs and ndc and c2w_staticcam is None:
        rays_o, rays_d = rays
        if _device_rays(rays_o, rays_d) and not isinstance(near, torch.Tensor) and not isinstance(far, torch.Tensor):
            # given rays -> [N, 11] in one launch (inerf_assemble_rays): view directions, NDC and the near / far columns with the
            # reference's CPU bits (run_nerf.py:106-128).  Only with ndc: without it the view directions are what torch's device
            # norm gives, as before - tests/test_adam_gpu.py::test_three_training_steps_in_place_of_torch_adam compares two
            # optimisers over three jittered steps and holds its 1e-4 on those bits (0.48 of the bound), not on the CPU's
            # (4.7 times it); kernels.assemble_rays itself takes ndc=None
            as_rows = lambda t: t if kernels.rows3_viewable(t) else t.contiguous()
            batch = kernels.assemble_rays(as_rows(rays_o), as_rows(rays_d), near, far, ndc=_ndc_coefficients(H, W, K[0][0], 1.))
            sh = rays_d.shape
    if batch is not None:
        all_ret = batchify_rays(batch, chunk, **kwargs)
        for k in all_ret:
            all_ret[k] = torch.reshape(all_ret[k], list(sh[:-1]) + list(all_ret[k].shape[1:]))
        return [all_ret[k] for k in k_extract] + [{k: all_ret[k] for k in all_ret if k not in k_extract}]
    if c2w is not None:
        rays_o, rays_d = get_rays(H, W, K, c2w)
    else:
        rays_o, rays_d = rays
    if use_viewdirs:
        viewdirs = rays_d
        if c2w_staticcam is not None:
            rays_o, rays_d = get_rays(H, W, K, c2w_staticcam)
        viewdirs = viewdirs / torch.norm(viewdirs, dim=-1, keepdim=True)
        viewdirs = torch.reshape(viewdirs, [-1, 3]).float()
    sh = rays_d.shape
    if ndc:
        rays_o, rays_d = ndc_rays(H, W, K[0][0], 1., rays_o, rays_d)
    rays_o = torch.reshape(rays_o, [-1, 3]).float()
    rays_d = torch.reshape(rays_d, [-1, 3]).float()
    near, far = near * torch.ones_like(rays_d[..., :1]), far * torch.ones_like(rays_d[..., :1])
    rays = torch.cat([rays_o, rays_d, near, far], -1)
    if use_viewdirs:
        rays = torch.cat([rays, viewdirs], -1)
    all_ret = batchify_rays(rays, chunk, **kwargs)
    for k in all_ret:
        all_ret[k] = torch.reshape(all_ret[k], list(sh[:-1]) + list(all_ret[k].shape[1:]))
    k_extract = ["rgb_map", "disp_map", "acc_map", "albedo_map", "shading_map", "residual_map"]
    return [all_ret[k] for k in k_extract] + [{k: all_ret[k] for k in all_ret if k not in k_extract}]


def to8b(x):
    """run_nerf_helpers.py:13 - numpy arrays as there; device tensors are quantised on the device."""
    from . import frames
    return frames.to8b(x)


def render_path(render_poses, hwf, K, chunk, render_kwargs, gt_imgs=None, savedir=None, render_factor=0, update_cluster=False,
                b_f=0.5, cluster_manager_factory=None, refresh=None, evaluator=None, products=None):
    """Render every pose of ``render_poses`` - run_nerf.py:142-272; returns ``(rgbs, disps, cluster_manager)``.

    Same arguments, same returned stacks (``[N, H, W, 3]`` / ``[N, H, W]`` float32 numpy), same files in ``savedir``
    (``{:03d}.png``, ``a*``, ``s*``, ``res*``, ``acc*``).  What differs is the plumbing: a pose becomes its ray batch
    in one launch (``inerf_gen_rays``), a frame's six maps travel to the host as ONE pinned, asynchronous copy that
    overlaps the next frame's kernels (frames.FrameStreamer) instead of six blocking ``.cpu()`` calls, and the host
    looks at a frame only after the next one is enqueued.  ``update_cluster`` needs the mean-shift fitting of the
    reference's ``Cluster_Manager.update_center`` (sklearn; training control plane, not rebuilt here): pass the
    reference's class as ``cluster_manager_factory``.  ``refresh`` (a ``refresh.ClusterRefresh``; opt-in): with
    ``update_cluster`` the sample set, the fit and the ``c*`` / ``edit*`` images stay on the device (csrc/refresh.hip) - same
    returned values, same files; no ``cluster_manager_factory`` is needed then.  ``evaluator`` (an
    ``evaluation.FrameEvaluator``; opt-in): when it holds targets registered for ``render_poses``, every frame's rgb, albedo and
    shading columns are handed to its ``add_frame`` from the device pack, before the host copy - the reference has no metric code
    here (its PSNR line is commented out, run_nerf.py:187-191) and ``gt_imgs`` stays unread; read ``evaluator.results()`` afterwards.
    ``products`` (a ``frames.FrameProducts``; opt-in): the five 8-bit images of a frame - ``{:03d}``, ``a``, ``s``, ``res`` and the
    ``(acc > 10)`` mask ``acc`` - are made on the device in one launch (csrc/frame_vis.hip) and travel as 11 bytes per pixel.  When no
    host-side cluster fit reads the other maps - ``update_cluster`` off, or ``refresh`` given with every pack inside its
    ``keep_bytes`` (``ClusterRefresh.keeps_all``, asked with the first pack's size) - only the columns of the returned
    ``(rgbs, disps)`` travel as floats: 4 floats + 11 bytes per pixel instead of the pack's 12 floats."""
    import os
    from . import frames
    H, W, focal = hwf
    if render_factor != 0:       # render downsampled for speed (run_nerf.py:146-150)
        H = H // render_factor
        W = W // render_factor
        focal = focal / render_factor
    H, W = int(H), int(W)
    keys = ("rgb_map", "disp_map", "acc_map", "albedo_map", "shading_map", "residual_map")
    rgbs, disps, albedos, shadings, residuals, accs, labels, sample_pixels, sample_labels = ([] for _ in range(9))
    frames.ensure_dir(savedir)
    widths = None

    def finish(i, frame):
        if filming and not imaging:
            products.images(i)          # (handed out once: lets go of the frame's host copy)
        if imaging:         # the five 8-bit images come from the device planes
            planes = products.images(i)
            encoded = products.files(i) if getattr(products, "encode", False) else None      # PNG files made on the device
            for prefix in ("", "a", "s", "res", "acc"):
                if encoded is not None:
                    with open(os.path.join(savedir, "{}{:03d}.png".format(prefix, i)), "wb") as fh:
                        fh.write(encoded[prefix])
                else:
                    frames.write_png(os.path.join(savedir, "{}{:03d}.png".format(prefix, i)), planes[prefix])
        if slim:            # the frame holds the rgb and disp columns alone
            m = frames.unpack_frame(frame, widths[:2], keys[:2], (H, W))
            rgbs.append(m["rgb_map"]); disps.append(m["disp_map"])
            return
        m = frames.unpack_frame(frame, widths, keys, (H, W))
        rgbs.append(m["rgb_map"]); disps.append(m["disp_map"]); albedos.append(m["albedo_map"])
        shadings.append(m["shading_map"]); residuals.append(m["residual_map"])
        label = (m["acc_map"] > 10).astype(int)              # run_nerf.py:173 as written there
        labels.append(label)
        accs.append(label.astype(np.float32))
        if update_cluster and not on_device:
            sample_pixels.append(albedos[-1][::2, ::2, :].reshape(-1, 3))
            sample_labels.append(label[::2, ::2].reshape(-1, 1))
        if savedir is not None and not imaging:
            for prefix, img in (("", rgbs[-1]), ("a", albedos[-1]), ("s", shadings[-1]), ("res", residuals[-1]), ("acc", accs[-1])):
                frames.write_png(os.path.join(savedir, "{}{:03d}.png".format(prefix, i)), frames.to8b(img))

    on_device = bool(update_cluster) and refresh is not None
    # with products, the float maps beyond rgb and disp are read on the host only by a host-side cluster fit, or by the refresh
    # pass for a frame whose pack it could not keep on the device (decided at the first frame, from the pack's real size)
    slim = products is not None and not update_cluster
    imaging = products is not None and savedir is not None            # (without savedir nobody looks at the images)
    filming = products is not None and bool(getattr(products, "movies", None))      # FrameProducts(movies=...): the planes feed movie files
    evaluating = evaluator is not None and evaluator.begin(render_poses)
    streamer, in_flight = None, []
    for i, c2w in enumerate(render_poses):
        out = render(H, W, K, chunk=chunk, c2w=c2w[:3, :4], **render_kwargs)
        pack, widths = frames.pack_maps({k: v.detach().reshape(H * W, -1) for k, v in zip(keys, out[:6])}, keys)
        if on_device:
            if not pack.is_cuda:
                raise RuntimeError(f"render_path(refresh=...): the rendered maps live on {pack.device}; the refresh pass runs only on a "
                                   "HIP device (no CPU / eager fallback exists)")
            if i == 0:                                   # class_num == 1 (run_nerf.py:218): the (acc > 10) label is not read
                refresh.begin(len(render_poses), H, W, 1, pack.device)
                # the refresh pass reads host maps only for a frame whose pack it did not keep: its own rule says whether one will be
                keeps_all = getattr(refresh, "keeps_all", None)
                slim = products is not None and keeps_all is not None and keeps_all(len(render_poses), pack.numel() * pack.element_size())
            refresh.add_frame(i, pack, widths, keys)
        if evaluating:
            start = {k: sum(widths[:j]) for j, k in enumerate(keys)}
            cols = {k: pack[:, start[k]:start[k] + widths[j]] for j, k in enumerate(keys)}
            evaluator.add_frame(i, rgb=cols["rgb_map"], albedo=cols["albedo_map"], shading=cols["shading_map"])
        if products is not None and not pack.is_cuda:
            raise RuntimeError(f"render_path(products=...): the rendered maps live on {pack.device}; the frame images are made only on a "
                               "HIP device (no CPU / eager fallback exists)")
        if imaging or filming:
            if i == 0:
                products.begin([("", "to8b", "rgb_map"), ("a", "to8b", "albedo_map"), ("s", "to8b", "shading_map"),
                                ("res", "to8b", "residual_map"), ("acc", "thresh", "acc_map", 10.0)],           # run_nerf.py:173
                               keys, widths, (H, W), pack.device)
            products.add_frame(i, pack)
        if pack.is_cuda:
            if streamer is None:
                streamer = frames.FrameStreamer(pack.device)
            done = streamer.push(pack[:, :4].contiguous() if slim else pack)          # slim: rgb_map and disp_map lead the pack
            in_flight.append(i)
            if done is not None:
                finish(in_flight.pop(0), done)
        else:
            finish(i, pack.numpy())
    if streamer is not None:
        for frame in streamer.drain():
            finish(in_flight.pop(0), frame)
    if filming:
        products.close_movies()
    cluster_manager = None
    if on_device:
        # the sample table was filled frame by frame; the fit reads it where it is, and every kept pack becomes its two 8-bit images
        cluster_manager = refresh.finish(b_f, host=None if slim else (lambda i: (albedos[i], None, shadings[i], residuals[i])))
        if savedir is not None:
            for i in range(len(rgbs)):
                c, edit = refresh.snap(i)
                frames.write_png(os.path.join(savedir, "c{:03d}.png".format(i)), c)
                frames.write_png(os.path.join(savedir, "edit{:03d}.png".format(i)), edit)
    elif update_cluster:
        if cluster_manager_factory is None:
            raise NotImplementedError("render_path(update_cluster=True) fits mean-shift clusters (Cluster_Manager.update_center, "
                                      "object_level cluster code of the reference); pass that class as cluster_manager_factory")
        cluster_manager = cluster_manager_factory(class_num=1)
        cluster_manager.update_center(np.concatenate(sample_labels, 0), np.concatenate(sample_pixels, 0), band_factor=b_f)
        dev = render_poses[0].device if isinstance(render_poses[0], torch.Tensor) else "cpu"
        for i, albedo in enumerate(albedos):           # run_nerf.py:226-241
            pixel = torch.from_numpy(albedo).reshape(-1, 3).to(dev)
            label = torch.from_numpy(labels[i]).reshape(-1, 1).to(dev)
            result = cluster_manager.dest_color(pixel, label).reshape(albedo.shape).cpu().numpy()
            if savedir is not None:
                frames.write_png(os.path.join(savedir, "c{:03d}.png".format(i)), frames.to8b(result))
                edit = (result.reshape(-1, 3) * shadings[i].reshape(-1, 1) + residuals[i].reshape(-1, 3)).reshape(result.shape)
                frames.write_png(os.path.join(savedir, "edit{:03d}.png".format(i)), frames.to8b(edit))
    return np.stack(rgbs, 0), np.stack(disps, 0), cluster_manager


# ----------------------------------------------------------------------------------------------
# ray generation (input producers of the path)
# ----------------------------------------------------------------------------------------------
def get_rays(H, W, K, c2w):
    """Pinhole rays in the OpenGL (-z forward) convention - run_nerf_helpers.py:359-368."""
    dev = c2w.device if isinstance(c2w, torch.Tensor) else None
    c2w = torch.as_tensor(c2w, dtype=torch.float32, device=dev)
    if c2w.is_cuda:       # one HIP launch, the reference's CPU bits on every device (csrc/frame_ops.hip)
        rays = kernels.gen_rays(c2w, H, W, K[0][0], K[1][1], K[0][2], K[1][2], 0., 1., True).reshape(H, W, -1)
        return rays[..., 0:3], rays[..., 3:6]
    j, i = torch.meshgrid(torch.linspace(0, H - 1, H, device=c2w.device), torch.linspace(0, W - 1, W, device=c2w.device),
                          indexing="ij")
    dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)
    rays_o = c2w[:3, -1].expand(rays_d.shape)
    return rays_o, rays_d


def get_rays_np(H, W, K, c2w):
    """NumPy twin of get_rays - run_nerf_helpers.py:371-378."""
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    dirs = np.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -np.ones_like(i)], -1)
    rays_d = np.sum(dirs[..., np.newaxis, :] * c2w[:3, :3], -1)
    return np.broadcast_to(c2w[:3, -1], np.shape(rays_d)), rays_d


def _ndc_coefficients(H, W, focal, near):
    """``(sx, sy, near)`` of ndc_rays: the reference's two scalar expressions (run_nerf_helpers.py:387-393) evaluated with the
    caller's own objects; the kernels round each to fp32 once, as ATen does with a Python scalar."""
    return -1. / (W / (2. * focal)), -1. / (H / (2. * focal)), near


def _device_rays(rays_o, rays_d):
    """Given rays the one-launch kernels take: two fp32 tensors of one shape [..., 3] on one HIP device, no autograd."""
    return (isinstance(rays_o, torch.Tensor) and isinstance(rays_d, torch.Tensor) and rays_o.is_cuda and rays_o.device == rays_d.device
            and rays_o.dtype == torch.float32 and rays_d.dtype == torch.float32 and rays_o.shape == rays_d.shape
            and rays_o.dim() >= 1 and rays_o.shape[-1] == 3 and not rays_o.requires_grad and not rays_d.requires_grad)


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    """Normalised-device-coordinate rays for forward-facing scenes - run_nerf_helpers.py:381-399.  Device fp32 tensors without
    autograd: one HIP launch (inerf_ndc_rays), the reference's CPU bits; CPU tensors: the reference's expressions."""
    sx, sy, _ = _ndc_coefficients(H, W, focal, near)
    if _device_rays(rays_o, rays_d) and not isinstance(near, torch.Tensor):
        as_rows = lambda t: t if kernels.rows3_viewable(t) else t.contiguous()
        return kernels.ndc_rays(as_rows(rays_o), as_rows(rays_d), (sx, sy, near))
    t = -(near + rays_o[..., 2]) / rays_d[..., 2]
    rays_o = rays_o + t[..., None] * rays_d
    o = torch.stack([sx * rays_o[..., 0] / rays_o[..., 2], sy * rays_o[..., 1] / rays_o[..., 2],
                     1. + 2. * near / rays_o[..., 2]], -1)
    d = torch.stack([sx * (rays_d[..., 0] / rays_d[..., 2] - rays_o[..., 0] / rays_o[..., 2]),
                     sy * (rays_d[..., 1] / rays_d[..., 2] - rays_o[..., 1] / rays_o[..., 2]),
                     -2. * near / rays_o[..., 2]], -1)
    return o, d


def create_nerf(args, device=None):
    """Instantiate coarse + fine networks and the render kwargs - run_nerf.py:275-356 (without the
    optimiser / checkpoint bookkeeping, which stays in the caller's training script).

    ``args`` needs: multires, multires_views, i_embed, use_viewdirs, N_importance, N_samples, netdepth,
    netwidth, netdepth_fine, netwidth_fine, netchunk, perturb, white_bkgd, raw_noise_std, lindisp,
    dataset_type, no_ndc.  Returns ``(render_kwargs_train, render_kwargs_test, grad_vars)``.
    """
    device = device or torch.device("cuda")
    embed_fn, input_ch = get_embedder(args.multires, args.i_embed)
    embeddirs_fn, input_ch_views = (get_embedder(args.multires_views, args.i_embed) if args.use_viewdirs else (None, 0))
    output_ch = 5 if args.N_importance > 0 else 4
    model = NeRF(D=args.netdepth, W=args.netwidth, input_ch=input_ch, output_ch=output_ch, skips=[4],
                 input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs).to(device)
    grad_vars = list(model.parameters())
    model_fine = None
    if args.N_importance > 0:
        model_fine = NeRF(D=args.netdepth_fine, W=args.netwidth_fine, input_ch=input_ch, output_ch=output_ch, skips=[4],
                          input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs).to(device)
        grad_vars += list(model_fine.parameters())
    train = {"network_query_fn": NetworkQuery(embed_fn, embeddirs_fn, args.netchunk), "perturb": args.perturb,
             "N_importance": args.N_importance, "network_fine": model_fine, "N_samples": args.N_samples,
             "network_fn": model, "use_viewdirs": args.use_viewdirs, "white_bkgd": args.white_bkgd,
             "raw_noise_std": args.raw_noise_std}
    if args.dataset_type != "llff" or args.no_ndc:
        train["ndc"] = False
        train["lindisp"] = args.lindisp
    test = dict(train)
    test["perturb"] = False
    test["raw_noise_std"] = 0.
    return train, test, grad_vars
