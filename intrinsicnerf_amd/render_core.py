"""The render control path the two front-ends (``object_level.py``, ``ssr.py``) share: which kernel path a batch takes, when the
f16 range words are read, what is rendered again in exact fp32, and how a training step falls back to the fp32 layer kernels.

  _fusable / run_network        is (network, encoders) a fused-kernel combination; arbitrary points through it
  render_chunks / advance_after the chunk loop of both ``batchify_rays``; the training draws' step after the last chunk
  staged_pass / make_query / training_step
                                coarse sampling, query, composite, fine sampling, query, composite on the stage kernels
  render_fused / report_non_finite
                                the whole-path launch with its range check; the reference's nan/inf print

Everything here is plumbing: the arithmetic is ``libinerf.so``'s (kernels.py, layered.py).  The front-ends keep what differs between
them: argument handling, RNG draws in their reference's order, the coalescing policy and the names of the returned keys.
"""
import contextlib
import os
import warnings

import torch
import torch.nn as nn

from . import _capi, kernels, layered, packing


def _fusable(fn, embed_fn, embeddirs_fn):
    """Descriptor if (network, encoders) is a combination the fused kernel implements, else None."""
    from .object_level import Embedder
    if not hasattr(fn, "fused_desc"):
        return None
    desc = fn.fused_desc()
    if desc is None or not isinstance(embed_fn, Embedder) or not isinstance(embeddirs_fn, Embedder):
        return None
    if embed_fn.n_freqs != desc.l_xyz or embeddirs_fn.n_freqs != desc.l_dir or embeddirs_fn.scalar_factor != 1.0:
        return None
    desc.xyz_div = embed_fn.scalar_factor
    return desc


def _wants_grad(*modules):
    """True inside a training step: autograd is recording and some network parameter is trainable."""
    return torch.is_grad_enabled() and any(p.requires_grad for m in modules if isinstance(m, nn.Module) for p in m.parameters())


_told_training_path = False


def _training_path_notice(what):
    """Training steps (run_nerf.py:942-1018, trainer.py:882-990) take the STAGED path: sampling and compositing run
    on the HIP kernels - compositing with its HIP backward (inerf_composite_backward) - and each network is one
    autograd node (kernels.mlp_train): fused HIP forward that keeps the activations, HIP input-gradient chain, weight
    gradients by the split-K MFMA kernel.  A network outside the fused architecture, ``INERF_TRAIN_MLP=layered`` and a batch
    outside the f16 range go layer by layer through the exact-fp32 MFMA kernels (layered.py: HIP forward and backward too);
    ``INERF_TRAIN_MLP=torch`` evaluates the modules' torch ``forward`` under autograd (debugging).  Said once per process."""
    global _told_training_path
    if not _told_training_path:
        warnings.warn(f"{what}: gradients requested - using the staged training path (HIP sampling, HIP compositing and "
                      "network kernels with HIP backward).  Render under torch.no_grad() for the fully fused path.")
        _told_training_path = True


_told_unfused = False


def _unfused_notice(what):
    """Said once per process (the object-level front-end's staged branch does the same for foreign networks)."""
    global _told_unfused
    if not _told_unfused:
        warnings.warn(f"{what}: network / encoders outside the fused kernels' architecture (D=8, W=256, skips=[4], multires<=10, "
                      "multires_views<=4): HIP sampling and compositing, the networks layer by layer on the fp32 MFMA kernels "
                      "(a foreign callable: through its own forward).")
        _told_unfused = True


def _train_desc(desc):
    """Descriptor for the fused training evaluation of a fusable network, or None when the layers are evaluated one by one:
    ``INERF_TRAIN_MLP`` = ``hip`` (default: fused split-precision forward that keeps the activations + HIP backward, kernels.mlp_train) |
    ``layered`` (exact fp32 throughout, like the reference's run_nerf.py:942-1018: the fp32 MFMA layer kernels, forward and backward) |
    ``torch`` (the modules' own torch ``forward`` under autograd: the comparison baseline of the gradient tests)."""
    if desc is None or os.environ.get("INERF_TRAIN_MLP", "hip") in ("torch", "layered"):
        return None
    return desc           # precision f32: exact-fp32 forward values, split-precision saved activations + HIP backward (kernels.mlp_train)


FP32_LAYERS_NOTE = "Evaluating this batch with the fp32 layer kernels instead."


def _train_query(train_desc, fn, ray_batch, z_vals, endpoint=False):
    """raw for a training step through kernels.mlp_train; None if this batch left the f16 range (the caller then evaluates it
    layer by layer in exact fp32: ``_layered_spec``)."""
    try:
        return kernels.mlp_train(train_desc, fn, ray_batch, z_vals, endpoint)
    except FloatingPointError as e:
        warnings.warn(f"{e}  {FP32_LAYERS_NOTE}")
        return None


def _layered_spec(fn, embed_fn, embeddirs_fn, with_dirs=True):
    """layered.Spec when ``fn`` can be evaluated layer by layer on the fp32 MFMA kernels (any D / W / skips of this package's
    networks, fed by this package's encoders), else None.  ``INERF_TRAIN_MLP=torch`` keeps torch's layers for a training step
    (the comparison baseline of the gradient tests)."""
    if os.environ.get("INERF_TRAIN_MLP", "hip") == "torch" and _wants_grad(fn):
        return None
    spec = layered.spec_for(fn, embed_fn, embeddirs_fn if with_dirs else None)
    if spec is None or spec.use_viewdirs != bool(with_dirs):
        return None
    return spec


def _run_network_torch(inputs, viewdirs, fn, embed_fn, embeddirs_fn, netchunk):
    """run_nerf.py:42-56 as written there: torch-evaluated embedding, ``fn`` applied in ``netchunk`` pieces.  Used for
    networks the fused kernel does not implement and for training steps (autograd records the layers)."""
    flat = torch.reshape(inputs, [-1, inputs.shape[-1]])
    emb = embed_fn(flat)
    if viewdirs is not None:
        dirs = viewdirs[:, None].expand(inputs.shape)
        emb = torch.cat([emb, embeddirs_fn(torch.reshape(dirs, [-1, dirs.shape[-1]]))], -1)
    out = torch.cat([fn(emb[i:i + netchunk]) for i in range(0, emb.shape[0], netchunk)], 0) if netchunk else fn(emb)
    return torch.reshape(out, list(inputs.shape[:-1]) + [out.shape[-1]])


def run_network(inputs, viewdirs, fn, embed_fn, embeddirs_fn, netchunk, endpoint=False, foreign=None):
    """Encode ``inputs[..., 3]`` (+ ``viewdirs[N, 3]``) and apply network ``fn`` - the body of both front-ends' ``run_network``.
    ``endpoint``: the raw rows carry the SSR network's endpoint feature.  ``foreign``: what is applied to the torch-evaluated
    embedding when ``fn`` is not one of this package's networks (default: ``fn`` itself, as the reference calls it)."""
    desc = _fusable(fn, embed_fn, embeddirs_fn) if viewdirs is not None else None
    if desc is None or _wants_grad(fn):
        # another depth / width / skip list, no view directions, or gradients wanted for arbitrary points: layer by layer on the
        # fp32 MFMA kernels (differentiable w.r.t. the parameters); a foreign callable is called as the reference calls it
        if desc is not None:
            _training_path_notice("run_network")
        spec = _layered_spec(fn, embed_fn, embeddirs_fn, viewdirs is not None) if inputs.is_cuda else None
        if spec is not None:
            return layered.evaluate_points(spec, fn, inputs, viewdirs, endpoint=endpoint)
        return _run_network_torch(inputs, viewdirs, fn if foreign is None else foreign, embed_fn, embeddirs_fn, netchunk)
    # arbitrary points: one "ray" per point with origin = point, direction = 0, depth 0 -> o + 0*0 = o
    pts = torch.reshape(inputs, [-1, 3]).float()
    dirs = torch.reshape(viewdirs[:, None].expand(inputs.shape), [-1, 3]).float()
    rays = torch.zeros(pts.shape[0], _capi.RAY_FLOATS, dtype=torch.float32, device=pts.device)
    rays[:, 0:3], rays[:, 8:11] = pts, dirs
    z = torch.zeros(pts.shape[0], 1, dtype=torch.float32, device=pts.device)

    def run(d):
        status = kernels._new_status(pts) if d.precision == _capi.PREC_F16X3 else None
        out = kernels.encode_mlp(d, packing.packed_for_module(fn, d, pts.device), rays, z, endpoint=endpoint, status=status)
        kernels.check_f16_range(status, "run_network")
        return out

    raw = kernels.with_f32_fallback(desc, run)
    return torch.reshape(raw, list(inputs.shape[:-1]) + [raw.shape[-1]])


# ----------------------------------------------------------------------------------------------
# the chunk loop (run_nerf.py:59-71, training_utils.py:5-17)
# ----------------------------------------------------------------------------------------------
def render_chunks(piece, n_rays, chunk, big, what):
    """``piece(i, count)`` - a dict of tensors for rays ``[i, i + count)`` - over ``n_rays`` rays, ``big >= chunk`` rays per call;
    the pieces' tensors concatenated (one piece: its own tensors; no rays: ``{}``).

    The split-precision kernel's range words are read ONCE, after the last piece has been enqueued (kernels.deferred_range_checks): a
    frame is one host synchronisation, not one per chunk.  With ``big > chunk`` (an eval-mode frame whose result cannot depend on the
    chunk boundaries: kernels.coalesced_chunk) the launches keep one range word per CALLER's chunk (kernels.chunked_status).  The
    chunks whose word reports an out-of-range activation - and only those - are rendered again with the exact fp32 kernel (only
    eval-mode pieces defer, so no random draw is repeated; pieces that draw random numbers check and fall back inside ``piece``)."""
    rets = []
    with kernels.deferred_range_checks(what, raise_on_trip=False) as block, (
            kernels.chunked_status(chunk) if big > chunk else contextlib.nullcontext()):
        for j, i in enumerate(range(0, n_rays, big)):
            block.tag = j
            rets.append(piece(i, min(big, n_rays - i)))
    if not rets:
        return {}
    out = {k: (rets[0][k] if len(rets) == 1 else torch.cat([r[k] for r in rets], 0)) for k in rets[0]}
    if block.tripped:
        # tags: (piece, word) of a piece with one word per caller's chunk, or the piece itself (it held no more than one chunk)
        spans = sorted({(t[0] * big + t[1] * chunk, chunk) if isinstance(t, tuple) else (t * big, big) for t in block.tripped})
        kernels.warn_f32_fallback(f"{what}: {len(spans)} of {-(-n_rays // chunk)} chunks left the f16 range of the "
                                  "split-precision MLP kernel.")
        with _capi.forced_precision(_capi.PREC_F32):
            for i, n_i in spans:
                n_i = min(n_i, n_rays - i)
                again = piece(i, n_i)
                for k in out:
                    out[k][i:i + n_i] = again[k]
    return out


def advance_after(draws, loop, *args, **kwargs):
    """``loop(*args, **kwargs)`` for a render that draws in the kernels (``draws``: a draws.DrawState): every chunk draws at the
    same step with its first global ray index as base, so the result does not depend on the chunking; the step advances once,
    after the last chunk - a chunk rendered again in exact fp32 repeats its own draws."""
    try:
        return loop(*args, **kwargs)
    finally:
        draws.advance()


# ----------------------------------------------------------------------------------------------
# one ray batch: staged (training steps, networks outside the fused architecture) and fused
# ----------------------------------------------------------------------------------------------
def make_query(train_desc, ray_batch, encoders, foreign):
    """``query(z, fn, endpoint)`` -> raw of network ``fn`` on the sample points of ``ray_batch`` at depths ``z``: through
    kernels.mlp_train with ``train_desc``; else - ``encoders`` = this package's (embed_fn, embeddirs_fn), or None - layer by layer on
    the fp32 kernels (any depth / width / skips, or a batch outside the f16 range); else ``foreign(pts, viewdirs, fn, endpoint)``,
    the front-end's call of a foreign network or query function as its reference calls it."""
    rays_o, rays_d, viewdirs = ray_batch[:, 0:3], ray_batch[:, 3:6].contiguous(), ray_batch[:, -3:]

    def query(z, fn, endpoint=False):
        raw = _train_query(train_desc, fn, ray_batch, z, endpoint) if train_desc is not None else None
        if raw is None:
            spec = _layered_spec(fn, *encoders) if encoders is not None else None
            if spec is not None:
                raw = layered.evaluate(spec, fn, ray_batch, z, endpoint)
            else:
                pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., :, None]
                raw = foreign(pts, viewdirs, fn, endpoint)
        return raw

    return query


def staged_pass(ray_batch, t_vals, rand, dr, nets, query, n_importance, white_bkgd=False, lindisp=False, n_classes=0, endpoint=False):
    """run_nerf.py:415-528 / trainer.py:717-808 stage by stage: HIP sampling, HIP compositing with its HIP backward, the networks
    ``nets`` = (coarse, fine) through ``query`` (make_query).  ``rand`` = the pre-drawn (t_rand, noise_c, u, noise_f); ``dr`` = None,
    or the draw arguments {"perturb", "noise_c", "noise_f"} of what is drawn in the kernels instead.  Same keys as
    kernels.render_rays_fused."""
    t_rand, noise_c, u, noise_f = rand
    dr = dr or {"perturb": None, "noise_c": None, "noise_f": None}
    rays_d = ray_batch[:, 3:6].contiguous()
    z_vals = kernels.sample_coarse(ray_batch, t_vals, t_rand, lindisp, draw=dr["perturb"])
    raw = query(z_vals, nets[0], False)
    c = kernels.composite(raw.float(), z_vals, rays_d, noise_c, white_bkgd, n_classes=n_classes, draw=dr["noise_c"])
    o = {k + "_coarse": v for k, v in c.items()}
    o["raw_coarse"] = raw
    if n_importance > 0:
        # the resampled depths carry no gradient (z_samples.detach(), run_nerf.py:501, trainer.py:762)
        z_samples, z_fine, z_std = kernels.sample_fine(z_vals, c["weights"].detach(), u, n_importance, draw=dr["perturb"])
        raw = query(z_fine, nets[1], endpoint)
        # the endpoint feature is the LAST 128 channels of raw (model_utils.py:99-103, a literal 128 there).  A foreign netwidth
        # gives raw another width (W // 2 feature channels): the kernel's feature lanes only take the 256-wide network's layout,
        # the reference's literal slice is evaluated as written for any other
        native_feat = endpoint and raw.shape[-1] == 11 + n_classes + 128
        f = kernels.composite(raw.float(), z_fine, rays_d, noise_f, white_bkgd, n_classes=n_classes, feat_dim=128 if native_feat else 0,
                              draw=dr["noise_f"])
        if endpoint and not native_feat:
            f["feat"] = torch.sum(f["weights"][..., None] * raw[..., -128:], -2)
        o.update({k + "_fine": v for k, v in f.items()})
        o["raw_fine"], o["z_std"] = raw, z_std
    return o


def training_step(staged, train_desc, what):
    """``staged(train_desc)`` with ONE read of the f16 range words per training forward, after every launch of the batch has been
    enqueued (a read after each network leaves the GPU idle while the host prepares the next launches).  If it trips, the whole batch
    is evaluated again layer by layer in exact fp32 (``staged(None)``: HIP forward and backward, no range limit) - with the same
    pre-drawn random tensors, so it consumes the RNG like the reference would."""
    if train_desc is None:
        return staged(None)
    try:
        with kernels.deferred_range_checks(f"{what} (training step)"):
            o = staged(train_desc)
    except FloatingPointError as e:
        warnings.warn(f"{e}  {FP32_LAYERS_NOTE}")
        o = staged(None)
    return o


def render_fused(desc, net_coarse, net_fine, what, ray_batch, n_samples, n_importance, t_vals, u, t_rand, noise_c, noise_f, **kwargs):
    """kernels.render_rays_fused (``kwargs``: its remaining keywords) with its f16 range check, once more in exact fp32 if that trips."""
    dev = ray_batch.device

    def run(d):
        res = kernels.render_rays_fused(
            d, packing.packed_for_module(net_coarse, d, dev),
            packing.packed_for_module(net_fine, d, dev) if n_importance > 0 else None,
            ray_batch, n_samples, n_importance, t_vals, u, t_rand, noise_c, noise_f, **kwargs)
        # eval-mode chunks of a frame (no RNG draws to repeat) leave the check to the chunk loop's end-of-frame one; so do chunks
        # whose draws come from the kernels (a second render of the chunk repeats them: the step has not advanced)
        kernels.check_f16_range(res.pop("status", None), what, deferrable=t_rand is None and noise_c is None)
        return res

    return kernels.with_f32_fallback(desc, run)


def report_non_finite(ret):
    """The reference's nan/inf scan (run_nerf.py:524-526, trainer.py:803-806); each check is a device sync, so not while a HIP
    graph records."""
    if kernels._capturing():
        return
    for k in ret:
        if torch.isnan(ret[k]).any() or torch.isinf(ret[k]).any():
            print(f"! [Numerical Error] {k} contains nan or inf.")
