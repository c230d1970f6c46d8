"""The training losses of both reference trainers on one forward and one backward HIP launch (csrc/losses.hip).

``compute_intrinsic_loss`` is the reference's function of that name (object_level/run_nerf_helpers.py:59-86 with a float
mask, SSR/training/training_utils.py:179-207 with int64 semantic labels): the same six 0-dim tensors in the same order,
differentiable through ONE autograd node, so the caller's own weighted sum (run_nerf.py:980-982, trainer.py:978-981)
drives one backward launch.  ``--inerf-losses`` of ``intrinsicnerf_amd.launch`` binds it into the reference's scripts.

``object_step_loss`` / ``ssr_step_loss`` are a whole step's loss - coarse and fine level, img2mse on the image
(run_nerf.py:976,1006; trainer.py:923,936) and on the cluster target (run_nerf.py:987,1012; trainer.py:985-986), the SSR
cross-entropy on ``label - 1`` with ``ignore_index = -1`` (trainer.py:858-865) and the weighted sum - in one forward and one
backward launch: what a ``graphs.GraphedTrainStep`` loss function calls.  Neither launch reads anything on the host.

Reference behaviour that is reproduced (tests/golden/loss_*.npz):

* pairing: ``split = N // 2``, ray ``i < split`` with ray ``i + (N - split)`` (an odd N leaves the middle ray alone);
  ``split2 = split // 2``, ray ``i < split2`` with ray ``i + (split - split2)``; ``disp`` and ``acc`` are accepted and not
  read (the reference computes ``compute_depth_weight`` and passes the literal 1);
* a mask of shape ``[N, 1]`` (``images[..., -1:]``, run_nerf.py:703) makes the reference broadcast its pair weights to a
  ``[split, split]`` matrix: sparsity, shading and far term become ``mean(mask product) * mean(weight * distance)``.  Both
  mask shapes are accepted and each is reproduced; the matrix is never formed;
* ``N < 4`` (no far pair) gives NaN for the far term, a batch whose labels are all void NaN for the cross-entropy.

There is no CPU or eager path: tensors that are not on a HIP device raise, as in the render entry points.
"""
import ctypes as C

import torch

from . import _capi
from .kernels import _dev, _stream

TERMS = _capi.LOSS_TERM_NAMES          # order of the terms inside the kernels' state
_STATE = _capi.LOSS_STATE_FLOATS
# compute_intrinsic_loss's return order (run_nerf_helpers.py:86): chroma, residual, reflect_sparsity, shading_smooth, far_reflect, intensity
_SIX = tuple(TERMS.index(n) for n in ("chroma", "residual", "sparsity", "shading", "far", "intensity"))

_weights = {}       # (device, values) -> device tensor[9]: a trainer changes its weights twice in 200 000 steps
_zeros = {}


def _weight_tensor(weights, device):
    unknown = set(weights) - set(TERMS)
    if unknown:
        raise ValueError(f"unknown loss weights {sorted(unknown)}: expected a subset of {TERMS}")
    values = tuple(float(weights.get(n, 1.0)) for n in TERMS)
    key = (str(device), values)
    t = _weights.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a new set of loss weights during graph capture: call the loss once with these weights before capturing")
        if len(_weights) > 256:
            _weights.clear()
        t = _weights[key] = torch.tensor(values, dtype=torch.float32, device=device)
    return t


def _zero(device):
    t = _zeros.get(str(device))
    if t is None:
        t = _zeros[str(device)] = torch.zeros((), dtype=torch.float32, device=device)
    return t


def _labels(t, name, n):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} lives on {t.device}: intrinsicnerf_amd runs only on a HIP device (no CPU / eager fallback exists)")
    if t.dtype != torch.int64:
        raise ValueError(f"{name} must be int64, got {t.dtype}")
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected ({n},)")
    return t if t.is_contiguous() else t.contiguous()


class _Config:
    """What one call of the kernels needs besides its tensors."""

    def __init__(self, n, n_levels, flags, n_classes, ce_offset, have_rgb, have_logits, six):
        self.n, self.n_levels, self.flags, self.n_classes, self.ce_offset = n, n_levels, flags, n_classes, ce_offset
        self.have_rgb, self.have_logits, self.six = have_rgb, have_logits, six
        self.per_level = 3 + int(have_rgb) + int(have_logits)


def _fill(args, cfg, gt, key, target, ce_labels, weights, levels, state):
    args.n_rays, args.n_levels, args.n_classes = cfg.n, cfg.n_levels, cfg.n_classes
    args.flags, args.ce_label_offset = cfg.flags, cfg.ce_offset
    args.gt_rgb, args.pair_key = gt.data_ptr(), key.data_ptr()
    args.cluster_target = None if target is None else target.data_ptr()
    args.ce_labels = None if ce_labels is None else ce_labels.data_ptr()
    args.weights = None if weights is None else weights.data_ptr()
    for l in range(cfg.n_levels):
        t = list(levels[l * cfg.per_level:(l + 1) * cfg.per_level])
        lv = args.level[l]
        lv.albedo, lv.shading, lv.residual = (x.data_ptr() for x in t[:3])
        lv.rgb = t[3].data_ptr() if cfg.have_rgb else None
        lv.logits = t[-1].data_ptr() if cfg.have_logits else None
    args.state, args.state_bytes = state.data_ptr(), state.numel() * 4


class _Loss(torch.autograd.Function):
    """inputs: cfg, gt, key, target, ce_labels, weights, then per level albedo, shading, residual[, rgb][, logits]."""

    @staticmethod
    def forward(ctx, cfg, gt, key, target, ce_labels, weights, *levels):
        lib = _capi.lib()
        state = torch.empty((cfg.n_levels + 1) * _STATE, dtype=torch.float32, device=gt.device)
        args = _capi.LossArgs()
        _fill(args, cfg, gt, key, target, ce_labels, weights, levels, state)
        _capi.check(lib.inerf_intrinsic_loss(C.byref(args), _stream(gt)), "inerf_intrinsic_loss")
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(gt, key, target, ce_labels, weights, state, *levels)
        if cfg.six:
            return tuple(state[t] for t in _SIX)
        return state[cfg.n_levels * _STATE], state[:cfg.n_levels * _STATE].view(cfg.n_levels, _STATE)

    @staticmethod
    def backward(ctx, *grads):
        cfg = ctx.cfg
        gt, key, target, ce_labels, weights, state, *levels = ctx.saved_tensors
        lib = _capi.lib()
        args = _capi.LossArgs()
        _fill(args, cfg, gt, key, target, ce_labels, weights, levels, state)
        if cfg.six:
            # the caller's own weighted sum: one upstream gradient per returned term (None for a term it left out)
            zero = _zero(gt.device)
            per_term = [zero] * _capi.LOSS_TERMS
            for t, g in zip(_SIX, grads):
                if g is not None:
                    per_term[t] = g.reshape(())
            g_terms = torch.stack(per_term)
            args.grad_total, args.grad_terms = None, g_terms.data_ptr()
        else:
            g_total, g_terms = grads
            if g_terms is not None:
                g_terms = g_terms.contiguous()
            args.grad_total = None if g_total is None else g_total.data_ptr()
            args.grad_terms = None if g_terms is None else g_terms.data_ptr()
        out = [torch.empty_like(t) for t in levels]
        for l in range(cfg.n_levels):
            t = out[l * cfg.per_level:(l + 1) * cfg.per_level]
            lv = args.level[l]
            lv.d_albedo, lv.d_shading, lv.d_residual = (x.data_ptr() for x in t[:3])
            lv.d_rgb = t[3].data_ptr() if cfg.have_rgb else None
            lv.d_logits = t[-1].data_ptr() if cfg.have_logits else None
        _capi.check(lib.inerf_intrinsic_loss_backward(C.byref(args), _stream(gt)), "inerf_intrinsic_loss_backward")
        need = ctx.needs_input_grad[6:]
        return (None,) * 6 + tuple(g if n else None for g, n in zip(out, need))


def _pair_key(key, n, name):
    """(tensor, flags) of a float mask [N] / [N,1] or int64 labels [N]."""
    if not isinstance(key, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if key.dtype == torch.int64:
        return _labels(key, name, n), _capi.LOSS_KEY_LABELS
    if key.dim() == 2 and key.shape[1] == 1:
        return _dev(key, name, (n, 1)).reshape(n), _capi.LOSS_MASK_OUTER
    return _dev(key, name, (n,)), 0


def _level(albedo, shading, residual, n, tag=""):
    return [_dev(albedo, "albedo" + tag, (n, 3)), _dev(shading, "shading" + tag, (n,)), _dev(residual, "residual" + tag, (n, 3))]


def compute_intrinsic_loss(albedo, shading, residual, gt_rgb, disp, acc, obj_mask):
    """run_nerf_helpers.py:59-86 (``obj_mask``: float ``[N]`` or ``[N,1]``) and training_utils.py:179-207 (int64 semantic
    labels ``[N]`` in its place): ``(chroma, residual, reflect_sparsity, shading_smooth, far_reflect, intensity)``."""
    gt_rgb = _dev(gt_rgb, "gt_rgb", (None, 3))
    n = gt_rgb.shape[0]
    key, flags = _pair_key(obj_mask, n, "obj_mask")
    cfg = _Config(n, 1, flags, 0, 0, False, False, True)
    return _Loss.apply(cfg, gt_rgb, key, None, None, None, *_level(albedo, shading, residual, n))


def compute_intrinsic_loss_ssr(albedo, shading, residual, gt_rgb, disp, acc, semantic_label):
    """training_utils.py:179-207 under its own parameter name (``semantic_label``: int64 ``[N]``)."""
    if isinstance(semantic_label, torch.Tensor) and semantic_label.dtype != torch.int64:
        raise ValueError(f"semantic_label must be int64, got {semantic_label.dtype}")
    return compute_intrinsic_loss(albedo, shading, residual, gt_rgb, disp, acc, semantic_label)


def _step_loss(levels, n_levels, gt_rgb, key, flags, weights, cluster_target, ce_labels, n_classes):
    n = gt_rgb.shape[0]
    if cluster_target is not None:
        cluster_target = _dev(cluster_target.detach(), "cluster_target", (n, 3))
    w = _weight_tensor(weights, gt_rgb.device)
    cfg = _Config(n, n_levels, flags, n_classes, -1, True, ce_labels is not None, False)
    total, terms = _Loss.apply(cfg, gt_rgb, key, cluster_target, ce_labels, w, *levels)
    present = [t for t in TERMS if not (t == "cluster" and cluster_target is None) and not (t == "semantic" and ce_labels is None)]
    return total, {name: terms[:, TERMS.index(name)] for name in present}


def object_step_loss(ret, target_rgb, target_mask, weights, cluster_target=None):
    """The loss of one object-level step (run_nerf.py:976-1013) from ``render_rays``' dictionary: ``rgb_map, albedo_map,
    shading_map, residual_map`` and, with a fine network, ``rgb0, albedo0, shading0, residual0`` (both levels get every
    term).  ``weights``: a mapping over ``TERMS`` (``image, chroma, residual, sparsity, shading, far, intensity, cluster``;
    a missing name weighs 1).  Returns ``(total, terms)``: the weighted sum and, per name, the ``[levels]`` tensor of that
    term (coarse first when there are two).  ``render``'s list ``[rgb, disp, acc, albedo, shading, residual, extras]`` is taken too."""
    if isinstance(ret, (list, tuple)):
        ret = dict(ret[6], rgb_map=ret[0], albedo_map=ret[3], shading_map=ret[4], residual_map=ret[5])
    gt = _dev(target_rgb, "target_rgb", (None, 3))
    n = gt.shape[0]
    key, flags = _pair_key(target_mask, n, "target_mask")
    if flags & _capi.LOSS_KEY_LABELS:
        raise ValueError("target_mask must be a float mask")
    levels, n_levels = [], 1
    if "rgb0" in ret:
        levels += _level(ret["albedo0"], ret["shading0"], ret["residual0"], n, "0") + [_dev(ret["rgb0"], "rgb0", (n, 3))]
        n_levels = 2
    levels += _level(ret["albedo_map"], ret["shading_map"], ret["residual_map"], n, "_map") + [_dev(ret["rgb_map"], "rgb_map", (n, 3))]
    return _step_loss(levels, n_levels, gt, key, flags, dict(weights, semantic=0.0), cluster_target, None, 0)


def ssr_step_loss(ret, target_rgb, semantic_label, weights, cluster_target=None, semantic=True):
    """The loss of one SSR step (trainer.py:923-988) from ``render_rays``' dictionary (``rgb_coarse, albedo_coarse,
    shading_coarse, residual_coarse, sem_logits_coarse`` and the ``_fine`` ones when present).  ``semantic_label``: the
    UNSHIFTED int64 labels (0 = void): they pair the rays, and ``label - 1`` with ``ignore_index = -1`` is the cross-entropy
    target (trainer.py:865) unless ``semantic`` is False.  ``weights`` / the result: as ``object_step_loss``, plus
    ``semantic``."""
    gt = _dev(target_rgb, "target_rgb", (None, 3))
    n = gt.shape[0]
    key = _labels(semantic_label, "semantic_label", n)
    levels, n_classes = [], 0
    tags = ["_coarse"] + (["_fine"] if "rgb_fine" in ret else [])
    for tag in tags:
        levels += _level(ret["albedo" + tag], ret["shading" + tag], ret["residual" + tag], n, tag) + [_dev(ret["rgb" + tag], "rgb" + tag, (n, 3))]
        if semantic:
            logits = _dev(ret["sem_logits" + tag], "sem_logits" + tag, (n, None))
            n_classes = logits.shape[1]
            if not 1 <= n_classes <= _capi.LOSS_MAX_CLASSES:
                raise ValueError(f"{n_classes} semantic classes: the loss kernels take 1..{_capi.LOSS_MAX_CLASSES}")
            levels.append(logits)
    return _step_loss(levels, len(tags), gt, key, _capi.LOSS_KEY_LABELS, weights if semantic else dict(weights, semantic=0.0),
                      cluster_target, key if semantic else None, n_classes)
