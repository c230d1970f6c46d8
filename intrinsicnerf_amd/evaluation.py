"""Validation metrics on the device.  Of the SSR trainer (csrc/eval.hip): the reference's ``calculate_segmentation_metrics`` and
``calculate_depth_metrics`` (SSR/training/training_utils.py:58-122) and ``img2mse`` / ``mse2psnr`` under their own names and
signatures, and ``FrameEvaluator``, which accumulates them frame by frame beside the render that produced their inputs.

One ``kernels.eval_accumulate`` pass reduces the pixels to an int64 table (the confusion matrix and eight counters) and six
fp64 sums; what remains - normalised rows, the masked means, the ious, a few quotients and square roots - is finished on the
host in float64 numpy by ``finish_segmentation`` / ``finish_depth``, which need no device.  The reference's ``np.float``
(removed in numpy 1.24) is read as ``float``.

Intrinsic-image metrics (csrc/imq.hip; neither reference has code for them, include/inerf.h states the definitions): mse / psnr,
scale-invariant MSE, LMSE and SSIM / DSSIM of image pairs.  One ``kernels.image_quality`` call reduces a whole stack to seven fp64
sums and three counts per image; ``finish_image_quality`` turns a row into the six metrics on the host.  ``FrameEvaluator`` keeps
the rows of rgb, albedo and shading on the device frame by frame and reads them back once.
"""
import warnings

import numpy as np

from . import _capi

COUNT = {name: i for i, name in enumerate(_capi.EVAL_COUNT_NAMES)}
SUM = {name: i for i, name in enumerate(_capi.EVAL_SUM_NAMES)}
IMQ_SUM = {name: i for i, name in enumerate(_capi.IMQ_SUM_NAMES)}
IMQ_COUNT = {name: i for i, name in enumerate(_capi.IMQ_COUNT_NAMES)}
IMAGE_QUALITY_KEYS = ("mse", "psnr", "si_mse", "lmse", "ssim", "dssim")
IMAGE_QUALITY_GROUPS = (("image_quality", "rgb", "image"), ("albedo", "albedo", "albedo"), ("shading", "shading", "shading"))   # (results key, add_frame keyword, target)
DEPTH_KEYS = ("AbsRel", "AbsDiff", "SqRel", "RMSE", "LogRMSE", "r1", "r2", "r3", "complete")


def _masked_mean(values):
    """Mean over the entries that are not NaN, as ``np.ma.masked_array(values, np.isnan(values)).mean()`` gives it (the masked
    constant when there is none)."""
    return np.ma.masked_array(values, np.isnan(values)).mean()


def finish_segmentation(table, n_not_ignored):
    """``(miou, miou_valid_class, total_accuracy, class_average_accuracy, ious)`` from a confusion table [C, C] (row = true,
    column = predicted, integers) and the number of pixels whose true label is not ignored - training_utils.py:59-84 after the
    ``confusion_matrix`` call.  With no such pixel the reference answers ``[0] * 4`` (four items, not five): kept."""
    if int(n_not_ignored) == 0:
        return [0] * 4
    conf = np.asarray(table, dtype=np.int64)
    classes = conf.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        per_true = conf.astype(float).sum(axis=1)                       # pixels of each true class
        norm = np.transpose(np.transpose(conf) / per_true)              # a class that never occurs: a row of NaN
        existing = ~np.isnan(norm.sum(1))
        class_average_accuracy = _masked_mean(np.diagonal(norm))
        total_accuracy = np.sum(np.diagonal(conf)) / np.sum(conf)
        ious = np.zeros(classes)
        for c in range(classes):
            ious[c] = conf[c, c] / (np.sum(conf[c, :]) + np.sum(conf[:, c]) - conf[c, c])
        miou = _masked_mean(ious)
        with warnings.catch_warnings():                                 # no class occurs (every valid pixel outside the table): NaN, quietly
            warnings.simplefilter("ignore")
            miou_valid_class = np.mean(ious[existing])
    return miou, miou_valid_class, total_accuracy, class_average_accuracy, ious


def finish_depth(counts, sums):
    """The reference's dict of depth metrics (training_utils.py:111-120, same keys, same order) from the eight counters and six
    sums of an accumulate pass; float64 throughout, NaN where the mask (or the frame) is empty, as ``np.mean`` of nothing."""
    counts = np.asarray(counts, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    n = np.float64(counts[COUNT["n_mask"]])
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"AbsRel": sums[SUM["abs_rel"]] / n,
                "AbsDiff": sums[SUM["abs_diff"]] / n,
                "SqRel": sums[SUM["sq_rel"]] / n,
                "RMSE": np.sqrt(sums[SUM["sq_diff"]] / n),
                "LogRMSE": np.sqrt(sums[SUM["sq_log_diff"]] / n),
                "r1": np.float64(counts[COUNT["r1"]]) / n,
                "r2": np.float64(counts[COUNT["r2"]]) / n,
                "r3": np.float64(counts[COUNT["r3"]]) / n,
                "complete": np.float64(counts[COUNT["n_pred_positive"]]) / np.float64(counts[COUNT["n_pixels"]])}


def finish_image(counts, sums):
    """``(mse, psnr)``: ``img2mse`` and ``mse2psnr`` (-10 ln(mse) / ln 10) in float64."""
    counts = np.asarray(counts, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = np.float64(np.asarray(sums, dtype=np.float64)[SUM["rgb_sq"]]) / np.float64(counts[COUNT["n_rgb"]])
        return mse, -10.0 * np.log(mse) / np.log(10.0)


_SSIM_TAPS = None


def ssim_taps():
    """The 11 taps of the SSIM window, w_i ~ exp(-(i / 1.5)^2 / 2) for i = -5..5, normalised in float64 on the host (the device
    receives them as 11 doubles and evaluates no exp)."""
    global _SSIM_TAPS
    if _SSIM_TAPS is None:
        w = np.exp(-0.5 * (np.arange(-5, 6, dtype=np.float64) / 1.5) ** 2)
        _SSIM_TAPS = tuple(float(v) for v in w / w.sum())
    return _SSIM_TAPS


def finish_image_quality(sums_row, counts_row, channels):
    """``{"mse", "psnr", "si_mse", "lmse", "ssim", "dssim"}`` of one image from its row of ``image_quality`` sums and counts
    (include/inerf.h, INERF_IMQ_*); float64 throughout, NaN where nothing was counted (0 / 0), no device needed."""
    s = np.asarray(sums_row, dtype=np.float64)
    n = np.asarray(counts_row, dtype=np.int64)
    c = np.float64(int(channels))
    with np.errstate(divide="ignore", invalid="ignore"):
        values = c * np.float64(n[IMQ_COUNT["n_valid"]])
        spp, spg, sgg = s[IMQ_SUM["spp"]], s[IMQ_SUM["spg"]], s[IMQ_SUM["sgg"]]
        mse = s[IMQ_SUM["sq_diff"]] / values
        alpha = spg / spp if spp > 1e-5 else np.float64(0.0)
        si_mse = ((sgg - 2.0 * alpha * spg) + alpha * alpha * spp) / values          # alpha = 0 keeps a NaN of the prediction: 0 * NaN
        lmse = s[IMQ_SUM["lmse_num"]] / s[IMQ_SUM["lmse_den"]]
        ssim = s[IMQ_SUM["ssim_sum"]] / (c * np.float64(n[IMQ_COUNT["n_ssim"]]))
        return {"mse": mse, "psnr": -10.0 * np.log10(mse), "si_mse": si_mse, "lmse": lmse, "ssim": ssim, "dssim": (1.0 - ssim) / 2.0}


def finish_image_quality_stack(sums, counts, channels):
    """``{"frames": [one finish_image_quality dict per row], "mean": their plain means}`` - a NaN frame makes its mean NaN."""
    frames = [finish_image_quality(s, n, channels) for s, n in zip(np.asarray(sums), np.asarray(counts))]
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                                              # no frame: NaN, quietly
        mean = {k: np.mean(np.array([f[k] for f in frames], dtype=np.float64)) for k in IMAGE_QUALITY_KEYS}
    return {"frames": frames, "mean": mean}


def split_table(counts, number_classes):
    """(confusion table [C, C], the eight counters) of a read-back ``counts`` vector."""
    counts = np.asarray(counts, dtype=np.int64)
    c = int(number_classes)
    return counts[:c * c].reshape(c, c), counts[c * c:]


def _device_of(*arrays):
    import torch
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda")


def _upload(a, device, tail=()):
    """Any numpy / torch array of any integer or float dtype as a flat fp32 tensor [n, *tail] on ``device`` (labels and 8-bit
    values are exact in fp32; the metric kernels are fp32 like the maps they evaluate)."""
    import torch
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    t = t.detach().to(device=device, dtype=torch.float32)
    return t.reshape(-1, *tail).contiguous()


def calculate_segmentation_metrics(true_labels, predicted_labels, number_classes, ignore_label):
    """training_utils.py:58-84 with the confusion matrix counted on the device: one ``eval_accumulate`` launch, one read-back."""
    from . import kernels
    device = _device_of(true_labels, predicted_labels)
    t, p = _upload(true_labels, device), _upload(predicted_labels, device)
    counts, sums = kernels.eval_tables(number_classes, device)
    kernels.eval_accumulate(counts, sums, number_classes, ignore_label, true_label=t, pred_label=p)
    table, scalars = split_table(counts.cpu().numpy(), number_classes)
    return finish_segmentation(table, scalars[COUNT["n_not_ignored"]])


def calculate_depth_metrics(depth_trgt, depth_pred):
    """training_utils.py:87-122 with the per-pixel terms and their sums on the device (fp32 terms, fp64 sums)."""
    from . import kernels
    device = _device_of(depth_trgt, depth_pred)
    t, p = _upload(depth_trgt, device), _upload(depth_pred, device)
    counts, sums = kernels.eval_tables(1, device)
    kernels.eval_accumulate(counts, sums, 1, depth_pred=p, depth_trgt=t)
    return finish_depth(split_table(counts.cpu().numpy(), 1)[1], sums.cpu().numpy())


def image_mse_psnr(pred, target):
    """``(img2mse(pred, target), mse2psnr(...))`` of two images (any shape ending in 3), finished in float64."""
    from . import kernels
    device = _device_of(pred, target)
    x, y = _upload(pred, device, (3,)), _upload(target, device, (3,))
    counts, sums = kernels.eval_tables(1, device)
    kernels.eval_accumulate(counts, sums, 1, rgb_pred=x, rgb_trgt=y)
    return finish_image(split_table(counts.cpu().numpy(), 1)[1], sums.cpu().numpy())


def _as_images(a, device):
    """An image, a map or a stack of them, numpy or torch, host or device, as an fp32 tensor of the same shape on ``device``; a
    float32 tensor already there is taken as the view it is."""
    import torch
    if not isinstance(a, torch.Tensor):
        a = np.ascontiguousarray(a)
        a = torch.from_numpy(a if a.flags.writeable else a.copy())
    if a.dtype == torch.bool:
        a = a.to(torch.uint8)
    return a.detach().to(device=device, dtype=torch.float32)


def intrinsic_image_metrics(pred, target, mask=None, window_size=20, window_shift=10):
    """mse, psnr, si_mse, lmse, ssim and dssim of ``pred`` against ``target`` (include/inerf.h states the definitions): [H, W, C]
    with C = 1 or 3, [H, W] (read as C = 1) or a stack [N, H, W, C]; ``mask`` [H, W] or [N, H, W], valid where > 0.  One device
    call for the whole stack; returns ``{"frames": [dict per image], "mean": dict}`` (plain means: a NaN stays visible)."""
    from . import kernels
    device = _device_of(pred, target, mask)
    p, g = _as_images(pred, device), _as_images(target, device)
    if p.dim() == 2:
        p, g = p[..., None], g[..., None]
    if p.shape != g.shape:
        raise ValueError(f"pred {tuple(p.shape)} and target {tuple(g.shape)} differ in shape")
    m = None if mask is None else _as_images(mask, device)
    sums, counts = kernels.image_quality(p, g, m, window_size=window_size, window_shift=window_shift)
    return finish_image_quality_stack(sums.cpu().numpy(), counts.cpu().numpy(), p.shape[-1])


class FrameEvaluator:
    """The metrics of a rendered frame set, accumulated on the device one frame at a time.

    ``register(rays, image=, depth=, semantic=)`` ties targets to a frame set by the identity of its ``rays`` object; they are
    uploaded once ([n_frames, H*W(, 3)] fp32) and stay resident.  ``semantic`` may be a dict of named targets, one confusion table
    each (the NYU-CNN trainer evaluates against its clean and its ground-truth labels).  ``begin(rays)`` selects the set and says
    whether it has targets; ``add_frame(i, logits=, depth=, rgb=)`` returns frame i's ``(label, entropy)`` maps and, with
    targets, accumulates in the same launch; ``results()`` reads the tables back and finishes the three metric groups;
    ``reset()`` zeroes them.

    Image quality: ``register(..., albedo=, shading=, mask=, shape=(H, W))`` adds ground-truth albedo / shading stacks and a validity
    mask (> 0); with ``shape`` every one of rgb, albedo and shading that ``add_frame`` is given and that has a target (``image`` for
    rgb) gets its ``kernels.image_quality`` rows, kept on the device per frame; ``results()`` reads them back once and adds the keys
    ``"image_quality"`` (rgb), ``"albedo"`` and ``"shading"``, each ``{"frames": {frame index: dict}, "mean": dict}``, for the
    groups that were seen."""

    def __init__(self, number_classes, ignore_label=-1):
        self.number_classes = int(number_classes)
        self.ignore_label = int(ignore_label)
        self._sets = {}
        self._current = None
        self._tables = {}                 # semantic target name (None: the unnamed one, or none at all) -> (counts, sums)
        self._seen = set()
        self._quality = {}                # results key -> [(frame index, channels, sums [1, 7], counts [1, 3])], device-resident

    def register(self, rays, image=None, depth=None, semantic=None, albedo=None, shading=None, mask=None, shape=None):
        device = _device_of(rays[0] if len(rays) else rays)
        n = len(rays)
        targets = {"rays": rays, "device": device, "image": None, "depth": None, "semantic": {}}
        if image is not None:
            targets["image"] = _upload(image, device, (3,)).reshape(n, -1, 3)
        if depth is not None:
            targets["depth"] = _upload(depth, device).reshape(n, -1)
        if semantic is not None:
            named = semantic if isinstance(semantic, dict) else {None: semantic}
            targets["semantic"] = {name: _upload(s, device).reshape(n, -1) for name, s in named.items()}
        if shape is not None:
            h, w = int(shape[0]), int(shape[1])
            targets["shape"] = (h, w)
            if image is not None and targets["image"].shape[1] != h * w:
                raise ValueError(f"image holds {targets['image'].shape[1]} pixels per frame, shape={shape} says {h * w}")
            for name, a in (("albedo", albedo), ("shading", shading)):
                if a is not None:
                    targets[name] = _upload(a, device).reshape(n, h * w, -1)
            if mask is not None:
                targets["mask"] = _upload(mask, device).reshape(n, h * w)
        elif albedo is not None or shading is not None or mask is not None:
            raise ValueError("albedo / shading / mask targets need shape=(H, W): their metrics are windowed")
        self._sets[id(rays)] = targets   # (the entry holds `rays`, so its id is not reused while registered)

    def begin(self, rays):
        self._current = self._sets.get(id(rays))
        return self._current is not None

    def _table(self, name, device):
        from . import kernels
        if name not in self._tables:
            self._tables[name] = kernels.eval_tables(self.number_classes, device)
        return self._tables[name]

    def _add_image_quality(self, cur, i, preds):
        from . import kernels
        h, w = cur["shape"]
        for (key, keyword, target), pred in zip(IMAGE_QUALITY_GROUPS, preds):
            if pred is None or cur.get(target) is None:
                continue
            g = cur[target][i]
            p = pred.reshape(h * w, -1) if pred.dim() != 2 or pred.shape[0] != h * w else pred
            sums, counts = kernels.image_quality(p, g, None if cur.get("mask") is None else cur["mask"][i], shape=(h, w))
            self._quality.setdefault(key, []).append((int(i), int(g.shape[-1]), sums, counts))

    def add_frame(self, i, logits=None, depth=None, rgb=None, albedo=None, shading=None):
        from . import kernels
        cur = self._current
        if cur is None:
            return kernels.sem_maps(logits) if logits is not None else (None, None)
        if cur.get("shape") is not None:
            self._add_image_quality(cur, i, (rgb, albedo, shading))
        names = list(cur["semantic"]) if logits is not None else []
        first = names[0] if names else None
        groups = {}
        if names:
            groups["true_label"] = cur["semantic"][first][i]
        if depth is not None and cur["depth"] is not None:
            groups["depth_pred"], groups["depth_trgt"] = depth.reshape(-1), cur["depth"][i]
            self._seen.add("depth")
        if rgb is not None and cur["image"] is not None:
            groups["rgb_pred"], groups["rgb_trgt"] = rgb.reshape(-1, 3), cur["image"][i]
            self._seen.add("image")
        if not groups:
            return kernels.sem_maps(logits) if logits is not None else (None, None)
        # depth and rgb ride with the first semantic target's launch, in that target's table (results() adds them up over tables)
        counts, sums = self._table(first, cur["device"])
        label, entropy = kernels.eval_accumulate(counts, sums, self.number_classes, self.ignore_label, logits=logits, **groups)
        for name in names[1:]:
            c2, s2 = self._table(name, cur["device"])
            kernels.eval_accumulate(c2, s2, self.number_classes, self.ignore_label, pred_label=label, true_label=cur["semantic"][name][i])
        self._seen.update(("semantic", n) for n in names)
        return label, entropy

    def results(self):
        """``{"segmentation": {name: 5-tuple}, "depth": dict | None, "image": (mse, psnr) | None}``; a single unnamed semantic
        target is under the key ``None``.  With image-quality rows (class docstring) also ``"image_quality"`` / ``"albedo"`` /
        ``"shading"``, each present only when its group was seen."""
        out = {"segmentation": {}, "depth": None, "image": None}
        scalars_all, sums_all = np.zeros(_capi.EVAL_COUNTS, dtype=np.int64), np.zeros(_capi.EVAL_SUMS, dtype=np.float64)
        for name, (counts, sums) in self._tables.items():
            table, scalars = split_table(counts.cpu().numpy(), self.number_classes)
            if ("semantic", name) in self._seen:
                out["segmentation"][name] = finish_segmentation(table, scalars[COUNT["n_not_ignored"]])
            scalars_all += scalars
            sums_all += sums.cpu().numpy()
        if "depth" in self._seen:
            out["depth"] = finish_depth(scalars_all, sums_all)
        if "image" in self._seen:
            out["image"] = finish_image(scalars_all, sums_all)
        if self._quality:
            import torch
            for key, rows in self._quality.items():
                sums = torch.cat([r[2] for r in rows], 0).cpu().numpy()                 # one read-back per group
                counts = torch.cat([r[3] for r in rows], 0).cpu().numpy()
                stack = finish_image_quality_stack(sums, counts, rows[0][1])
                out[key] = {"frames": {r[0]: f for r, f in zip(rows, stack["frames"])}, "mean": stack["mean"]}
        return out

    def tables(self):
        """``{name: (counts, sums)}``: the device-resident accumulators."""
        return dict(self._tables)

    def reset(self):
        for counts, sums in self._tables.values():
            counts.zero_()
            sums.zero_()
        self._seen.clear()
        self._quality.clear()
