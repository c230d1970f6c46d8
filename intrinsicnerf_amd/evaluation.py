"""Validation metrics of the SSR trainer on the device (csrc/eval.hip): the reference's ``calculate_segmentation_metrics`` and
``calculate_depth_metrics`` (SSR/training/training_utils.py:58-122) and ``img2mse`` / ``mse2psnr`` under their own names and
signatures, and ``FrameEvaluator``, which accumulates them frame by frame beside the render that produced their inputs.

One ``kernels.eval_accumulate`` pass reduces the pixels to an int64 table (the confusion matrix and eight counters) and six
fp64 sums; what remains - normalised rows, the masked means, the ious, a few quotients and square roots - is finished on the
host in float64 numpy by ``finish_segmentation`` / ``finish_depth``, which need no device.  The reference's ``np.float``
(removed in numpy 1.24) is read as ``float``.
"""
import warnings

import numpy as np

from . import _capi

COUNT = {name: i for i, name in enumerate(_capi.EVAL_COUNT_NAMES)}
SUM = {name: i for i, name in enumerate(_capi.EVAL_SUM_NAMES)}
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


class FrameEvaluator:
    """The metrics of a rendered frame set, accumulated on the device one frame at a time.

    ``register(rays, image=, depth=, semantic=)`` ties targets to a frame set by the identity of its ``rays`` object; they are
    uploaded once ([n_frames, H*W(, 3)] fp32) and stay resident.  ``semantic`` may be a dict of named targets, one confusion table
    each (the NYU-CNN trainer evaluates against its clean and its ground-truth labels).  ``begin(rays)`` selects the set and says
    whether it has targets; ``add_frame(i, logits=, depth=, rgb=)`` returns frame i's ``(label, entropy)`` maps and, with
    targets, accumulates in the same launch; ``results()`` reads the tables back and finishes the three metric groups;
    ``reset()`` zeroes them."""

    def __init__(self, number_classes, ignore_label=-1):
        self.number_classes = int(number_classes)
        self.ignore_label = int(ignore_label)
        self._sets = {}
        self._current = None
        self._tables = {}                 # semantic target name (None: the unnamed one, or none at all) -> (counts, sums)
        self._seen = set()

    def register(self, rays, image=None, depth=None, semantic=None):
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
        self._sets[id(rays)] = targets   # (the entry holds `rays`, so its id is not reused while registered)

    def begin(self, rays):
        self._current = self._sets.get(id(rays))
        return self._current is not None

    def _table(self, name, device):
        from . import kernels
        if name not in self._tables:
            self._tables[name] = kernels.eval_tables(self.number_classes, device)
        return self._tables[name]

    def add_frame(self, i, logits=None, depth=None, rgb=None):
        from . import kernels
        cur = self._current
        if cur is None:
            return kernels.sem_maps(logits) if logits is not None else (None, None)
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
        target is under the key ``None``."""
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
        return out

    def tables(self):
        """``{name: (counts, sums)}``: the device-resident accumulators."""
        return dict(self._tables)

    def reset(self):
        for counts, sums in self._tables.values():
            counts.zero_()
            sums.zero_()
        self._seen.clear()
