"""A/B partners of scripts/bench_evaluation.py: what the validation step does WITHOUT csrc/eval.hip.

``torch_sem_maps`` is the four lines of ssr.SSRRenderMixin.render_path that compute the label and entropy maps with torch
(six launches, [H*W, C] temporaries).  ``host_segmentation`` / ``host_depth`` restate the reference's two metric functions on host
arrays with sklearn and numpy - the work the reference's trainer does at every validation step (its own
``calculate_segmentation_metrics`` cannot run on a numpy >= 1.24: ``np.float``).  ``torch_accumulate`` counts the same tables
with torch ops on the device (bincount and masked sums): the obvious eager alternative to the accumulate kernel.
"""
import numpy as np
import torch
import torch.nn.functional as F


def torch_sem_maps(logits):
    logp = F.log_softmax(logits, dim=-1)
    label = torch.argmax(F.softmax(logits, dim=-1), dim=-1).float()
    entropy = torch.sum(-logp * F.softmax(logits, dim=-1), dim=-1)
    return label, entropy


def host_segmentation(true_labels, predicted_labels, number_classes, ignore_label):
    true_labels, predicted_labels = true_labels.flatten(), predicted_labels.flatten()
    if (true_labels == ignore_label).all():
        return [0] * 4
    valid = true_labels != ignore_label
    t, p = true_labels[valid], predicted_labels[valid]
    try:
        from sklearn.metrics import confusion_matrix
        conf = confusion_matrix(t, p, labels=list(range(number_classes)))
    except ImportError:
        keep = (t >= 0) & (t < number_classes) & (p >= 0) & (p < number_classes)
        conf = np.zeros((number_classes, number_classes), dtype=np.int64)
        np.add.at(conf, (t[keep].astype(np.int64), p[keep].astype(np.int64)), 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = (conf.T / conf.astype(float).sum(axis=1)).T
        occurs = ~np.isnan(norm.sum(1))
        class_acc = np.ma.masked_invalid(np.diagonal(norm)).mean()
        acc = np.trace(conf) / conf.sum()
        ious = np.array([conf[k, k] / (conf[k, :].sum() + conf[:, k].sum() - conf[k, k]) for k in range(number_classes)])
        return np.ma.masked_invalid(ious).mean(), np.mean(ious[occurs]), acc, class_acc, ious


def host_depth(depth_trgt, depth_pred):
    pos = depth_pred > 0
    mask = (depth_trgt < 10) * (depth_trgt > 0) * pos
    p, t = depth_pred[mask], depth_trgt[mask]
    ad = np.abs(p - t)
    sq = ad ** 2
    thr = np.maximum(t / p, p / t)
    return {"AbsRel": np.mean(ad / t), "AbsDiff": np.mean(ad), "SqRel": np.mean(sq / t), "RMSE": np.sqrt(np.mean(sq)),
            "LogRMSE": np.sqrt(np.mean((np.log(p) - np.log(t)) ** 2)), "r1": np.mean((thr < 1.25).astype("float")),
            "r2": np.mean((thr < 1.25 ** 2).astype("float")), "r3": np.mean((thr < 1.25 ** 3).astype("float")),
            "complete": np.mean(pos.astype("float"))}


def torch_accumulate(n_classes, ignore, true, pred, depth_trgt, depth_pred):
    """(table [C, C] int64, [n_pixels, n_pred_positive, n_mask, r1, r2, r3] int64, five fp64 sums) with eager torch on the device."""
    valid = true != ignore
    t, p = true[valid].long(), pred[valid].long()
    keep = (t >= 0) & (t < n_classes) & (p >= 0) & (p < n_classes)
    table = torch.bincount(t[keep] * n_classes + p[keep], minlength=n_classes * n_classes).reshape(n_classes, n_classes)
    pos = depth_pred > 0
    mask = (depth_trgt < 10) & (depth_trgt > 0) & pos
    dp, dt = depth_pred[mask], depth_trgt[mask]
    ad = (dp - dt).abs()
    sq = ad * ad
    thr = torch.maximum(dt / dp, dp / dt)
    lg = (dp.log() - dt.log()) ** 2
    counts = torch.stack([torch.tensor(true.numel(), device=true.device), pos.sum(), mask.sum(), (thr < 1.25).sum(), (thr < 1.5625).sum(),
                          (thr < 1.953125).sum()])
    sums = torch.stack([(ad / dt).double().sum(), ad.double().sum(), (sq / dt).double().sum(), sq.double().sum(), lg.double().sum()])
    return table, counts, sums
