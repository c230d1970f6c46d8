"""Cases and judges of the validation-metric tests (csrc/eval.hip, intrinsicnerf_amd/evaluation.py).

The three routines the kernels stand in for - SSR/training/training_utils.py's ``calculate_segmentation_metrics`` and
``calculate_depth_metrics`` and ``img2mse`` - are restated here in this project's own words: ``confusion`` counts the table
(sklearn's ``confusion_matrix`` when it is importable, checked against the ``np.add.at`` table used otherwise),
``segmentation_from_table`` / ``depth_from_table`` do the float64 finishing, ``depth_terms`` evaluates the per-pixel terms with
numpy in fp32 the way the reference's expressions do.  Logit cases are built so that "the lowest index of the maximum" and
torch's ``argmax(softmax(x))`` must agree on every row (test_evaluation_cpu.py checks it with a cap of zero): ``randn * 3`` with
the top-two gap forced to at least 1e-3, rows with a bitwise tie at the last index and at index 0, and rows with NaN, +inf, all
-inf and a single -inf.
"""
import warnings
from functools import lru_cache

import numpy as np
import torch

N_SIZES = (1, 63, 64, 65, 255, 256, 257, 4099)
CLASSES = (1, 2, 3, 28, 63, 64, 65, 240)            # 63 | 64 | 65: either side of the LDS / global-atomic switch of the table
SECOND_TRIP_N = 512 * 256 + 65                      # the accumulate grid is capped at 512 workgroups of 256 pixels
COUNT_NAMES = ("n_not_ignored", "n_pixels", "n_pred_positive", "n_mask", "r1", "r2", "r3", "n_rgb")
SUM_NAMES = ("abs_rel", "abs_diff", "sq_rel", "sq_diff", "sq_log_diff", "rgb_sq")
EPS21 = 2.0 ** -21


# ---- logits ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def logit_case(n, n_classes, seed=0):
    """[n, C] fp32 CPU logits.  The last rows are the special ones when n leaves room (n >= 8): NaN, +inf, all -inf, one -inf;
    before them min(50, n // 4) rows tied bitwise at the last index and as many tied at index 0."""
    g = torch.Generator().manual_seed(1000 * n_classes + n + 7919 * seed)
    x = torch.randn(n, n_classes, generator=g) * 3
    if n_classes > 1:
        top = torch.topk(x, 2, dim=-1)
        close = (top.values[:, 0] - top.values[:, 1]) < 1e-3
        x[close, top.indices[close, 0]] += 4e-3                 # the gap of every row is now >= 1e-3
        top = torch.topk(x, 2, dim=-1)
        assert bool(((top.values[:, 0] - top.values[:, 1]) >= 1e-3).all())
    special = 4 if n >= 8 else 0
    ties = min(50, (n - special) // 4)
    body = n - special - 2 * ties
    for r in range(body, body + ties):
        x[r, n_classes - 1] = x[r].max()
    for r in range(body + ties, body + 2 * ties):
        x[r, 0] = x[r].max()
    if special:
        r = n - 4
        x[r, n_classes // 2] = float("nan")
        x[r + 1, n_classes - 1] = float("inf")
        x[r + 2, :] = float("-inf")
        if n_classes > 1:
            x[r + 3, 0] = float("-inf")
    return x


def lowest_index_of_maximum(x):
    """The kernel's label rule on the CPU: the lowest index that attains the row's maximum; 0 for a row that holds a NaN or
    whose maximum is not finite."""
    a = x.numpy()
    out = np.zeros(a.shape[0], dtype=np.int64)
    for r in range(a.shape[0]):
        row = a[r]
        m = row.max() if not np.isnan(row).any() else np.nan
        out[r] = int(np.flatnonzero(row == m)[0]) if np.isfinite(m) else 0
    return out


@lru_cache(maxsize=None)
def logit_reference(n, n_classes, seed=0):
    """(label, H32, H64, D) of a logit case on the CPU: torch's ``argmax(softmax(x))``, the reference's entropy expression in fp32
    and in fp64, and D = the largest error of the fp32 one over the rows where both are finite."""
    x = logit_case(n, n_classes, seed)
    F = torch.nn.functional
    label = torch.argmax(F.softmax(x, dim=-1), dim=-1).numpy()
    h32 = torch.sum(-F.log_softmax(x, dim=-1) * F.softmax(x, dim=-1), dim=-1).numpy()
    xd = x.double()
    h64 = torch.sum(-F.log_softmax(xd, dim=-1) * F.softmax(xd, dim=-1), dim=-1).numpy()
    fin = np.isfinite(h32) & np.isfinite(h64)
    d = float(np.abs(h32[fin].astype(np.float64) - h64[fin]).max()) if fin.any() else 0.0
    return label, h32, h64, d


def entropy_judgement(got, n, n_classes, seed=0):
    """(worst err / bound, message or None): |got - H64| <= 4 D + 2^-21 max(1, |H64|), NaN exactly where the reference has NaN."""
    _, h32, h64, d = logit_reference(n, n_classes, seed)
    got = np.asarray(got, dtype=np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(h32)):
        return float("inf"), f"NaN pattern differs on rows {np.flatnonzero(np.isnan(got) != np.isnan(h32))[:8]}"
    fin = ~np.isnan(h32)
    if not fin.any():
        return 0.0, None
    bound = 4 * d + EPS21 * np.maximum(1.0, np.abs(h64[fin]))
    ratio = float((np.abs(got[fin] - h64[fin]) / bound).max())
    return ratio, None if ratio <= 1.0 else f"entropy err / bound = {ratio:.3f} (D = {d:.3e})"


# ---- the restated metric routines -----------------------------------------------------------------------------------------------
def _integral_in_range(v, n_classes):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (v >= 0) & (v < n_classes) & (v == np.floor(v))


def confusion(true, pred, n_classes):
    """The table sklearn.metrics.confusion_matrix(true, pred, labels=range(C)) gives: row = true, column = predicted, a pair
    counted only when both labels are among range(C).  Labels that are no integers (or NaN) can be no member of range(C)."""
    true, pred = np.asarray(true).reshape(-1), np.asarray(pred).reshape(-1)
    keep = _integral_in_range(true, n_classes) & _integral_in_range(pred, n_classes)
    table = np.zeros((n_classes, n_classes), dtype=np.int64)
    np.add.at(table, (true[keep].astype(np.int64), pred[keep].astype(np.int64)), 1)
    try:
        from sklearn.metrics import confusion_matrix
    except ImportError:
        return table
    whole = np.isfinite(true.astype(np.float64)) & np.isfinite(pred.astype(np.float64))
    whole &= (true == np.floor(true)) & (pred == np.floor(pred))            # sklearn refuses continuous targets outright
    t, p = true[whole].astype(np.int64), pred[whole].astype(np.int64)
    if np.isin(t, np.arange(n_classes)).any():                              # (and a label list of which y_true holds none)
        with warnings.catch_warnings():                                     # (its remarks on few samples / a single label)
            warnings.simplefilter("ignore")
            theirs = confusion_matrix(t, p, labels=list(range(n_classes)))
        assert np.array_equal(theirs, table), "the np.add.at table and sklearn's differ"
    return table


def segmentation_from_table(table, n_not_ignored):
    """What the reference returns once it holds the table: four zeros when every true label is ignored, else mean IoU over the
    classes whose IoU is a number, mean IoU over the classes that occur as a true label, overall accuracy, mean per-class
    accuracy over the classes that occur, and the IoU vector."""
    if n_not_ignored == 0:
        return [0] * 4
    table = np.asarray(table, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        row_total = table.astype(float).sum(axis=1)
        recall_rows = (table.T / row_total).T
        occurs = ~np.isnan(recall_rows.sum(1))
        class_average_accuracy = np.ma.masked_invalid(np.diagonal(recall_rows)).mean()
        total_accuracy = np.trace(table) / table.sum()
        ious = np.zeros(table.shape[0])
        for k in range(table.shape[0]):
            ious[k] = table[k, k] / (table[k, :].sum() + table[:, k].sum() - table[k, k])
        with warnings.catch_warnings():                                     # (np.mean of no class at all: NaN, and a remark)
            warnings.simplefilter("ignore")
            valid_mean = np.mean(ious[occurs])
        return np.ma.masked_invalid(ious).mean(), valid_mean, total_accuracy, class_average_accuracy, ious


def depth_from_table(counts, sums):
    c, s = dict(zip(COUNT_NAMES, np.asarray(counts, dtype=np.int64))), dict(zip(SUM_NAMES, np.asarray(sums, dtype=np.float64)))
    m = np.float64(c["n_mask"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"AbsRel": s["abs_rel"] / m, "AbsDiff": s["abs_diff"] / m, "SqRel": s["sq_rel"] / m, "RMSE": np.sqrt(s["sq_diff"] / m),
                "LogRMSE": np.sqrt(s["sq_log_diff"] / m), "r1": c["r1"] / m, "r2": c["r2"] / m, "r3": c["r3"] / m,
                "complete": np.float64(c["n_pred_positive"]) / np.float64(c["n_pixels"])}


def same_bits(a, b):
    """Two metric values (floats, arrays, np.ma.masked, lists) equal bit for bit."""
    if a is np.ma.masked or b is np.ma.masked:
        return a is b
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_metrics(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same_bits(a[k], b[k]) for k in a)
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def depth_terms(trgt, pred):
    """The reference's per-pixel depth terms with numpy in fp32 (training_utils.py:96-109): the counters, the float64 sums of the
    fp32 terms, and for the log term its fp64 evaluation on the fp32 inputs with D' = the error of the fp32 sum against it."""
    t, p = np.asarray(trgt, dtype=np.float32).reshape(-1), np.asarray(pred, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        pos = p > 0
        mask = (t < 10) * (t > 0) * pos
        pm, tm = p[mask], t[mask]
        ad = np.abs(pm - tm)
        sq = ad ** 2
        thr = np.maximum(tm / pm, pm / tm)
        lg = (np.log(pm) - np.log(tm)) ** 2
        lg64 = (np.log(pm.astype(np.float64)) - np.log(tm.astype(np.float64))) ** 2
    assert ad.dtype == sq.dtype == thr.dtype == lg.dtype == np.float32
    counts = {"n_pixels": t.size, "n_pred_positive": int(pos.sum()), "n_mask": int(mask.sum()), "r1": int((thr < 1.25).sum()),
              "r2": int((thr < 1.25 ** 2).sum()), "r3": int((thr < 1.25 ** 3).sum())}
    f64 = lambda v: float(np.sum(v, dtype=np.float64))
    sums = {"abs_rel": f64(ad / tm), "abs_diff": f64(ad), "sq_rel": f64(sq / tm), "sq_diff": f64(sq)}
    want_log = f64(lg64)
    return counts, sums, want_log, abs(f64(lg) - want_log)


def rgb_terms(x, y):
    x, y = np.asarray(x, dtype=np.float32).reshape(-1), np.asarray(y, dtype=np.float32).reshape(-1)
    return x.size, float(np.sum((x - y) ** 2, dtype=np.float64))


# ---- accumulate cases -----------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def label_case(n, n_classes, kind="mixed", ignore=-1):
    """(true, pred) fp32 CPU vectors.  "mixed": uniform over [ignore .. C) x [0 .. C) with, when n leaves room, labels outside
    [0, C) on either side, non-integers and NaNs sprinkled in; "one_pair": every pixel (C - 1, 0), the contention worst case;
    "ignored": every true label ignored; "out_of_range": valid pixels that are all outside the table."""
    g = torch.Generator().manual_seed(31 * n + n_classes)
    if kind == "one_pair":
        return torch.full((n,), float(n_classes - 1)), torch.zeros(n)
    if kind == "ignored":
        return torch.full((n,), float(ignore)), torch.randint(0, n_classes, (n,), generator=g).float()
    if kind == "out_of_range":
        return torch.full((n,), float(n_classes)), torch.randint(0, n_classes, (n,), generator=g).float()
    t = torch.randint(-1, n_classes, (n,), generator=g).float()
    t[t < 0] = float(ignore)
    p = torch.randint(0, n_classes, (n,), generator=g).float()
    if n >= 64:
        odd = [float(n_classes), float(n_classes + 3), -2.0, 0.5, float("nan"), 1e9, -0.5, float("inf")]
        for j, v in enumerate(odd):
            t[3 + 7 * j] = v                    # rows 3, 10, ...: the true side
            p[5 + 7 * j] = v                    # rows 5, 12, ...: the predicted side
    return t, p


@lru_cache(maxsize=None)
def depth_case(n):
    """(trgt, pred) fp32 CPU vectors: targets over (0, 12) so that some exceed 10, predictions around them; when n leaves room the
    edges of the mask (0, 10, negative, NaN on either side) and ratios exactly at, one ulp below and one ulp above 1.25, 1.5625
    and 1.953125 in both directions."""
    g = torch.Generator().manual_seed(77 + n)
    t = torch.rand(n, generator=g) * 12 + 1e-3
    p = t * (0.5 + 1.2 * torch.rand(n, generator=g))
    if n >= 64:
        edges = [(0.0, 1.0), (10.0, 9.0), (-1.0, 1.0), (float("nan"), 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, float("nan")), (9.999999, 5.0)]
        for thr in (1.25, 1.5625, 1.953125):
            for v in (thr, float(np.nextafter(np.float32(thr), np.float32(0))), float(np.nextafter(np.float32(thr), np.float32(4)))):
                edges += [(1.0, v), (v, 1.0)]
        for j, (tv, pv) in enumerate(edges):
            t[2 * j + 1], p[2 * j + 1] = tv, pv
    return t, p


@lru_cache(maxsize=None)
def rgb_case(n):
    g = torch.Generator().manual_seed(5 + n)
    return torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)


def reference_counts(n_classes, ignore, true=None, pred=None, depth=None, rgb=None):
    """The int64 vector an accumulate pass must leave: the C x C table then the eight counters; and the sums it is judged against."""
    table = np.zeros((n_classes, n_classes), dtype=np.int64)
    scalars = dict.fromkeys(COUNT_NAMES, 0)
    sums, want_log, d_log = {}, 0.0, 0.0
    if true is not None:
        t, p = np.asarray(true, dtype=np.float32), np.asarray(pred, dtype=np.float32)
        valid = t != np.float32(ignore)
        scalars["n_not_ignored"] = int(valid.sum())
        table = confusion(t[valid], p[valid], n_classes)
    if depth is not None:
        c, sums, want_log, d_log = depth_terms(*depth)
        scalars.update(c)
    if rgb is not None:
        scalars["n_rgb"], sums["rgb_sq"] = rgb_terms(*rgb)
    counts = np.concatenate([table.reshape(-1), np.array([scalars[k] for k in COUNT_NAMES], dtype=np.int64)])
    return counts, sums, want_log, d_log


def sums_judgement(got, n, sums, want_log, d_log):
    """Messages for every sum outside its bound: the exact terms within relative n 2^-52 of numpy's float64 sum (the terms are
    bitwise equal and two fp64 sums of n non-negative terms err by at most (n - 1) 2^-53 each), the log term within
    4 D' + 2^-21 |want| of its fp64 evaluation."""
    got = dict(zip(SUM_NAMES, np.asarray(got, dtype=np.float64)))
    bad = []
    for k, want in sums.items():
        if abs(got[k] - want) > n * 2.0 ** -52 * abs(want):
            bad.append(f"{k}: got {got[k]!r}, want {want!r}")
    if "abs_rel" in sums and abs(got["sq_log_diff"] - want_log) > 4 * d_log + EPS21 * abs(want_log):
        bad.append(f"sq_log_diff: got {got['sq_log_diff']!r}, want {want_log!r} (D' = {d_log:.3e})")
    return bad
