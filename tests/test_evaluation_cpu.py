"""Validation metrics without a device: the ABI number, the host finishing of ``intrinsicnerf_amd.evaluation`` against the
restatement of the reference (_evaluation.py) bit for bit, the fairness of the logit cases the GPU tests use (torch's
``argmax(softmax(x))`` and "the lowest index of the maximum" agree on EVERY row: the cap on rows left out is zero), the launchers'
argument checks, and ``--inerf-eval``'s rebinding."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import _evaluation as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_number_agrees_and_covers_the_evaluation_entry_points():
    from intrinsicnerf_amd import _capi as capi
    with open(os.path.join(REPO, "include", "inerf.h")) as fh:
        text = fh.read()
    header = int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1))
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version() and header >= 40020
    for name in ("inerf_sem_maps", "inerf_eval_accumulate", "inerf_eval_workspace_bytes"):
        assert name in capi.SYMBOLS and re.search(r"\b%s\(" % name, text)
    assert capi.EVAL_COUNT_NAMES == V.COUNT_NAMES and capi.EVAL_SUM_NAMES == V.SUM_NAMES
    for i, name in enumerate(V.COUNT_NAMES):
        assert re.search(r"#define INERF_EVAL_%s\s+%d\b" % (name.upper(), i), text), name
    for i, name in enumerate(V.SUM_NAMES):
        assert re.search(r"#define INERF_EVAL_%s\s+%d\b" % (name.upper(), i), text), name
    assert capi.lib().inerf_eval_workspace_bytes(0) == 0 and capi.lib().inerf_eval_workspace_bytes(1) == 48
    assert capi.lib().inerf_eval_workspace_bytes(1 << 30) == 512 * 48            # the grid cap


def _tables():
    rng = np.random.default_rng(3)
    full = rng.integers(0, 50, size=(5, 5)).astype(np.int64)
    missing = full.copy(); missing[2, :] = 0                        # class 2 never true: a NaN row
    never_true = np.zeros((4, 4), dtype=np.int64); never_true[0, 0], never_true[0, 3], never_true[1, 1] = 7, 2, 5     # 3 predicted, never true
    return {"full": (full, int(full.sum())), "missing class": (missing, int(missing.sum())), "predicted never true": (never_true, 14),
            "one class": (np.array([[9]], dtype=np.int64), 9), "all ignored": (np.zeros((3, 3), dtype=np.int64), 0),
            "all out of range": (np.zeros((3, 3), dtype=np.int64), 11), "one class, out of range": (np.zeros((1, 1), dtype=np.int64), 4)}


@pytest.mark.parametrize("name", list(_tables()))
def test_finish_segmentation_equals_the_restatement_bit_for_bit(name):
    from intrinsicnerf_amd import evaluation
    table, n = _tables()[name]
    got, want = evaluation.finish_segmentation(table, n), V.segmentation_from_table(table, n)
    assert V.same_metrics(got, want), (got, want)
    if n == 0:
        assert got == [0, 0, 0, 0]                                   # four items: the reference's quirk
    else:
        assert len(got) == 5
    if name == "missing class":
        assert got[4][2] == 0 and got[1] == np.mean(np.delete(got[4], 2)) and got[1] != got[0]        # its normalised row is NaN: left out of the valid-class mean
    if name == "all out of range":
        assert got[0] is np.ma.masked and np.isnan(got[2])


def test_finish_segmentation_on_a_counted_table():
    """From labels to metrics through the restated table: hand-checked values on a 2-class case."""
    from intrinsicnerf_amd import evaluation
    true, pred = np.array([0, 0, 1, 1, -1, 1]), np.array([0, 1, 1, 1, 0, 0])
    valid = true != -1
    table = V.confusion(true[valid], pred[valid], 2)
    assert table.tolist() == [[1, 1], [1, 2]]
    miou, miou_valid, acc, class_acc, ious = evaluation.finish_segmentation(table, int(valid.sum()))
    assert ious.tolist() == [1 / 3, 2 / 4] and acc == 3 / 5 and miou == miou_valid == np.mean([1 / 3, 0.5]) and class_acc == np.mean([0.5, 2 / 3])


@pytest.mark.parametrize("counts,sums", [((100, 120, 110, 90, 40, 70, 85, 360), (3.5, 7.25, 1.125, 9.0, 0.75, 2.5)),
                                         ((0, 64, 0, 0, 0, 0, 0, 0), (0.0,) * 6),          # an empty mask: NaN
                                         ((0, 0, 0, 0, 0, 0, 0, 0), (0.0,) * 6)])          # no pixel at all
def test_finish_depth_equals_the_restatement_bit_for_bit(counts, sums):
    from intrinsicnerf_amd import evaluation
    got, want = evaluation.finish_depth(counts, sums), V.depth_from_table(counts, sums)
    assert list(got) == list(evaluation.DEPTH_KEYS) == ["AbsRel", "AbsDiff", "SqRel", "RMSE", "LogRMSE", "r1", "r2", "r3", "complete"]
    assert V.same_metrics(got, want), (got, want)
    assert all(isinstance(v, (float, np.float64)) for v in got.values())
    if counts[3] == 0:
        assert all(np.isnan(got[k]) for k in ("AbsRel", "RMSE", "r1"))
    mse, psnr = evaluation.finish_image(counts, sums)
    if counts[7]:
        assert mse == sums[5] / counts[7] and psnr == -10.0 * np.log(mse) / np.log(10.0)


@pytest.mark.parametrize("n_classes", V.CLASSES)
def test_logit_cases_are_fair(n_classes):
    """On every row of every label case torch's CPU argmax(softmax(x)) IS the lowest index of the maximum - nothing is left out -
    and D, the fp32 error of the reference's entropy expression against fp64, is printed for every case."""
    for n in V.N_SIZES:
        x = V.logit_case(n, n_classes)
        label, h32, h64, d = V.logit_reference(n, n_classes)
        mismatches = int((label != V.lowest_index_of_maximum(x)).sum())
        print(f"C = {n_classes:3d}  n = {n:5d}  label mismatches {mismatches}  D = {d:.3e}")
        assert mismatches == 0
        assert np.array_equal(np.isnan(h32), np.isnan(h64))
        if n >= 8:                                                  # the special rows: NaN, +inf, all -inf -> label 0, entropy NaN
            assert label[n - 4:n - 1].tolist() == [0, 0, 0] and np.isnan(h32[n - 4:n - 1]).all()
            if n_classes > 1:
                assert np.isnan(h32[n - 1]) and label[n - 1] > 0    # one -inf at index 0: the label stays, the entropy is NaN
        assert d < 2e-6


def test_launchers_name_the_argument_they_reject():
    from intrinsicnerf_amd import kernels
    x = torch.zeros(8, 5)
    with pytest.raises(ValueError, match="n_classes=241"):
        kernels.sem_maps(torch.zeros(2, 241))
    with pytest.raises(ValueError, match="n_classes=0"):
        kernels.eval_tables(0, "cpu")
    with pytest.raises(ValueError, match="logits must be a \\[n, C\\]"):
        kernels.sem_maps(torch.zeros(8))
    with pytest.raises(ValueError, match="logits must be float32"):
        kernels.sem_maps(x.double())
    with pytest.raises(ValueError, match="logits must have unit stride"):
        kernels.sem_maps(torch.zeros(5, 8).t())
    with pytest.raises(ValueError, match="label has a row stride of 0"):
        kernels.sem_maps(x, label=torch.zeros(1).expand(8))
    with pytest.raises(ValueError, match="entropy holds 7 rows, expected 8"):
        kernels.sem_maps(x, entropy=torch.zeros(7))
    with pytest.raises(ValueError, match="label is on meta, expected cpu"):
        kernels.sem_maps(x, label=torch.zeros(8, device="meta"))
    with pytest.raises(RuntimeError, match="logits lives on cpu"):
        kernels.sem_maps(x)
    counts, sums = kernels.eval_tables(5, "cpu")
    with pytest.raises(ValueError, match="counts must be a contiguous torch.int64 vector of 33"):
        kernels.eval_accumulate(counts[:-1], sums, 5, true_label=torch.zeros(8), pred_label=torch.zeros(8))
    with pytest.raises(ValueError, match="logits must be a \\[n, 5\\]"):
        kernels.eval_accumulate(counts, sums, 5, logits=torch.zeros(8, 4))
    with pytest.raises(ValueError, match="rgb_trgt has a row stride of 2 floats, smaller than its width 3"):
        kernels.eval_accumulate(counts, sums, 5, rgb_pred=torch.zeros(8, 3), rgb_trgt=torch.zeros(32).as_strided((8, 3), (2, 1)))
    with pytest.raises(ValueError, match="depth_pred and depth_trgt go together"):
        kernels.eval_accumulate(counts, sums, 5, depth_pred=torch.zeros(8))
    with pytest.raises(ValueError, match="true_label needs a prediction"):
        kernels.eval_accumulate(counts, sums, 5, true_label=torch.zeros(8))
    with pytest.raises(ValueError, match="pred_label holds 9 rows, expected 8"):
        kernels.eval_accumulate(counts, sums, 5, true_label=torch.zeros(8), pred_label=torch.zeros(9))
    with pytest.raises(ValueError, match="depth_trgt is on meta, expected cpu"):
        kernels.eval_accumulate(counts, sums, 5, depth_pred=torch.zeros(8), depth_trgt=torch.zeros(8, device="meta"))
    with pytest.raises(RuntimeError, match="counts lives on cpu"):
        kernels.eval_accumulate(counts, sums, 5, true_label=torch.zeros(8), pred_label=torch.zeros(8))


def test_the_library_rejects_bad_arguments_before_touching_a_device():
    """The C entry points themselves: class count, negative n and strides smaller than their width return their codes (no
    device is needed to be told so); n = 0 is a no-op."""
    import ctypes as C
    from intrinsicnerf_amd import _capi as capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.inerf_sem_maps(p, 5, 4, 0, p, 1, p, 1, None) == capi.E_UNSUPPORTED
    assert lib.inerf_sem_maps(p, 241, 4, 241, p, 1, p, 1, None) == capi.E_UNSUPPORTED
    assert lib.inerf_sem_maps(p, 5, -1, 5, p, 1, p, 1, None) == capi.E_INVALID
    assert lib.inerf_sem_maps(p, 4, 4, 5, p, 1, p, 1, None) == capi.E_INVALID
    assert lib.inerf_sem_maps(p, 5, 4, 5, p, 0, p, 1, None) == capi.E_INVALID
    assert lib.inerf_sem_maps(p, 5, 0, 5, p, 1, p, 1, None) == capi.OK
    a = capi.EvalArgs()
    a.n, a.n_classes, a.ignore_label = 4, 5, -1
    a.true_label, a.true_label_stride, a.pred_label, a.pred_label_stride = p.value, 1, p.value, 1
    a.counts, a.sums, a.workspace, a.workspace_bytes = p.value, p.value, p.value, 48
    for field, value, code in (("n_classes", 0, capi.E_UNSUPPORTED), ("n_classes", 241, capi.E_UNSUPPORTED), ("n", -1, capi.E_INVALID),
                               ("true_label_stride", 0, capi.E_INVALID), ("pred_label_stride", 0, capi.E_INVALID),
                               ("workspace_bytes", 40, capi.E_WORKSPACE)):
        saved = getattr(a, field)
        setattr(a, field, value)
        assert lib.inerf_eval_accumulate(C.byref(a), None) == code, field
        setattr(a, field, saved)
    a.rgb_pred, a.rgb_trgt, a.rgb_pred_stride, a.rgb_trgt_stride = p.value, p.value, 3, 2
    assert lib.inerf_eval_accumulate(C.byref(a), None) == capi.E_INVALID
    a.rgb_trgt_stride, a.n = 3, 0
    assert lib.inerf_eval_accumulate(C.byref(a), None) == capi.OK


STAND_IN = {
    "SSR/__init__.py": "", "SSR/models/__init__.py": "", "SSR/training/__init__.py": "",
    "SSR/models/model_utils.py": "def run_network(*a, **k): raise NotImplementedError\ndef raw2outputs(*a, **k): raise NotImplementedError\n",
    "SSR/models/rays.py": "def sample_pdf(*a, **k): raise NotImplementedError\ndef create_rays(*a, **k): raise NotImplementedError\n",
    "SSR/models/semantic_nerf.py": "def Semantic_NeRF(*a, **k): raise NotImplementedError\ndef get_embedder(*a, **k): raise NotImplementedError\n",
    "SSR/training/training_utils.py": "def calculate_segmentation_metrics(*a, **k): raise NotImplementedError('stand-in')\n"
                                      "def calculate_depth_metrics(*a, **k): raise NotImplementedError('stand-in')\n"
                                      "def batchify_rays(*a, **k): raise NotImplementedError('stand-in')\n",
    "SSR/training/trainer.py": """
        import SSR.models.model_utils
        import SSR.models.rays
        import SSR.models.semantic_nerf
        from SSR.training.training_utils import batchify_rays, calculate_segmentation_metrics, calculate_depth_metrics


        class SSRTrainer:
            def render_rays(self, *a): raise NotImplementedError
            def volumetric_rendering(self, *a): raise NotImplementedError
            def create_ssr(self, *a): raise NotImplementedError
            def step(self, *a): raise NotImplementedError
        """,
    "train_SSR_main.py": "import SSR.training.trainer\n\n\ndef train():\n    raise NotImplementedError\n\n\nif __name__ == '__main__':\n    train()\n",
    "object_level/run_nerf.py": "def train():\n    raise NotImplementedError\n\n\n"
                                + "".join(f"def {n}(*a, **k): raise NotImplementedError\n" for n in
                                          ("run_network", "batchify_rays", "render", "render_rays", "raw2outputs", "NeRF", "get_embedder",
                                           "Embedder", "sample_pdf", "get_rays", "get_rays_np", "ndc_rays", "create_nerf"))
                                + "\nif __name__ == '__main__':\n    train()\n",
}

CHECK = r'''
import sys
sys.dont_write_bytecode = True
sys.path.insert(0, %(repo)r)
from intrinsicnerf_amd import evaluation, launch
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py", evaluate=%(flag)s)
trainer, utils = sys.modules["SSR.training.trainer"], sys.modules["SSR.training.training_utils"]
for m in (trainer, utils):
    for name in ("calculate_segmentation_metrics", "calculate_depth_metrics"):
        ours = getattr(m, name) is getattr(evaluation, name)
        assert ours == %(flag)s, (m.__name__, name)
assert trainer.batchify_rays is utils.batchify_rays and trainer.batchify_rays.__code__.co_filename.endswith("training_utils.py")
bound = mod.__inerf_bound__
assert ("calculate_depth_metrics" in bound.get("SSR.training.training_utils", [])) == %(flag)s
assert ("calculate_depth_metrics" in bound.get("SSR.training.trainer", [])) == %(flag)s
print("eval rebinding ok")
'''

OBJECT_CHECK = r'''
import sys
sys.dont_write_bytecode = True
sys.path.insert(0, %(repo)r)
from intrinsicnerf_amd import launch
launch.prepare(%(ref)r + "/object_level/run_nerf.py", evaluate=True)
launch.prepare(%(ref)r + "/object_level/run_nerf.py", evaluate=True)
print("object ok")
'''


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    base = tmp_path_factory.mktemp("eval_stand_in")
    for rel, text in STAND_IN.items():
        path = base / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(textwrap.dedent(text).lstrip("\n"))
    return str(base)


@pytest.mark.parametrize("flag", [True, False])
def test_inerf_eval_rebinds_both_names_in_both_modules(ref, flag):
    proc = subprocess.run([sys.executable, "-c", CHECK % {"repo": REPO, "ref": ref, "flag": flag}], capture_output=True, text=True)
    assert proc.returncode == 0 and "eval rebinding ok" in proc.stdout, proc.stdout + proc.stderr


def test_inerf_eval_tells_the_object_level_script_once(ref):
    proc = subprocess.run([sys.executable, "-c", OBJECT_CHECK % {"repo": REPO, "ref": ref}], capture_output=True, text=True)
    assert proc.returncode == 0 and "object ok" in proc.stdout, proc.stdout + proc.stderr
    assert proc.stderr.count("--inerf-eval has no effect on run_nerf.py") == 1
