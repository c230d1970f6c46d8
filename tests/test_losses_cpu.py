"""The training losses (intrinsicnerf_amd/losses.py, csrc/losses.hip) as far as they go without a GPU: the public names, the C
ABI's argument checks, the fixtures of tests/golden/loss_*.npz against the float64 restatement of tests/_losses.py (and that
restatement against the live reference where it is mounted), and the launcher's opt-in ``--inerf-losses`` rebinding."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import _losses
from test_launch_cpu import PRELUDE, STAND_IN, _placeholders, _run

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_module_and_exports():
    from intrinsicnerf_amd import _capi, losses, object_level as ol, ssr
    assert ol.compute_intrinsic_loss is losses.compute_intrinsic_loss and ol.object_step_loss is losses.object_step_loss
    assert ssr.compute_intrinsic_loss is losses.compute_intrinsic_loss_ssr and ssr.ssr_step_loss is losses.ssr_step_loss
    assert losses.TERMS == _losses.TERMS == _capi.LOSS_TERM_NAMES
    for name in ("inerf_intrinsic_loss", "inerf_intrinsic_loss_backward", "inerf_intrinsic_loss_workspace_bytes"):
        assert name in _capi.SYMBOLS and getattr(_capi.lib(), name) is not None
    import inspect
    assert list(inspect.signature(ol.compute_intrinsic_loss).parameters) == ["albedo", "shading", "residual", "gt_rgb", "disp", "acc", "obj_mask"]
    assert list(inspect.signature(ssr.compute_intrinsic_loss).parameters)[-1] == "semantic_label"


def test_header_constants_match_binding():
    import re
    from intrinsicnerf_amd import _capi
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    value = lambda name: int(re.search(rf"#define {name}\s+(\d+)", text).group(1))
    assert value("INERF_LOSS_TERMS") == _capi.LOSS_TERMS == len(_capi.LOSS_TERM_NAMES)
    assert value("INERF_LOSS_STATE_FLOATS") == _capi.LOSS_STATE_FLOATS and value("INERF_LOSS_MAX_CLASSES") == _capi.LOSS_MAX_CLASSES
    for i, name in enumerate(_capi.LOSS_TERM_NAMES):
        assert value("INERF_LOSS_TERM_" + name.upper()) == i
    for struct, mirror in (("inerf_loss_level", _capi.LossLevel), ("inerf_loss_args", _capi.LossArgs)):
        body = text[text.index(f"typedef struct {struct} {{"):text.index(f"}} {struct};")]
        names = re.findall(r"([a-z_]+)(?:\[\d+\])?\s*;", body)
        assert names == [f[0] for f in mirror._fields_], struct


def test_argument_validation_needs_no_device():
    """Every bad call is turned away before a launch: the pointers below are never dereferenced."""
    from intrinsicnerf_amd import _capi
    lib = _capi.lib()
    fake = 0x1000

    def args(**over):
        a = _capi.LossArgs()
        a.n_rays, a.n_levels, a.gt_rgb, a.pair_key, a.state, a.state_bytes = 64, 1, fake, fake, fake, 2 * 16 * 4
        for l in range(2):
            a.level[l].albedo = a.level[l].shading = a.level[l].residual = fake
            a.level[l].d_albedo = a.level[l].d_shading = a.level[l].d_residual = fake
        for k, v in over.items():
            if "." in k:
                lv, field = k.split(".")
                setattr(a.level[int(lv)], field, v)
            else:
                setattr(a, k, v)
        return a

    assert lib.inerf_intrinsic_loss_workspace_bytes(2048, 1) == 2 * 16 * 4 and lib.inerf_intrinsic_loss_workspace_bytes(0, 2) == 3 * 16 * 4
    assert lib.inerf_intrinsic_loss_workspace_bytes(-1, 1) == _capi.E_INVALID and lib.inerf_intrinsic_loss_workspace_bytes(8, 3) == _capi.E_INVALID
    for fn in (lib.inerf_intrinsic_loss, lib.inerf_intrinsic_loss_backward):
        bad = lambda want, **over: fn(C.byref(args(**over)), None) == want or pytest.fail(f"{fn.__name__} {over}: expected {want}")
        assert fn(None, None) == _capi.E_INVALID
        bad(_capi.E_INVALID, n_rays=-1)
        bad(_capi.E_INVALID, n_levels=0)
        bad(_capi.E_INVALID, n_levels=3)
        bad(_capi.E_INVALID, flags=4)
        bad(_capi.E_INVALID, flags=_capi.LOSS_KEY_LABELS | _capi.LOSS_MASK_OUTER)
        bad(_capi.E_INVALID, gt_rgb=None)
        bad(_capi.E_INVALID, pair_key=None)
        bad(_capi.E_INVALID, **{"0.albedo": None})
        bad(_capi.E_INVALID, n_levels=2, state_bytes=3 * 16 * 4, **{"1.shading": None})
        bad(_capi.E_INVALID, n_levels=2, state_bytes=3 * 16 * 4, **{"0.rgb": fake})                  # the image term on one level only
        bad(_capi.E_INVALID, n_classes=5, **{"0.logits": fake, "0.d_logits": fake})                    # logits without labels
        bad(_capi.E_INVALID, n_classes=0, ce_labels=fake, **{"0.logits": fake, "0.d_logits": fake})
        bad(_capi.E_UNSUPPORTED, n_classes=102, ce_labels=fake, **{"0.logits": fake, "0.d_logits": fake})
        bad(_capi.E_UNSUPPORTED, n_rays=(1 << 30) + 1)
        bad(_capi.E_WORKSPACE, state=None)
        bad(_capi.E_WORKSPACE, state_bytes=2 * 16 * 4 - 1)
        bad(_capi.E_WORKSPACE, n_levels=2)
    back = lib.inerf_intrinsic_loss_backward
    assert back(C.byref(args(**{"0.d_albedo": None})), None) == _capi.E_INVALID
    assert back(C.byref(args(**{"0.rgb": fake})), None) == _capi.E_INVALID                             # rgb given, d_rgb missing
    assert back(C.byref(args(n_classes=5, ce_labels=fake, **{"0.logits": fake})), None) == _capi.E_INVALID
    assert back(C.byref(args(n_rays=0)), None) == _capi.OK                                             # nothing to write, nothing launched


def test_cpu_tensors_raise():
    from intrinsicnerf_amd import losses
    n = 8
    a, s, r, g = torch.rand(n, 3), torch.rand(n), torch.rand(n, 3), torch.rand(n, 3)
    with pytest.raises(RuntimeError, match="no CPU"):
        losses.compute_intrinsic_loss(a, s, r, g, None, None, torch.ones(n))
    with pytest.raises(RuntimeError, match="no CPU"):
        losses.object_step_loss({"rgb_map": g, "albedo_map": a, "shading_map": s, "residual_map": r}, g, torch.ones(n), {})
    with pytest.raises(RuntimeError, match="no CPU"):
        losses.ssr_step_loss({"rgb_coarse": g, "albedo_coarse": a, "shading_coarse": s, "residual_coarse": r, "sem_logits_coarse": torch.rand(n, 4)},
                             g, torch.ones(n, dtype=torch.int64), {})


@pytest.mark.parametrize("kind", ["object", "ssr"])
def test_fixture_sets_hold_the_cases_the_kernels_must_reproduce(kind):
    cs = _losses.cases(kind)
    shapes = {name: (c["gt"].shape[0], c["key"].shape, int(c["levels"]), "target" in c) for name, c in cs.items()}
    ns = {v[0] for v in shapes.values()}
    if kind == "object":
        assert {2048, 2047, 3, 2} <= ns
        assert any(v[0] == 2048 and len(v[1]) == 1 for v in shapes.values()) and any(v[0] == 2048 and len(v[1]) == 2 for v in shapes.values())
        assert any(not c["key"].any() for c in cs.values())                                      # a mask that is all zero
    else:
        classes = {c["logits0"].shape[1] for c in cs.values() if c["gt"].shape[0] == 1024}
        assert classes >= {1, 28, 101}
        assert any(not c["key"].any() for c in cs.values())                                      # every label void
        mixed = cs["n1024_c28_target"]["key"]
        h = mixed.shape[0] // 2
        assert (mixed == 0).any() and (mixed[:h] == mixed[h:]).any() and (mixed[:h] != mixed[h:]).any()
    assert any(v[3] for v in shapes.values()) and any(not v[3] for v in shapes.values())          # with and without the cluster target
    assert any(v[2] == 2 for v in shapes.values())
    for name, c in cs.items():
        # the condition under which the tests may use the plain 1e-4 bound: the reference's own fp32-vs-fp64 distance is 10x smaller
        devs = [np.nanmax(v) for k, v in c.items() if k.startswith("dev_")]
        assert max(devs) < 1e-5, (name, max(devs))
        if c["gt"].shape[0] >= 4:
            g = c["gt"]
            assert abs(g.mean() - c["albedo0"].mean()) > 0.05, name                              # the intensity term is well conditioned
            cr = g[:, :2] / (g.sum(-1, keepdims=True) + 1e-5)
            h = g.shape[0] // 2
            assert np.exp(-60 * ((cr[:h] - cr[-h:]) ** 2).sum(-1)).mean() > 0.05 or g.shape[0] % 2, name   # w_chroma is not ~0 everywhere


@pytest.mark.parametrize("kind,name", [(k, n) for k in ("object", "ssr") for n in _losses.case_names(k)])
def test_float64_restatement_reproduces_fixture(kind, name):
    c = _losses.cases(kind)[name]
    terms, total, grads = _losses.restate(c)
    for l, t in enumerate(terms):
        _losses.assert_terms(t.detach().numpy(), c[f"terms64_{l}"], f"{name} level {l} against the reference in fp64")
        np.testing.assert_allclose(t.detach().numpy(), c[f"terms64_{l}"], rtol=1e-10, atol=1e-14, equal_nan=True)
        _losses.assert_terms(t.detach().numpy(), c[f"terms{l}"], f"{name} level {l}")
    _losses.assert_terms([float(total)], [float(c["total"])], f"{name} total")
    assert set(grads) == {k for k in c if k.startswith("g_")}
    for k, g in grads.items():
        _losses.assert_gradient(g, c[k], f"{name} {k}")


def test_fixtures_exist():
    assert len(_losses.case_names("object")) >= 7 and len(_losses.case_names("ssr")) >= 5


def test_restatement_equals_the_live_reference_on_random_shapes():
    """Where the reference is mounted (the build container): both mask shapes, odd and tiny N, labels with void rays, with
    gradients - tests/golden/check_losses_live.py in a subprocess (the import recipe patches torch)."""
    if not os.path.isdir("/root/reference/object_level"):
        pytest.skip("reference not mounted")
    script = os.path.join(REPO, "tests", "golden", "check_losses_live.py")
    out = subprocess.run([sys.executable, script], capture_output=True, text=True, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "restatement == reference on 24 random cases" in out.stdout


# ---- the launcher's --inerf-losses: same stand-in entry scripts as test_launch_cpu.py, plus the modules that hold the loss ----
LOSS_STAND_IN = dict(STAND_IN)
LOSS_STAND_IN["object_level/run_nerf_helpers.py"] = _placeholders("compute_intrinsic_loss", "img2mse")
LOSS_STAND_IN["object_level/run_nerf.py"] = "from run_nerf_helpers import *\n" + STAND_IN["object_level/run_nerf.py"]
LOSS_STAND_IN["SSR/training/training_utils.py"] = _placeholders("compute_intrinsic_loss", "img2mse")
LOSS_STAND_IN["SSR/training/trainer.py"] = "from SSR.training.training_utils import compute_intrinsic_loss\n" + STAND_IN["SSR/training/trainer.py"]


@pytest.fixture(scope="module")
def loss_ref(tmp_path_factory):
    root = os.environ.get("INERF_REFERENCE_ROOT")
    if root:
        return root
    base = tmp_path_factory.mktemp("launcher_loss_stand_in")
    for rel, text in LOSS_STAND_IN.items():
        path = base / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(textwrap.dedent(text).lstrip("\n"))
    return str(base)


WITH_FLAG = PRELUDE + r'''
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
from intrinsicnerf_amd import losses
mod, main = launch.prepare(%(ref)r + "/object_level/run_nerf.py", losses=True)
assert mod.compute_intrinsic_loss is losses.compute_intrinsic_loss is ol.compute_intrinsic_loss
assert "compute_intrinsic_loss" in mod.__inerf_bound__
assert mod.train.__code__.co_filename.endswith("object_level/run_nerf.py")                 # the training loop that calls it stays the script's
assert sys.modules["run_nerf_helpers"].compute_intrinsic_loss.__code__.co_filename.endswith("run_nerf_helpers.py")   # the helper module is left alone
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py", losses=True)
trainer = sys.modules["SSR.training.trainer"]
assert trainer.compute_intrinsic_loss is losses.compute_intrinsic_loss_ssr is ssr.compute_intrinsic_loss
assert "compute_intrinsic_loss" in mod.__inerf_bound__["SSR.training.trainer"]
assert sys.modules["SSR.training.training_utils"].compute_intrinsic_loss.__code__.co_filename.endswith("training_utils.py")
print("loss flag ok")
'''

WITHOUT_FLAG = PRELUDE + r'''
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
mod, main = launch.prepare(%(ref)r + "/object_level/run_nerf.py", with_render_path=True, cluster_fit=True)
assert mod.compute_intrinsic_loss.__code__.co_filename.endswith("run_nerf_helpers.py")
assert "compute_intrinsic_loss" not in mod.__inerf_bound__
assert set(mod.__inerf_bound__) == set(launch.OBJECT_SYMBOLS + launch.OBJECT_OPTIONAL)
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py", with_render_path=True, cluster_fit=True)
trainer = sys.modules["SSR.training.trainer"]
assert trainer.compute_intrinsic_loss.__code__.co_filename.endswith("training_utils.py")
assert all("compute_intrinsic_loss" not in v for v in mod.__inerf_bound__.values())
print("default loss bindings ok")
'''


def test_loss_flag_rebinds_both_scripts(loss_ref):
    assert "loss flag ok" in _run(WITH_FLAG, loss_ref)


def test_without_the_flag_the_reference_loss_stays(loss_ref):
    assert "default loss bindings ok" in _run(WITHOUT_FLAG, loss_ref)


def test_loss_flag_is_parsed_and_removed(monkeypatch):
    from intrinsicnerf_amd import _capi, launch
    seen = []
    fake = lambda *a: seen.append(a) or (type("M", (), {"__dict__": {}})(), compile("", "x", "exec"))
    monkeypatch.setattr(launch, "prepare", fake)
    monkeypatch.setattr(_capi, "lib", lambda: None)
    monkeypatch.setattr(sys, "argv", sys.argv[:])
    for argv in (["run_nerf.py", "--inerf-losses", "--config", "x"], ["run_nerf.py", "--config", "x"]):
        try:
            launch.main(argv)
        except Exception:
            pass
    assert seen[0] == ("run_nerf.py", False, False, True) and seen[1] == ("run_nerf.py", False, False)
    assert sys.argv == ["run_nerf.py", "--config", "x"]
