"""The Adam step (intrinsicnerf_amd/optim.py, csrc/adam.hip, ``inerf_adam_step``) as far as it goes without a GPU: the header,
the exported symbol and its binding, the C ABI's argument checks (all of them run before a launch), the optimizer's state layout
against ``torch.optim.Adam`` in both directions, the options it refuses, and the launcher's opt-in ``--inerf-adam`` on entry
scripts with the reference's file names (the stand-in of tests/test_launch_cpu.py, whose ``create_nerf`` here builds an
optimizer; INERF_REFERENCE_ROOT=<an IntrinsicNeRF checkout> points the same checks at the real scripts)."""
import ctypes as C
import os
import re
import textwrap

import pytest
import torch

from test_launch_cpu import PRELUDE, STAND_IN, _run

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. header, library, binding ----
def test_header_library_and_binding_agree():
    from intrinsicnerf_amd import _capi
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    assert re.search(r"int\s+inerf_adam_step\s*\(\s*const\s+inerf_adam_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)\s*;", text)
    body = text[text.index("typedef struct inerf_adam_args {"):text.index("} inerf_adam_args;")]
    names = re.findall(r"([a-z_0-9]+)\s*;", body)
    assert names == [f[0] for f in _capi.AdamArgs._fields_]
    assert names == ["n_tensors", "params", "grads", "exp_avg", "exp_avg_sq", "steps", "counts", "lr", "lr_dev", "beta1", "beta2", "eps"]
    for line in ("run_nerf.py:304,1019", "trainer.py:842,991"):                         # the lines it replaces, as every entry point cites
        assert line in text
    header_abi = int(re.search(r"#define INERF_ABI_VERSION\s+(\d+)", text).group(1))
    lib = _capi.lib()
    assert "inerf_adam_step" in _capi.SYMBOLS and lib.inerf_adam_step is not None
    assert lib.inerf_abi_version() == header_abi == _capi.ABI_VERSION and header_abi >= 40011
    assert C.sizeof(_capi.AdamArgs) == 96                                               # the C layout: 4 + pad, 6 pointers, float + pad, pointer, 3 doubles


# ---- 2. argument checks: the pointers below are never dereferenced, nothing is launched ----
def _args(n=2, **over):
    from intrinsicnerf_amd import _capi
    fake = 0x1000
    a = _capi.AdamArgs()
    keep = []
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "steps"):
        arr = (C.c_void_p * max(n, 1))(*[fake + 64 * i for i in range(max(n, 1))])
        keep.append(arr)
        setattr(a, name, C.cast(arr, C.c_void_p))
    counts = (C.c_int64 * max(n, 1))(*[7] * max(n, 1))
    keep.append(counts)
    a.counts = C.cast(counts, C.c_void_p)
    a.n_tensors, a.lr, a.beta1, a.beta2, a.eps = n, 5e-4, 0.9, 0.999, 1e-8
    for k, v in over.items():
        if k == "count0":
            counts[0] = v
        elif k == "param1":
            keep[0][1] = v
        else:
            setattr(a, k, v)
    a._keep = keep
    return a


@pytest.mark.parametrize("over", [dict(params=None), dict(grads=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(steps=None),
                                  dict(counts=None), dict(count0=0), dict(count0=-3), dict(param1=None), dict(param1=0x1002),
                                  dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(eps=0.0),
                                  dict(eps=-1e-8), dict(n_tensors=-1)], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_bad_arguments_are_turned_away_before_any_launch(over):
    from intrinsicnerf_amd import _capi
    assert _capi.lib().inerf_adam_step(C.byref(_args(**over)), None) == _capi.E_INVALID


def test_null_block_and_empty_list():
    from intrinsicnerf_amd import _capi
    lib = _capi.lib()
    assert lib.inerf_adam_step(None, None) == _capi.E_INVALID
    assert lib.inerf_adam_step(C.byref(_args(n=0)), None) == _capi.OK
    empty = _capi.AdamArgs()                                                            # n_tensors = 0: the arrays may be null
    assert lib.inerf_adam_step(C.byref(empty), None) == _capi.OK


# ---- 3. the optimizer on CPU parameters: construction and state layout (no arithmetic) ----
def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=gen) * 0.06) for s in ((5, 3), (1,), (7,))]


def _stepped_torch_adam(params, steps=3, **kw):
    opt = torch.optim.Adam(params, **kw)
    gen = torch.Generator().manual_seed(1)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    return opt


def _assert_same_state_dict(a, b):
    assert list(a) == list(b) == ["state", "param_groups"]
    assert a["param_groups"] == b["param_groups"]
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert list(ga) == list(gb) and type(ga["lr"]) is float and ga["capturable"] is False
    assert list(a["state"]) == list(b["state"])
    for k in a["state"]:
        assert list(a["state"][k]) == list(b["state"][k]) == ["step", "exp_avg", "exp_avg_sq"]
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert x.dtype == y.dtype == torch.float32 and x.device == y.device and x.shape == y.shape, (k, name)
            assert torch.equal(x, y), (k, name)
        assert a["state"][k]["step"].dim() == 0 and float(a["state"][k]["step"]) == 3.0


def test_exported_and_constructs_like_torch_adam():
    import intrinsicnerf_amd
    from intrinsicnerf_amd import optim
    assert intrinsicnerf_amd.Adam is optim.Adam and intrinsicnerf_amd.optim is optim
    assert issubclass(optim.Adam, torch.optim.Optimizer) and not issubclass(optim.Adam, torch.optim.Adam)
    params = _params()
    for kw in (dict(lr=5e-4, betas=(0.9, 0.999)), dict(lr=5e-4), dict()):                # run_nerf.py:304, trainer.py:842, the defaults
        ours, theirs = optim.Adam(params=params, **kw), torch.optim.Adam(params=params, **kw)
        assert ours.state_dict() == theirs.state_dict()
        assert list(ours.param_groups[0]) == list(theirs.param_groups[0])
    assert optim.Adam(params).defaults["lr"] == 1e-3 and optim.Adam(params).defaults["eps"] == 1e-8


def test_state_dict_round_trips_with_torch_adam_in_both_directions():
    from intrinsicnerf_amd import optim
    params = _params()
    theirs = _stepped_torch_adam(params, lr=5e-4, betas=(0.9, 0.999))
    want = theirs.state_dict()
    ours = optim.Adam(_params(), lr=1e-3)
    ours.load_state_dict(want)
    _assert_same_state_dict(ours.state_dict(), want)
    # ... through a file, as run_nerf.py:1041 / :325 and trainer.py:1046 do
    import io
    buf = io.BytesIO()
    torch.save(ours.state_dict(), buf)
    buf.seek(0)
    fresh = torch.optim.Adam(_params(), lr=1e-2)
    fresh.load_state_dict(torch.load(buf))
    _assert_same_state_dict(fresh.state_dict(), want)
    assert fresh.param_groups[0]["lr"] == 5e-4
    # an eager torch Adam goes on stepping from it (its step counts are host tensors, as it keeps them)
    for p in fresh.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    fresh.step()
    assert all(float(st["step"]) == 4.0 and st["step"].device.type == "cpu" for st in fresh.state.values())


def test_unsupported_options_raise_value_error():
    from intrinsicnerf_amd import optim
    for kw, word in ((dict(weight_decay=1e-4), "weight_decay"), (dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize")):
        with pytest.raises(ValueError, match=word):
            optim.Adam(_params(), **kw)
    with pytest.raises(ValueError):
        optim.Adam(_params(), betas=(1.0, 0.999))
    with pytest.raises(ValueError):
        optim.Adam(_params(), eps=0.0)
    amsgrad = torch.optim.Adam(_params(), amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        optim.Adam(_params()).load_state_dict(amsgrad.state_dict())
    with pytest.raises(ValueError):
        optim.from_torch(amsgrad)


def test_step_on_cpu_parameters_raises_and_computes_nothing():
    from intrinsicnerf_amd import optim
    params = _params()
    before = [p.detach().clone() for p in params]
    opt = optim.Adam(params, lr=5e-4)
    opt.step()                                                                          # no gradient anywhere: nothing to do, as in torch
    for p in params:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU"):
        opt.step()
    assert all(torch.equal(p, b) for p, b in zip(params, before)) and not any(opt.state[p] for p in params)
    half = [torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))]
    half[0].grad = torch.ones_like(half[0])
    with pytest.raises((RuntimeError, ValueError)):
        optim.Adam(half).step()


def test_from_torch_carries_groups_and_state_over():
    from intrinsicnerf_amd import optim
    params = _params()
    theirs = _stepped_torch_adam(params, lr=5e-4, betas=(0.8, 0.99), eps=1e-7)
    ours = optim.from_torch(theirs)
    assert type(ours) is optim.Adam and optim.from_torch(ours) is ours
    assert [id(p) for p in ours.param_groups[0]["params"]] == [id(p) for p in params]
    _assert_same_state_dict(ours.state_dict(), theirs.state_dict())
    with pytest.raises(TypeError):
        optim.from_torch(torch.optim.SGD(params, lr=0.1))


# ---- 4. the launcher's --inerf-adam ----
ADAM_STAND_IN = dict(STAND_IN)
ADAM_STAND_IN["object_level/run_nerf.py"] = STAND_IN["object_level/run_nerf.py"].replace(
    "    return kwargs, dict(kwargs), 0, None, None\n",
    "    grad_vars = list(coarse.parameters()) + list(fine.parameters())\n"
    "    optimizer = torch.optim.Adam(params=grad_vars, lr=args.lrate, betas=(0.9, 0.999))\n"
    "    return kwargs, dict(kwargs), 0, grad_vars, optimizer\n")
assert ADAM_STAND_IN["object_level/run_nerf.py"] != STAND_IN["object_level/run_nerf.py"]


@pytest.fixture(scope="module")
def adam_ref(tmp_path_factory):
    root = os.environ.get("INERF_REFERENCE_ROOT")
    if root:
        return root
    base = tmp_path_factory.mktemp("launcher_adam_stand_in")
    for rel, text in ADAM_STAND_IN.items():
        path = base / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(textwrap.dedent(text).lstrip("\n"))
    return str(base)


ARGS = r'''
import tempfile
def make_args(base):
    os.makedirs(os.path.join(base, "exp"), exist_ok=True)
    return types.SimpleNamespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=128, netdepth=8, netwidth=256,
                                 netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4, basedir=base, expname="exp", ft_path=None,
                                 no_reload=True, perturb=1.0, N_samples=64, white_bkgd=True, raw_noise_std=0.0, dataset_type="blender",
                                 no_ndc=False, lindisp=False)
SSR_CONFIG = {"render": {"multires": 10, "multires_views": 4, "i_embed": 0, "use_viewdirs": True},
              "model": {"netdepth": 8, "netwidth": 256, "netdepth_fine": 8, "netwidth_fine": 256}}
def ssr_trainer(trainer):
    t = trainer.SSRTrainer.__new__(trainer.SSRTrainer)
    t.config, t.N_importance, t.enable_semantic, t.num_valid_semantic_class, t.lrate = SSR_CONFIG, 128, True, 28, 5e-4
    return t
'''

WITH_ADAM = PRELUDE + ARGS + r'''
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
from intrinsicnerf_amd import optim
torch_adam, torch_init = torch.optim.Adam, torch.optim.Adam.__init__
mod, main = launch.prepare(%(ref)r + "/object_level/run_nerf.py", adam=True)
assert torch.optim.Adam is torch_adam and torch.optim.Adam.__init__ is torch_init and mod.torch.optim.Adam is torch_adam     # nothing in torch.optim is patched
assert "create_nerf" in mod.__inerf_bound__ and set(mod.__inerf_bound__) == set(launch.OBJECT_SYMBOLS) | {"create_nerf"}
assert mod.create_nerf.__wrapped__.__code__.co_filename.endswith("object_level/run_nerf.py")      # around the script's own factory
for name in ("train", "render_path", "config_parser", "batchify"):
    assert getattr(mod, name).__code__.co_filename.endswith("object_level/run_nerf.py"), name
with tempfile.TemporaryDirectory() as base:
    train_kw, test_kw, start, grad_vars, optimizer = mod.create_nerf(make_args(base))
assert type(optimizer) is optim.Adam and len(optimizer.param_groups) == 1
g = optimizer.param_groups[0]
assert g["lr"] == 5e-4 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
assert len(g["params"]) == len(grad_vars) == 64 and all(a is b for a, b in zip(g["params"], grad_vars))
assert sum(p.numel() for p in grad_vars) == 2 * 662152
assert isinstance(train_kw["network_fn"], ol.NeRF)
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py", adam=True)
assert torch.optim.Adam is torch_adam and torch.optim.Adam.__init__ is torch_init
trainer = sys.modules["SSR.training.trainer"]
assert trainer.SSRTrainer.create_ssr.__wrapped__ is ssr.SSRRenderMixin.create_ssr
for name in ("render_rays", "volumetric_rendering"):
    assert getattr(trainer.SSRTrainer, name) is getattr(ssr.SSRRenderMixin, name), name
for name in ("step", "init_rays", "set_params", "prepare_data_replica"):
    assert getattr(trainer.SSRTrainer, name).__code__.co_filename.endswith("SSR/training/trainer.py"), name
t = ssr_trainer(trainer)
t.create_ssr()
assert type(t.optimizer) is optim.Adam and t.optimizer.param_groups[0]["lr"] == 5e-4
want = list(t.ssr_net_coarse.parameters()) + list(t.ssr_net_fine.parameters())
assert len(want) == 72 and all(a is b for a, b in zip(t.optimizer.param_groups[0]["params"], want))
print("adam flag ok")
'''

WITHOUT_ADAM = PRELUDE + ARGS + r'''
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
torch_adam = torch.optim.Adam
mod, main = launch.prepare(%(ref)r + "/object_level/run_nerf.py", with_render_path=True, cluster_fit=True, losses=False)
assert mod.create_nerf.__code__.co_filename.endswith("object_level/run_nerf.py") and not hasattr(mod.create_nerf, "__wrapped__")
assert "create_nerf" not in mod.__inerf_bound__
with tempfile.TemporaryDirectory() as base:
    optimizer = mod.create_nerf(make_args(base))[4]
assert type(optimizer) is torch_adam
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py")
trainer = sys.modules["SSR.training.trainer"]
assert trainer.SSRTrainer.create_ssr is ssr.SSRRenderMixin.create_ssr
t = ssr_trainer(trainer)
t.create_ssr()
assert type(t.optimizer) is torch_adam
print("default optimizer ok")
'''


def test_adam_flag_wraps_create_nerf_and_create_ssr_and_nothing_else(adam_ref):
    assert "adam flag ok" in _run(WITH_ADAM, adam_ref)


def test_without_the_flag_the_trainers_keep_torch_adam(adam_ref):
    assert "default optimizer ok" in _run(WITHOUT_ADAM, adam_ref)


def test_adam_flag_is_parsed_and_removed(monkeypatch):
    import sys
    from intrinsicnerf_amd import _capi, launch
    seen = []
    fake = lambda *a, **k: seen.append((a, k)) or (type("M", (), {"__dict__": {}})(), compile("", "x", "exec"))
    monkeypatch.setattr(launch, "prepare", fake)
    monkeypatch.setattr(_capi, "lib", lambda: None)
    monkeypatch.setattr(sys, "argv", sys.argv[:])
    for argv in (["run_nerf.py", "--inerf-adam", "--config", "x"], ["run_nerf.py", "--inerf-losses", "--inerf-adam"], ["run_nerf.py", "--config", "x"]):
        try:
            launch.main(argv)
        except Exception:
            pass
    assert seen[0] == (("run_nerf.py", False, False, False), {"adam": True})
    assert seen[1] == (("run_nerf.py", False, False, True), {"adam": True})
    assert seen[2] == (("run_nerf.py", False, False), {})                               # default bindings: the call is what it was
    assert sys.argv == ["run_nerf.py", "--config", "x"]
