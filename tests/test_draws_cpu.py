"""CPU: the training draws (csrc/draws.h; include/inerf.h, "Training draws") without a device - the NumPy restatement
(tests/_draws.py) against Philox4x32-10's known answers and its statistics, the ABI of the drawn entry points (version, struct
layout, argument validation: nothing here reaches a launch), and the launcher's ``--inerf-draws`` hooks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _draws
from conftest import REPO
from test_launch_cpu import PRELUDE, _run, ref  # noqa: F401  (the stand-in scripts of the launcher tests)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi


# ---- the generator ----------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    got = _draws.philox4x32_10(counter, key)
    assert " ".join("%08x" % int(w) for w in got) == want


def test_layout_of_one_call():
    """counter = {ray_base + ray, block | stream << 16, step lo, step hi}, key = {seed lo, seed hi}; word i of block b is sample 4b + i."""
    seed, step, base = 0xA4093822299F31D0, (7 << 32) | 9, (1 << 32) - 3
    w = _draws.words(seed, step, _draws.U, 5, 10, ray_base=base)
    for ray in (0, 2, 4):          # rays 3 and 4 wrap to 0 and 1: the ray word is 32 bits
        for s in (0, 3, 4, 9):
            one = _draws.philox4x32_10(((base + ray) & 0xFFFFFFFF, (s >> 2) | (2 << 16), 9, 7), (0x299F31D0, 0xA4093822))
            assert int(w[ray, s]) == int(one[s & 3])
    u = _draws.uniform(seed, step, _draws.JITTER, 3, 7)
    assert u.dtype == np.float32 and u.shape == (3, 7)
    assert np.array_equal(_draws.uniform_from(np.array([0xFFFFFFFF, 0, 0x100], dtype=np.uint64)),
                          np.array([1 - 2.0 ** -24, 0, 2.0 ** -24], dtype=np.float32))
    # Box-Muller's corners: u1 = 2^-23 (the largest |z|) and u1 = 1 (zero)
    z = _draws.normal_from(np.array([[0, 0, 0xFFFFFFFF, 0]], dtype=np.uint64))
    assert abs(z[0, 0] - _draws.MAX_NORMAL) < 1e-12 and z[0, 1] == 0.0 and z[0, 2] == 0.0 and _draws.MAX_NORMAL < 5.65


# ---- statistics of the restatement alone ---------------------------------------------------------------------------
# Conditions, not measurements: the seeds were picked once so that the restatement passes, and are recorded here.
STAT_SEEDS = {_draws.JITTER: 0x1D2C3B4A59687766, _draws.NOISE_COARSE: 0x2E3D4C5B6A798877, _draws.U: 0x3F4E5D6C7B8A9988,
              _draws.NOISE_FINE: 0x405F6E7D8C9BAA99}
STAT_STEP = (1 << 32) + 11
N_RAYS, N_PER_RAY = 1024, 256          # 2^18 draws per stream
_erf = np.frompyfunc(math.erf, 1, 1)


def _stream(stream, seed, step):
    if stream in (_draws.JITTER, _draws.U):
        return _draws.uniform(seed, step, stream, N_RAYS, N_PER_RAY).astype(np.float64)
    return _draws.normal(seed, step, stream, N_RAYS, N_PER_RAY)


def _ks(x, cdf):
    x = np.sort(x.ravel())
    n = x.size
    f = cdf(x)
    return max(np.max(np.arange(1, n + 1) / n - f), np.max(f - np.arange(n) / n))


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float(np.dot(a, b) / np.sqrt(np.dot(a, a) * np.dot(b, b)))


@pytest.mark.parametrize("stream", [_draws.JITTER, _draws.NOISE_COARSE, _draws.U, _draws.NOISE_FINE])
def test_statistics_of_a_stream(stream):
    n = N_RAYS * N_PER_RAY
    x = _stream(stream, STAT_SEEDS[stream], STAT_STEP)
    if stream in (_draws.JITTER, _draws.U):
        assert x.min() >= 0.0 and x.max() < 1.0
        ks, mean, var = _ks(x, lambda v: v), 0.5, 1.0 / 12.0
    else:
        assert np.abs(x).max() <= _draws.MAX_NORMAL
        ks, mean, var = _ks(x, lambda v: 0.5 * (1.0 + _erf(v / math.sqrt(2.0)).astype(np.float64))), 0.0, 1.0
    assert ks * math.sqrt(n) < 1.95, ks * math.sqrt(n)
    assert abs(x.mean() - mean) < 4 / math.sqrt(n) and abs(x.var() - var) < 8 / math.sqrt(n), (x.mean(), x.var())
    bound = 4 / math.sqrt(n)
    assert abs(_corr(x[:, :-1], x[:, 1:])) < bound                       # along the samples of a ray
    assert abs(_corr(x[:-1], x[1:])) < bound                             # along the rays
    assert abs(_corr(x, _stream(stream, STAT_SEEDS[stream], STAT_STEP + 1))) < bound       # consecutive steps


def test_the_two_noise_streams_are_uncorrelated():
    seed = STAT_SEEDS[_draws.NOISE_COARSE]
    a, b = _stream(_draws.NOISE_COARSE, seed, STAT_STEP), _stream(_draws.NOISE_FINE, seed, STAT_STEP)
    bound = 4 / math.sqrt(a.size)
    assert abs(_corr(a, b)) < bound and abs(_corr(a[:, :-1], b[:, 1:])) < bound
    u, v = _stream(_draws.JITTER, seed, STAT_STEP), _stream(_draws.U, seed, STAT_STEP)
    assert abs(_corr(u, v)) < bound


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_abi_version_and_struct_layout(capi):
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    header = int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1))
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version() and header > 40013
    body = text[text.index("typedef struct inerf_draw_args"):text.index("} inerf_draw_args;")]
    assert re.findall(r"([a-z_]+)\s*;", body) == [f[0] for f in capi.DrawArgs._fields_]
    assert C.sizeof(capi.DrawArgs) == 40 and capi.DrawArgs.noise_std.offset == 32 and capi.DrawArgs.flags.offset == 36
    for name, value in (("STREAM_JITTER", 0), ("STREAM_NOISE_COARSE", 1), ("STREAM_U", 2), ("STREAM_NOISE_FINE", 3), ("PERTURB", 1), ("FINE", 2)):
        assert int(re.search(rf"#define INERF_DRAW_{name}\s+(\d+)", text).group(1)) == value == getattr(capi, "DRAW_" + name)
    quoted = re.findall(r'#include "([^"]+)"', open(os.path.join(REPO, "intrinsicnerf_amd", "csrc", "ray_ops.hip")).read())
    from intrinsicnerf_amd import _build
    assert "draws.h" in quoted and os.path.join(_build.CSRC, "draws.h") in _build.HEADERS


FAKE = 0x10000          # a non-NULL "device pointer": every check below returns before anything could read it


def _entry_points(capi):
    """name -> call(draw pointer, n_rays, classic random pointer): every other pointer NULL, shapes inside the stage limits."""
    lib = capi.lib()
    co = capi.CompositeOut()

    def render(field):
        def call(d, n, p):
            a = capi.RenderArgs()
            a.net = capi.net_desc(capi.VARIANT_OBJECT)
            a.n_rays, a.n_samples, a.n_importance = n, 64, 128
            setattr(a, field, p)
            return lib.inerf_render_rays_drawn(C.byref(a), d, None)
        return call

    return {
        "sample_coarse": lambda d, n, p: lib.inerf_sample_coarse_drawn(None, None, p, n, 64, 0, None, d, None),
        "composite": lambda d, n, p: lib.inerf_composite_drawn(None, None, None, 3, p, n, 64, 11, 0, 0, 0, C.byref(co), d, None),
        "composite_backward": lambda d, n, p: lib.inerf_composite_backward_drawn(None, None, None, 3, p, n, 64, 11, 0, 0, 0, C.byref(co), None, d, None),
        "sample_fine": lambda d, n, p: lib.inerf_sample_fine_drawn(None, None, p, n, 64, 128, 0, None, None, None, d, None),
        "sample_pdf": lambda d, n, p: lib.inerf_sample_pdf_drawn(None, None, p, n, 63, 128, 0, None, d, None),
        "render_rays/t_rand": render("t_rand"),
        "render_rays/noise_coarse": render("noise_coarse"),
        "render_rays/noise_fine": render("noise_fine"),
        "render_rays/u": render("u"),
    }


def test_drawn_entry_points_validate_before_they_launch(capi):
    lib = capi.lib()
    D = capi.DrawArgs
    good = lambda **kw: D(**dict(dict(seed=(1 << 40) + 3, step=5, step_dev=None, ray_base=0, noise_std=1.0, flags=0), **kw))
    top = (1 << 32) - 8
    for name, call in _entry_points(capi).items():
        perturb = capi.DRAW_PERTURB if name == "render_rays/u" else 0      # (without PERTURB the whole path takes the caller's u)
        ok = C.byref(good(flags=perturb))
        assert call(ok, 0, None) == capi.OK, name                            # an empty batch
        assert call(None, 0, None) == capi.E_INVALID, name                   # no draw arguments
        assert call(ok, 0, FAKE) == capi.E_INVALID, name                     # the classic random tensor must be NULL
        assert call(C.byref(good(flags=perturb, step_dev=FAKE + 4)), 0, None) == capi.E_INVALID, name      # misaligned step_dev
        assert call(C.byref(good(flags=perturb, step_dev=FAKE + 8)), 0, None) == capi.OK, name
        assert call(C.byref(good(flags=perturb, noise_std=-1.0)), 0, None) == capi.E_INVALID, name
        assert call(C.byref(good(flags=perturb, noise_std=float("nan"))), 0, None) == capi.E_INVALID, name
        assert call(C.byref(good(flags=perturb | 64)), 0, None) == capi.E_INVALID, name                   # unknown flag
        # a flag that means nothing to the entry point: PERTURB is the whole path's, FINE the composite calls'
        assert call(C.byref(good(flags=perturb | capi.DRAW_FINE)), 0, None) == (capi.OK if name.startswith("composite") else capi.E_INVALID), name
        assert call(C.byref(good(flags=capi.DRAW_PERTURB)), 0, None) == (capi.OK if name.startswith("render_rays") else capi.E_INVALID), name
        # the counter's ray word is 32 bits: ray_base + n_rays may reach 2^32, not pass it - checked before the (NULL) data pointers
        assert call(C.byref(good(flags=perturb, ray_base=top)), 9, None) == capi.E_UNSUPPORTED, name
        assert call(C.byref(good(flags=perturb, ray_base=top)), 8, None) == capi.E_INVALID, name           # passes; then the NULL pointers
        assert call(C.byref(good(flags=perturb, ray_base=1 << 32)), 0, None) == capi.OK, name
        assert call(C.byref(good(flags=perturb, ray_base=(1 << 32) + 1)), 0, None) == capi.E_UNSUPPORTED, name
    # without PERTURB inerf_render_rays_drawn takes the caller's shared u, as the classic form does
    assert _entry_points(capi)["render_rays/u"](C.byref(good()), 0, FAKE) == capi.OK
    # the stage limits still come first, for an empty batch too
    assert lib.inerf_composite_drawn(None, None, None, 3, None, 0, 1025, 11, 0, 0, 0, C.byref(capi.CompositeOut()), C.byref(good()), None) == capi.E_UNSUPPORTED
    assert lib.inerf_sample_coarse_drawn(None, None, None, 0, 1025, 0, None, C.byref(good()), None) == capi.E_UNSUPPORTED
    assert lib.inerf_sample_fine_drawn(None, None, None, 0, 2, 128, 0, None, None, None, C.byref(good()), None) == capi.E_UNSUPPORTED
    # inerf_draw_fill / inerf_draw_advance
    g = C.byref(good())
    assert lib.inerf_draw_fill(g, 0, 0, 64, None, None) == capi.OK and lib.inerf_draw_fill(None, 0, 0, 64, None, None) == capi.E_INVALID
    assert lib.inerf_draw_fill(g, 4, 0, 64, None, None) == capi.E_INVALID and lib.inerf_draw_fill(g, -1, 0, 64, None, None) == capi.E_INVALID
    assert lib.inerf_draw_fill(g, 0, 0, 1025, None, None) == capi.E_UNSUPPORTED and lib.inerf_draw_fill(g, 0, 0, 0, None, None) == capi.E_INVALID
    assert lib.inerf_draw_fill(g, 0, 4, 64, None, None) == capi.E_INVALID                                   # no output buffer
    assert lib.inerf_draw_fill(C.byref(good(flags=capi.DRAW_FINE)), 0, 0, 64, None, None) == capi.E_INVALID   # the stream is an argument here
    assert lib.inerf_draw_fill(C.byref(good(ray_base=top)), 0, 9, 64, None, None) == capi.E_UNSUPPORTED
    assert lib.inerf_draw_fill(C.byref(good(step_dev=FAKE + 4)), 0, 0, 64, None, None) == capi.E_INVALID
    assert lib.inerf_draw_advance(None, None) == capi.E_INVALID and lib.inerf_draw_advance(FAKE + 4, None) == capi.E_INVALID


def test_front_ends_refuse_what_the_draws_cannot_do():
    import torch
    from intrinsicnerf_amd import draws, kernels
    with pytest.raises(RuntimeError, match="no CPU / eager fallback exists"):
        draws.DrawState(1, "cpu")
    with pytest.raises(RuntimeError, match="no CPU / eager fallback exists"):
        kernels.draw_fill(None, 0, 4, 4, torch.device("cpu"))


# ---- the launcher -------------------------------------------------------------------------------------------------------
OBJECT_DRAWS = PRELUDE + r'''
import tempfile
from intrinsicnerf_amd import draws
made = []
draws.DrawState = lambda seed, device, step=0: made.append((seed, str(device))) or ("DrawState", seed)
def names(**flags):
    mod, main = launch.prepare(%(ref)r + "/object_level/run_nerf.py", **flags)
    return mod, set(mod.__dict__["__inerf_bound__"])
plain, bound_plain = names()
assert plain.create_nerf.__code__.co_filename.endswith("object_level/run_nerf.py")          # without the flag: the script's own
mod, bound = names(draws=True)
assert bound - bound_plain == {"create_nerf"} and bound_plain <= bound
assert mod.create_nerf.__wrapped__.__code__.co_filename.endswith("object_level/run_nerf.py")
for name in ("train", "render_path", "config_parser", "batchify"):
    assert getattr(mod, name).__code__.co_filename.endswith("object_level/run_nerf.py"), name
with tempfile.TemporaryDirectory() as base:
    os.makedirs(os.path.join(base, "exp"))
    args = types.SimpleNamespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=128, netdepth=8, netwidth=256,
                                 netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4, basedir=base, expname="exp", ft_path=None,
                                 no_reload=True, perturb=1.0, N_samples=64, white_bkgd=True, raw_noise_std=0.0, dataset_type="blender",
                                 no_ndc=False, lindisp=False)
    torch.manual_seed(1234)                                               # the script's own seeding comes first
    train_kw, test_kw = mod.create_nerf(args)[:2]
    assert train_kw["draws"] == ("DrawState", 1234) and made == [(1234, "cpu")] and "draws" not in test_kw
    assert "draws" not in plain.create_nerf(args)[0]
print("object-level draws hook ok")
'''

SSR_DRAWS = PRELUDE + r'''
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
from intrinsicnerf_amd import draws
made = []
draws.DrawState = lambda seed, device, step=0: made.append((seed, str(device))) or ["DrawState", seed]
trainer_mod = lambda: sys.modules["SSR.training.trainer"]
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py")
before = dict(mod.__dict__["__inerf_bound__"])
assert vars(trainer_mod().SSRTrainer)["draws"] is None                    # without the flag: the mixin's default, no hook
t = trainer_mod().SSRTrainer.__new__(trainer_mod().SSRTrainer)
assert t.draws is None
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py", draws=True)
after = mod.__dict__["__inerf_bound__"]
assert set(after) == set(before)
for k in after:
    extra = [n for n in after[k] if n not in before[k]]
    assert extra == (["draws"] if k == "SSR.training.trainer.SSRTrainer" else []), (k, extra)
T = trainer_mod().SSRTrainer
assert isinstance(vars(T)["draws"], launch._TrainerDraws)
t = T.__new__(T)
t.ssr_net_coarse = torch.nn.Linear(2, 2)
torch.manual_seed(4321)
try:
    T.__new__(T).draws                                                    # a trainer without networks yet: loud, not torch's generator
except AttributeError:
    pass
else:
    raise AssertionError("expected AttributeError")
first = t.draws
assert first == ["DrawState", 4321] and t.draws is first and made == [(4321, "cpu")]        # one state per trainer, made on first use
print("ssr draws hook ok")
'''


def test_launcher_draws_flag_wraps_create_nerf_and_nothing_else(ref):  # noqa: F811
    assert "object-level draws hook ok" in _run(OBJECT_DRAWS, ref)


def test_launcher_draws_flag_sets_the_ssr_trainers_draws_and_nothing_else(ref):  # noqa: F811
    assert "ssr draws hook ok" in _run(SSR_DRAWS, ref)


def test_launcher_main_strips_the_flag(monkeypatch):
    from intrinsicnerf_amd import _capi, launch
    seen = {}

    def fake_prepare(script, *a, **kw):
        seen.update(script=script, a=a, kw=kw)
        import types
        return types.ModuleType("m"), compile("", "x", "exec")

    monkeypatch.setattr(launch, "prepare", fake_prepare)
    monkeypatch.setattr(_capi, "lib", lambda: None)
    import sys
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    launch.main(["--inerf-draws", "object_level/run_nerf.py", "--config", "c.txt"])
    assert seen["kw"] == {"draws": True} and sys.argv == ["object_level/run_nerf.py", "--config", "c.txt"]
    launch.main(["object_level/run_nerf.py"])
    assert seen["kw"] == {}
