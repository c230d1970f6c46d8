"""CPU: training-batch assembly (csrc/batch.hip, intrinsicnerf_amd/batches.py) without a device.

1. The index draw, on its NumPy restatement (tests/_batch_draw.py - the GPU suite holds the kernel to it bit for bit): the keyed
   Feistel permutation is a bijection of [0, M) by full enumeration, its cycle walk stays far below the compile-time bound,
   different steps permute differently, the offsets take all three values, and the pixels of many steps are uniform.
2. The argument checks of ``inerf_batch_assemble`` through the ctypes binding (every check runs before anything is launched).
3. The front-ends refuse host tensors; the launcher's ``--inerf-batches`` binds ``SSRTrainer.sample_data`` and nothing else new.
"""
import ctypes as C
import os
import re
import textwrap

import numpy as np
import pytest
import torch

import _batch_draw as bd
from conftest import REPO
from test_launch_cpu import PRELUDE, STAND_IN, _run

SEEDS, STEPS = (1, 0xDEADBEEFCAFE), (0, 7)
SIZES = (1, 2, 3, 5, 255, 256, 257, 40_000, 160_000, 640_000)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi, batches  # noqa: F401  (the feature: absent on the parent commit)
    return _capi


# ---- 1. the draw ----
@pytest.mark.parametrize("m", SIZES)
def test_permutation_is_a_bijection_and_its_walk_stays_below_the_bound(m):
    worst = 0
    for seed in SEEDS:
        for step in STEPS:
            p, walk, hit = bd.perm(np.arange(m), m, seed, step, return_walk=True)
            assert p.dtype == np.int64 and p.min() >= 0 and p.max() < m
            assert np.array_equal(np.sort(p), np.arange(m)), (m, seed, step)
            assert not hit.any()
            worst = max(worst, int(walk.max()))
    print(f"M = {m}: longest cycle walk {worst} of {bd.MAX_WALK}")
    assert worst < bd.MAX_WALK
    if m & (m - 1) == 0:
        assert worst == 1                                  # a power of two: the Feistel domain is [0, M) itself


def test_half_widths_cover_the_domain_and_keep_half_of_it_in_range():
    for m in list(range(1, 70)) + [255, 256, 257, 40_000, 65_536, 65_537, 640_000, 2 ** 31 - 1]:
        a, c = bd.split_bits(m)
        assert a == (a + c) // 2 and 0 <= c - a <= 1 and c <= 16          # unbalanced for odd widths; halves fit 16 bits
        assert (1 << (a + c)) >= m and (m == 1 or (1 << (a + c - 1)) < m)
        assert 2 * m > (1 << (a + c)) or m == 1                            # more than half of the Feistel domain is in range


def test_different_steps_and_seeds_give_different_permutations():
    m = 4096
    perms = [bd.perm(np.arange(m), m, seed, step) for seed in SEEDS for step in range(4)]
    for i in range(len(perms)):
        for j in range(i):
            same = float((perms[i] == perms[j]).mean())
            assert same < 0.01, (i, j, same)                               # two random permutations agree in ~1 / M places


def test_offsets_take_each_value_and_the_two_streams_differ():
    first, second = bd.offsets(3, 5, 3000)
    for off in (first, second):
        assert off.dtype == np.int64
        counts = np.bincount(off + 1, minlength=3)
        assert counts.sum() == 3000 and len(counts) == 3
        assert (np.abs(counts - 1000) < 6 * np.sqrt(3000 * (1 / 3) * (2 / 3))).all(), counts
    assert (first != second).mean() > 0.5
    images = [bd.image(3, s, n_images=5) for s in range(400)]
    assert set(images) == set(range(5))
    ids = np.array([4, 9, 17])
    assert {bd.image(3, s, image_ids=ids) for s in range(200)} == {4, 9, 17}
    img, pix, orow, ocol = bd.ssr_draw(3, 5, 3000, 42, n_images=2)
    assert pix.min() >= 0 and pix.max() < 42 and len(set(pix.tolist())) == 42
    f, s = bd.offsets(3, 5, 3000)
    assert np.array_equal(ocol, f) and np.array_equal(orow, s)              # SSR: bias_w is drawn first (rays.py:161-162)
    img, pix, orow, ocol = bd.object_draw(3, 5, 30, 42, n_images=2)
    assert np.array_equal(orow, f[:30]) and np.array_equal(ocol, s[:30])    # object level: bias_x (row) first (run_nerf.py:920-921)
    assert len(set(pix.tolist())) == 30


def test_drawn_pixels_are_uniform_over_many_steps():
    """4 000 steps of N = 64 distinct pixels from M = 256: every pixel is drawn Binomial(4000, 1/4) times; all 256 counts lie
    within 6 sigma (fixed seed: deterministic)."""
    m, n, steps = 256, 64, 4000
    counts = np.zeros(m, dtype=np.int64)
    for step in range(steps):
        p = bd.perm(np.arange(n), m, 11, step)
        assert len(np.unique(p)) == n
        counts += np.bincount(p, minlength=m)
    mean, sigma = steps * n / m, np.sqrt(steps * (n / m) * (1 - n / m))
    worst = float(np.abs(counts - mean).max() / sigma)
    print(f"uniformity: counts {counts.min()} .. {counts.max()} around {mean:.0f}, worst {worst:.2f} sigma")
    assert worst < 6.0


# ---- 2. the C ABI ----
def test_header_constants_and_struct_mirror(capi):
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    body = text[text.index("typedef struct inerf_batch_args"):text.index("} inerf_batch_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"([a-z_0-9]+)\s*;", body) == [f[0] for f in capi.BatchArgs._fields_]
    define = lambda name: int(re.search(rf"#define {name}\s+(\d+)", text).group(1))
    assert define("INERF_BATCH_MAX_WALK") == capi.BATCH_MAX_WALK == bd.MAX_WALK
    assert (define("INERF_BATCH_OBJECT"), define("INERF_BATCH_SSR")) == (capi.BATCH_OBJECT, capi.BATCH_SSR)
    assert (define("INERF_BATCH_DRAW"), define("INERF_BATCH_ADVANCE"), define("INERF_BATCH_OPENGL")) == \
        (capi.BATCH_DRAW, capi.BATCH_ADVANCE, capi.BATCH_OPENGL)
    assert (define("INERF_BATCH_STATUS_WALK"), define("INERF_BATCH_STATUS_INDEX")) == (capi.BATCH_STATUS_WALK, capi.BATCH_STATUS_INDEX)
    assert C.sizeof(capi.BatchArgs) == 288
    from intrinsicnerf_amd import _build
    assert "batch.hip" in _build.SOURCES


def _object_args(capi, **over):
    """A complete, valid object-level form (a) call on a 6 x 7 frame - with made-up non-null pointers: only checks that return
    before the launch are exercised with it."""
    p = 0x1000
    a = capi.BatchArgs()
    a.form, a.flags, a.n, a.n_images, a.height, a.width = capi.BATCH_OBJECT, capi.BATCH_OPENGL, 9, 3, 6, 7
    a.row0, a.col0, a.win_h, a.win_w, a.pose_stride, a.poses = 0, 0, 6, 7, 12, p
    a.fx = a.fy = 7.25
    a.images, a.image_bytes, a.image_host = p, 4, 0
    a.pixels = a.off_row = a.off_col = p
    a.out_rays = a.out_rgb = p
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_argument_checks_without_a_device(capi):
    call = lambda a: capi.lib().inerf_batch_assemble(C.byref(a), None)
    assert capi.lib().inerf_batch_assemble(None, None) == capi.E_INVALID
    assert call(_object_args(capi, n=-1)) == capi.E_INVALID
    assert call(_object_args(capi, n=0)) == capi.OK                                   # a no-op: nothing launched
    assert call(capi.BatchArgs()) == capi.OK                                          # (n == 0 before anything else is looked at)
    assert call(_object_args(capi, form=2)) == capi.E_INVALID
    assert call(_object_args(capi, flags=8)) == capi.E_INVALID
    bad = [dict(images=None), dict(out_rays=None), dict(out_rgb=None), dict(poses=None), dict(pose_stride=11), dict(pixels=None),
           dict(off_row=None), dict(off_col=None), dict(n_images=0), dict(height=0), dict(width=-1), dict(image_bytes=8), dict(image_bytes=2),
           dict(aux=0x1000), dict(aux=0x1000, out_aux=0x1000, aux_bytes=8), dict(semantic=0x1000), dict(ray_table=0x1000),
           dict(image_host=3), dict(image_host=-1),                                   # an image index outside its table
           dict(row0=-1), dict(col0=1), dict(row0=1, win_h=6), dict(win_h=0), dict(win_w=8),      # a window that leaves the image
           dict(flags=capi.BATCH_OPENGL | capi.BATCH_ADVANCE)]                        # advancing is for drawn steps
    for over in bad:
        assert call(_object_args(capi, **over)) == capi.E_INVALID, over
    # the distinct draw: at most M pixels
    drawn = dict(flags=capi.BATCH_OPENGL | capi.BATCH_DRAW, pixels=None, off_row=None, off_col=None)
    assert call(_object_args(capi, n=43, **drawn)) == capi.E_INVALID
    assert call(_object_args(capi, n=5, row0=2, col0=2, win_h=2, win_w=2, **drawn)) == capi.E_INVALID
    assert call(_object_args(capi, flags=capi.BATCH_OPENGL | capi.BATCH_DRAW | capi.BATCH_ADVANCE)) == capi.E_INVALID      # no step_dev
    assert call(_object_args(capi, **dict(drawn, step_dev=0x1004))) == capi.E_INVALID                                     # misaligned
    assert call(_object_args(capi, **dict(drawn, image_ids=0x1000, n_image_ids=0))) == capi.E_INVALID
    # sizes beyond 32-bit pixel arithmetic
    assert call(_object_args(capi, height=1 << 16, width=1 << 15, win_h=1, win_w=1)) == capi.E_UNSUPPORTED
    assert call(_object_args(capi, n=1 << 30)) == capi.E_UNSUPPORTED
    # SSR
    ssr = dict(form=capi.BATCH_SSR, flags=0)
    assert call(_object_args(capi, **dict(ssr, poses=None, ray_table=None))) == capi.E_INVALID
    assert call(_object_args(capi, **dict(ssr, image_bytes=3))) == capi.E_INVALID
    assert call(_object_args(capi, **dict(ssr, semantic=0x1000))) == capi.E_INVALID                  # no out_semantic
    assert call(_object_args(capi, **dict(ssr, semantic=0x1000, out_semantic=0x1000, semantic_bytes=3))) == capi.E_INVALID
    assert call(_object_args(capi, **dict(ssr, avail=0x1000))) == capi.E_INVALID
    assert call(_object_args(capi, **dict(ssr, aux=0x1000, out_aux=0x1000, aux_bytes=2))) == capi.E_INVALID


# ---- 3. front-ends and launcher ----
def test_front_ends_refuse_host_tensors(capi):
    from intrinsicnerf_amd import batches, kernels
    images, masks, poses = torch.zeros(3, 6, 7, 3), torch.zeros(3, 6, 7, 1), torch.eye(4)[None].repeat(3, 1, 1)
    K = np.array([[7.25, 0, 3.5], [0, 7.25, 3.0], [0, 0, 1]])
    with pytest.raises(RuntimeError, match="HIP device"):
        batches.ObjectBatcher(images, masks, poses, K, [0, 1], 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        batches.ObjectBatcher(images.numpy(), masks.numpy(), poses.numpy(), K, [0, 1], 4, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        batches.SSRBatcher(images.double(), torch.zeros(3, 6, 7).double(), torch.zeros(3, 6, 7, dtype=torch.uint8), 4, rays=torch.zeros(3, 42, 11))
    with pytest.raises(RuntimeError, match="no CPU"):
        kernels.batch_object(images, masks, poses, (7.25, 7.25, 3.5, 3.0), (0, 0, 6, 7), 4, draw=dict(seed=1, step=0))
    with pytest.raises(RuntimeError, match="no CPU"):
        kernels.batch_ssr(images.double(), None, None, 4, rays=torch.zeros(3, 42, 11), draw=dict(seed=1, step=0))


def test_object_batcher_window_follows_the_reference():
    from intrinsicnerf_amd import batches
    b = batches.ObjectBatcher.__new__(batches.ObjectBatcher)
    b.H, b.W, b.precrop_iters, b.precrop_frac = 400, 400, 500, 0.5
    assert b.window(0) == (100, 100, 200, 200) and b.window(499) == (100, 100, 200, 200) and b.window(500) == (0, 0, 400, 400)
    b.H, b.W, b.precrop_frac = 6, 7, 0.7
    assert b.window(0) == (1, 1, 4, 4)                     # dH = int(3 * 0.7) = 2, dW = int(3 * 0.7) = 2  (run_nerf.py:903-904)
    b.H, b.W, b.precrop_frac = 378, 504, 0.5
    assert b.window(0) == (95, 126, 188, 252)              # odd dH: int(189 * 0.5) = 94


BATCH_STAND_IN = dict(STAND_IN)
BATCH_STAND_IN["SSR/models/rays.py"] = STAND_IN["SSR/models/rays.py"] + "def sampling_index(*args, **kwargs):\n    raise NotImplementedError('stand-in')\n"
BATCH_STAND_IN["SSR/training/trainer.py"] = STAND_IN["SSR/training/trainer.py"] + \
    "    def sample_data(self, *args, **kwargs):\n        raise NotImplementedError('stand-in')\n"


@pytest.fixture(scope="module")
def batch_ref(tmp_path_factory):
    root = os.environ.get("INERF_REFERENCE_ROOT")
    if root:
        return root
    base = tmp_path_factory.mktemp("launcher_batches_stand_in")
    for rel, text in BATCH_STAND_IN.items():
        path = base / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(textwrap.dedent(text).lstrip("\n"))
    return str(base)


WITH_BATCHES = PRELUDE + r'''
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py")
trainer = sys.modules["SSR.training.trainer"]
rays_mod = sys.modules["SSR.models.rays"]
assert trainer.SSRTrainer.sample_data.__code__.co_filename.endswith("SSR/training/trainer.py")       # without the flag: the reference's
plain = {k: v for k, v in vars(trainer.SSRTrainer).items()}
bound_plain = {k: list(v) for k, v in mod.__inerf_bound__.items()}
draw = rays_mod.sampling_index
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py", batches=True)
trainer = sys.modules["SSR.training.trainer"]
assert trainer.SSRTrainer.sample_data is ssr.SSRRenderMixin.sample_data
assert sys.modules["SSR.models.rays"].sampling_index is draw and draw.__code__.co_filename.endswith("SSR/models/rays.py")   # the draws stay the reference's
now = vars(trainer.SSRTrainer)
changed = sorted(k for k in set(plain) | set(now) if plain.get(k) is not now.get(k))
assert changed == ["sample_data"], changed
bound = mod.__inerf_bound__
assert bound["SSR.training.trainer.SSRTrainer"] == bound_plain["SSR.training.trainer.SSRTrainer"] + ["sample_data"]
assert {k: v for k, v in bound.items() if k != "SSR.training.trainer.SSRTrainer"} == {k: v for k, v in bound_plain.items() if k != "SSR.training.trainer.SSRTrainer"}
for name in ("step", "init_rays", "set_params", "prepare_data_replica"):
    assert getattr(trainer.SSRTrainer, name).__code__.co_filename.endswith("SSR/training/trainer.py"), name
# the object level: nothing to bind (the batch code is inline in train()); the launcher says so, once
import contextlib, io
err = io.StringIO()
with contextlib.redirect_stderr(err):
    mod, main = launch.prepare(%(ref)r + "/object_level/run_nerf.py", batches=True)
    launch.prepare(%(ref)r + "/object_level/run_nerf.py", batches=True)
assert err.getvalue().count("--inerf-batches") == 1 and "ObjectBatcher" in err.getvalue(), err.getvalue()
assert set(mod.__inerf_bound__) == set(launch.OBJECT_SYMBOLS)
assert mod.train.__code__.co_filename.endswith("object_level/run_nerf.py")
print("batches flag ok")
'''


def test_batches_flag_binds_sample_data_and_nothing_else(batch_ref):
    assert "batches flag ok" in _run(WITH_BATCHES, batch_ref)


def test_batches_flag_is_parsed_and_passed_by_keyword_only_when_given(monkeypatch):
    import sys
    from intrinsicnerf_amd import _capi, launch
    seen = []
    fake = lambda *a, **k: seen.append((a, k)) or (type("M", (), {"__dict__": {}})(), compile("", "x", "exec"))
    monkeypatch.setattr(launch, "prepare", fake)
    monkeypatch.setattr(_capi, "lib", lambda: None)
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    launch.main(["train_SSR_main.py", "--inerf-batches", "--config_file", "x.yaml"])
    assert seen[-1] == (("train_SSR_main.py", False, False, False), {"batches": True}) and sys.argv[1:] == ["--config_file", "x.yaml"]
    launch.main(["train_SSR_main.py", "--inerf-adam", "--inerf-batches"])
    assert seen[-1] == (("train_SSR_main.py", False, False, False), {"adam": True, "batches": True})
    launch.main(["train_SSR_main.py"])
    assert seen[-1] == (("train_SSR_main.py", False, False), {})                    # a stand-in with fewer arguments keeps working
