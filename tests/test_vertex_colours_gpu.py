"""The vertex-colour pass of mesh extraction on the device: inerf_vertex_rays against torch's CPU tensors (tests/golden/vertex_rays.npz)
and against inerf_assemble_rays, inerf_vertex_colours against inerf_frame_to_u8 and inerf_sem_maps, and geometry.vertex_colours /
SSRRenderMixin.vertex_colours end to end against the composed path on a tiny trainer.

Sizes, next to the kernels' constants: the ray kernel takes 256 vertices per workgroup and the colour kernels 256 (four waves, each one
64-row tile of logits), so n sits either side of 64 (1, 63, 64, 65) and at 4 097 (17 workgroups, a ragged last one).  C = 1, 2, 28, 101
and INERF_MAX_CLASSES (240: the library's limit lies below 256) take 1, 2, 32, 64 and 64 lanes per logits row."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

GUARD = 67
NEAR, FAR = 0.1, 10.0


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def fx():
    return load_golden("vertex_rays")


def torch_rays(vertices, normals, near_t):
    """the [n, 11] batch by torch on the CPU, from float32 or float64 numpy rows"""
    rays_d = -torch.FloatTensor(normals)
    near = NEAR * torch.ones_like(rays_d[:, :1])
    far = FAR * torch.ones_like(rays_d[:, :1])
    rays_o = torch.FloatTensor(vertices) - rays_d * near * near_t
    viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    return torch.cat([rays_o, rays_d, near, far, viewdirs], -1)


# ---------------------------------------------------------------------------------------------------------------------
# inerf_vertex_rays
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_vertex_rays_are_the_reference_bits(fx, dt, n):
    from intrinsicnerf_amd import geometry, kernels
    rows = np.arange(n) % fx["vertices_" + dt].shape[0]                    # the fixture's rows, tiled
    v, m = fx["vertices_" + dt][rows], fx["normals_" + dt][rows]
    for i, near_t in enumerate(fx["near_t"]):
        want = fx[f"rays_{dt}_{i}"][rows]
        got = kernels.vertex_rays(torch.from_numpy(v).to(_dev()), torch.from_numpy(m).to(_dev()), NEAR, FAR, float(near_t))
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n, 11)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (dt, n, near_t)
        got = geometry.vertex_rays(v, m, near_t=float(near_t), device=_dev())          # numpy in, uploaded as it is
        assert got.is_cuda and np.array_equal(bits(got.cpu().numpy()), bits(want)), (dt, n, near_t)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_vertex_rays_of_strided_rows(fx, dt):
    """vertices as columns 1:4 of a [n, 5] tensor, normals as columns 2:5 of a [n, 7] one (row strides 5 and 7 elements; the float64 rows
    start 8 and 16 bytes into theirs)"""
    from intrinsicnerf_amd import kernels
    for n in (1, 65, 4097):
        rows = np.arange(n) % 100
        v, m = torch.from_numpy(fx["vertices_" + dt][rows]), torch.from_numpy(fx["normals_" + dt][rows])
        wide_v, wide_m = torch.full((n, 5), 99.0, dtype=v.dtype, device=_dev()), torch.full((n, 7), -99.0, dtype=m.dtype, device=_dev())
        wide_v[:, 1:4], wide_m[:, 2:5] = v.to(_dev()), m.to(_dev())
        got = kernels.vertex_rays(wide_v[:, 1:4], wide_m[:, 2:5], NEAR, FAR, 0.3)
        assert np.array_equal(bits(got.cpu().numpy()), bits(fx[f"rays_{dt}_2"][rows])), (dt, n)


def test_vertex_rays_equal_assemble_rays_on_torch_origins_and_directions(fx):
    from intrinsicnerf_amd import kernels
    rows = np.arange(4097) % 100
    for dt in ("f64", "f32"):
        v, m = fx["vertices_" + dt][rows], fx["normals_" + dt][rows]
        for near_t in (2.0, 0.0, 0.3):
            ref = torch_rays(v, m, near_t)
            want = kernels.assemble_rays(ref[:, 0:3].contiguous().to(_dev()), ref[:, 3:6].contiguous().to(_dev()), NEAR, FAR)
            got = kernels.vertex_rays(torch.from_numpy(v).to(_dev()), torch.from_numpy(m).to(_dev()), NEAR, FAR, near_t)
            assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy())), (dt, near_t)


# ---------------------------------------------------------------------------------------------------------------------
# inerf_vertex_colours
# ---------------------------------------------------------------------------------------------------------------------
def _guarded_u8(n):
    buf = torch.full((n + 2 * GUARD, 3), 0xAB, dtype=torch.uint8, device=_dev())
    return buf, buf[GUARD:GUARD + n]


def _guarded_i32(n):
    buf = torch.full((n + 2 * GUARD,), -77, dtype=torch.int32, device=_dev())
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, value):
    return bool((buf[:GUARD] == value).all()) and bool((buf[GUARD + n:] == value).all())


def colour_values():
    """every k / 255 and its two neighbours, values outside [0, 1], zeros of both signs, infinities and NaN"""
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    edge = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))])
    q = (np.arange(256, dtype=np.float32) / np.float32(255.0))             # ... and the fp32 quotient, where it differs
    special = np.array([-0.0, 0.0, -1e-45, 1e-45, -0.5, -3e38, 1.5, 3e38, 0.999999, 1.0000001, np.inf, -np.inf, np.nan, -np.nan, 0.5, 0.25],
                       np.float32)
    return np.concatenate([special, edge, q])


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_colour_mode_is_frame_to_u8(n):
    from intrinsicnerf_amd import kernels
    vals = colour_values()
    for shift in (0, 5, 12):                                               # (n = 1 and 65 see the specials at the front)
        x = torch.from_numpy(np.roll(vals, -shift)[np.arange(3 * n) % vals.size].reshape(n, 3)).to(_dev())
        want = kernels.frame_to_u8(x).cpu().numpy()
        buf, out = _guarded_u8(n)
        got, labels = kernels.vertex_colours(rgb=x, out=out)
        assert got is out and labels is None and _guards_intact(buf, n, 0xAB)
        assert np.array_equal(out.cpu().numpy(), want), (n, shift)
        xn = x.cpu().numpy()
        ok = ~np.isnan(xn)                                                 # numpy's own cast, where it is defined
        with np.errstate(invalid="ignore"):
            assert np.array_equal(want[ok], (255 * np.clip(xn, 0, 1)).astype(np.uint8)[ok]) and (want[~ok] == 0).all()
        # rows with a stride: columns 4:7 of a [n, 9] tensor
        wide = torch.full((n, 9), 0.7, device=_dev())
        wide[:, 4:7] = x
        got, _ = kernels.vertex_colours(rgb=wide[:, 4:7])
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (n, shift)


def logit_rows(n, c, seed):
    """[n, c] logits: random rows, exact ties (in value and at the maximum), rows holding NaN and infinities"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, c)) * 3.0).astype(np.float32)
    for r in range(n):
        kind = r % 16
        if kind == 1:
            x[r] = 0.25                                                    # all equal: label 0
        elif kind == 2 and c > 1:
            a, b = sorted(rng.choice(c, 2, replace=False))
            x[r, a] = x[r, b] = 50.0                                       # the maximum twice: the lower index
        elif kind == 3:
            x[r, rng.integers(c)] = np.nan                                 # a NaN anywhere: label 0
        elif kind == 4:
            x[r, rng.integers(c)] = np.inf                                 # a non-finite maximum: label 0
        elif kind == 5 and c > 1:
            x[r, rng.integers(c)] = -np.inf                                # -inf below a finite maximum: the label stands
        elif kind == 6:
            x[r, c - 1] = 60.0                                             # the last class
        elif kind == 7 and c > 2:
            x[r, 1:] = 7.5                                                 # a run of equals from index 1
            x[r, 0] = 7.0
        elif kind == 8:
            x[r] = np.nan
    return x


def host_label(x):
    """the lowest index of the maximum; 0 for a row with a NaN or a non-finite maximum"""
    bad = np.isnan(x).any(1) | ~np.isfinite(np.where(np.isnan(x), 0.0, x).max(1))
    return np.where(bad, 0, np.argmax(np.where(np.isnan(x), -np.inf, x), 1)).astype(np.int32)


@pytest.mark.parametrize("c", [1, 2, 28, 101, 256])
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_semantic_mode_is_the_colour_of_sem_maps_label(n, c):
    from intrinsicnerf_amd import _capi, kernels
    c = min(c, _capi.MAX_CLASSES)                                          # the library's class limit (240) is below 256
    rng = np.random.default_rng(c)
    cmap = rng.integers(0, 256, (c, 3), dtype=np.uint8)
    for row0 in ((0,) if n > 65 else range(0, 16, 5)):                     # small n: start at different kinds of row
        x = logit_rows(n + row0, c, 100 * c + n)[row0:]
        wide = torch.full((n, c + 5), 1e9, device=_dev())                  # logits_stride = C + 5 > C; the neighbours would win
        wide[:, 3:3 + c] = torch.from_numpy(x).to(_dev())
        logits = wide[:, 3:3 + c]
        want_label = kernels.sem_maps(logits, want_entropy=False)[0].cpu().numpy()
        assert np.array_equal(want_label, host_label(x).astype(np.float32)), (n, c)
        buf, out = _guarded_u8(n)
        lbuf, lab = _guarded_i32(n)
        got, got_lab = kernels.vertex_colours(logits=logits, colour_map=torch.from_numpy(cmap).to(_dev()), out=out, labels=lab)
        assert got is out and got_lab is lab and _guards_intact(buf, n, 0xAB) and _guards_intact(lbuf, n, -77)
        assert np.array_equal(lab.cpu().numpy(), want_label.astype(np.int32)), (n, c)
        assert np.array_equal(out.cpu().numpy(), cmap[want_label.astype(np.int64)]), (n, c)
        # contiguous logits, outputs allocated by the launcher, no labels
        got, none = kernels.vertex_colours(logits=logits.contiguous(), colour_map=torch.from_numpy(cmap).to(_dev()))
        assert none is None and np.array_equal(got.cpu().numpy(), cmap[want_label.astype(np.int64)]), (n, c)


# ---------------------------------------------------------------------------------------------------------------------
# end to end on a tiny trainer
# ---------------------------------------------------------------------------------------------------------------------
N_CLASSES, N_VERTICES = 5, 300


def sphere(n):
    """n points of a Fibonacci sphere of radius 0.4 about (0.1, -0.05, 0.2) and their outward unit normals, float64 as open3d gives them"""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    normals = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    return np.array([0.1, -0.05, 0.2]) + 0.4 * normals, normals


# Default-initialised networks (measured on an MI355X) have no positive density anywhere on these rays: every colour is 0 and every
# logit 0, which compares zeros with zeros.  So each trainer comes a second time with the density heads' bias raised to 0.5 - a few
# samples per ray then carry weight, and colours and labels differ from vertex to vertex.
@pytest.fixture(scope="module", params=[(8, None), (0, None), (8, 0.5), (0, 0.5)], ids=["fine", "coarse_only", "fine_dense", "coarse_only_dense"])
def scene(request):
    """(trainer, vertices, normals, colour_map, the composed path's render, dense): one render_rays call on rays built by torch on the CPU"""
    from intrinsicnerf_amd import ssr
    n_importance, density_bias = request.param
    torch.manual_seed(7)
    t = ssr.SSRRenderer(N_CLASSES, N_samples=8, N_importance=n_importance, perturb=0., raw_noise_std=0., device=_dev())
    if density_bias is not None:
        with torch.no_grad():
            for net in (t.ssr_net_coarse, t.ssr_net_fine):
                if net is not None:
                    net.alpha_linear.bias.fill_(density_bias)
    t.return_raw = False
    v, m = sphere(N_VERTICES)
    cmap = np.random.default_rng(3).integers(0, 256, (N_CLASSES, 3), dtype=np.uint8)
    with torch.no_grad():
        ret = t.render_rays(torch_rays(v, m, 2.0).to(_dev()))
    lvl = "fine" if n_importance > 0 else "coarse"
    assert ("rgb_fine" in ret) == (n_importance > 0)
    return t, v, m, cmap, {"rgb": ret["rgb_" + lvl].cpu().numpy(), "sem": ret["sem_logits_" + lvl]}, density_bias is not None


def test_vertex_colours_equal_the_composed_path(scene):
    t, v, m, cmap, ref, dense = scene
    want = (255 * np.clip(ref["rgb"], 0, 1)).astype(np.uint8)
    got = t.vertex_colours(v, m)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (N_VERTICES, 3)
    print("distinct colour bytes:", np.unique(got).size, " rgb range:", float(ref["rgb"].min()), float(ref["rgb"].max()))
    if dense:
        assert np.unique(want).size > 8                                    # (a render that says something)
    assert np.array_equal(got, want)
    assert t.return_raw is False and t.check_numerics is True
    for chunk in (64, 100, 300):
        assert np.array_equal(t.vertex_colours(v, m, chunk=chunk), want), chunk
    # float32 vertices that round to the same numbers, as tensors on the device
    v32, m32 = torch.from_numpy(v).float().to(_dev()), torch.from_numpy(m).float().to(_dev())
    assert np.array_equal(t.vertex_colours(v32, m32, chunk=100), want)


def test_semantic_vertex_colours_equal_the_composed_path(scene):
    from intrinsicnerf_amd import geometry, kernels
    t, v, m, cmap, ref, dense = scene
    label = kernels.sem_maps(ref["sem"], want_entropy=False)[0].cpu().numpy().astype(np.int64)
    print("labels:", np.bincount(label, minlength=N_CLASSES).tolist())
    if dense:
        assert np.array_equal(label, np.argmax(ref["sem"].cpu().numpy(), 1)) and (np.abs(ref["sem"].cpu().numpy()).max(1) > 0).all()
    want = cmap[label]
    assert np.array_equal(t.vertex_colours(v, m, sem=True, colour_map=cmap), want)
    for chunk in (64, 100, 300):
        assert np.array_equal(t.vertex_colours(v, m, sem=True, colour_map=torch.from_numpy(cmap), chunk=chunk), want), chunk
    t.valid_colour_map = torch.from_numpy(cmap).to(_dev())                 # the trainer keeps it on the GPU
    try:
        assert np.array_equal(t.vertex_colours(v, m, sem=True), want)
    finally:
        del t.valid_colour_map
    colours, labels = geometry.vertex_colours(t.render_rays, v, m, sem=True, colour_map=cmap, chunk=100, return_labels=True)
    assert labels.dtype == np.int32 and np.array_equal(labels, label) and np.array_equal(colours, want)
    with pytest.raises(ValueError):
        t.vertex_colours(v, m, sem=True, colour_map=cmap[:4])               # a map with fewer rows than the logits have classes
