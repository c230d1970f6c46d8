"""GPU: every ray batch the object-level front-end hands to batchify_rays comes out of one HIP launch with the reference's CPU bits -
pose -> NDC frames (inerf_gen_rays_ndc), given rays with and without NDC (inerf_assemble_rays), ndc_rays alone (inerf_ndc_rays).
Every comparison is bit for bit: against the real reference's fixtures, and against the front-end's CPU expressions, which
reproduce those fixtures bit for bit (tests/test_frontends_cpu.py, tests/test_ray_forms_cpu.py).  No tolerance anywhere."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _cpu_batch(o, d, near, far, ndc=None, view=None):
    """The [n, 11] batch of render()'s torch lines (run_nerf.py:106-128) on CPU tensors; ``ndc`` = (H, W, focal, near_plane)."""
    from intrinsicnerf_amd import object_level as ol
    v = d if view is None else view
    v = (v / torch.norm(v, dim=-1, keepdim=True)).reshape(-1, 3)
    if ndc is not None:
        o, d = ol.ndc_rays(ndc[0], ndc[1], ndc[2], ndc[3], o, d)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    return torch.cat([o, d, near * torch.ones_like(d[..., :1]), far * torch.ones_like(d[..., :1]), v], -1)


def _coeff(H, W, focal, near_plane):
    from intrinsicnerf_amd import object_level as ol
    return ol._ndc_coefficients(H, W, focal, near_plane)


def _same_words(got, want):
    """Equal as int32 words, -0 and infinities included; NaN exactly where ``want`` has NaN (sign and payload free)."""
    got, want = got.cpu().contiguous(), want.contiguous()
    nan = torch.isnan(want)
    return (got.shape == want.shape and torch.equal(torch.isnan(got), nan)
            and torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan]))


def _forward_rays(n, seed):
    """Random forward-facing rays (o_z around 0, d_z around -1): finite NDC."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g) * torch.tensor([1.0, 1.0, 0.3])
    d = torch.randn(n, 3, generator=g) * 0.5 + torch.tensor([0.0, 0.0, -1.5])
    return o, d


def _spy(monkeypatch, ol, seen):
    def spy(rays_flat, chunk=1024 * 32, **kw):
        seen["rays"] = rays_flat.clone()
        n, dev = rays_flat.shape[0], rays_flat.device
        z3, z1 = torch.zeros(n, 3, device=dev), torch.zeros(n, device=dev)
        return {"rgb_map": z3, "disp_map": z1, "acc_map": z1, "albedo_map": z3, "shading_map": z1, "residual_map": z3}
    monkeypatch.setattr(ol, "batchify_rays", spy)


def test_fixtures_bit_for_bit():
    from intrinsicnerf_amd import kernels
    dev = _dev()
    fx = load_golden("rays_generators")
    H, W, K, focal = int(fx["H"]), int(fx["W"]), fx["K"], fx["K"][0][0]
    c2w = torch.from_numpy(fx["c2w"]).to(dev)
    got = kernels.gen_rays(c2w, H, W, K[0][0], K[1][1], K[0][2], K[1][2], 2.0, 6.0, True, ndc=_coeff(H, W, focal, 1.))
    assert torch.equal(got.cpu(), torch.from_numpy(fx["render_rays_ndc"]))
    ro = torch.from_numpy(fx["get_rays_o"]) + torch.tensor([0.0, 0.0, 4.0])
    o2, d2 = kernels.ndc_rays(ro.to(dev), torch.from_numpy(fx["get_rays_d"]).to(dev), _coeff(H, W, float(fx["focal"]), 1.0))
    assert tuple(o2.shape) == tuple(d2.shape) == (H, W, 3)
    assert torch.equal(o2.cpu(), torch.from_numpy(fx["ndc_o"])) and torch.equal(d2.cpu(), torch.from_numpy(fx["ndc_d"]))
    got = kernels.assemble_rays(torch.from_numpy(fx["given_o"]).to(dev), torch.from_numpy(fx["given_d"]).to(dev), 0.5, 3.0)
    assert torch.equal(got.cpu(), torch.from_numpy(fx["render_rays_given"]))
    # the real reference's LLFF frame: 12 x 16, near 0, far 1
    fl = load_golden("uncurated_object_llff_ndc")
    H, W, K = int(fl["H"]), int(fl["W"]), fl["K"]
    got = kernels.gen_rays(torch.from_numpy(fl["c2w"]).to(dev), H, W, K[0][0], K[1][1], K[0][2], K[1][2], 0., 1., True,
                           ndc=_coeff(H, W, K[0][0], 1.))
    assert torch.equal(got.cpu(), torch.from_numpy(fl["rays"]))


def test_render_hands_over_the_cpu_bits(monkeypatch):
    """render() itself, batch captured in front of batchify_rays, against the same call made with CPU tensors.

    Given rays with ndc=False stay on render()'s torch lines: with the one-launch path taken for them too,
    tests/test_adam_gpu.py::test_three_training_steps_in_place_of_torch_adam measured 4.733 of its 1e-4 bound (0.482 on the bits of
    torch's device norm).  For those cases the copied columns 0:8 and the path taken are checked here, and kernels.assemble_rays on
    the same inputs against the CPU batch, bit for bit."""
    from intrinsicnerf_amd import kernels, object_level as ol
    dev = _dev()
    fx = load_golden("rays_generators")
    H, W, K = int(fx["H"]), int(fx["W"]), fx["K"]
    c2w, c2s = torch.from_numpy(fx["c2w"]), torch.from_numpy(fx["c2w_static"])
    seen = {}
    _spy(monkeypatch, ol, seen)
    launches = []
    for name in ("gen_rays", "assemble_rays"):
        real = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, lambda *a, _n=name, _r=real, **k: (launches.append(_n), _r(*a, **k))[1])

    def both(shape, exact=True, **kw):
        on_dev = {k: (v.to(dev) if isinstance(v, torch.Tensor) else tuple(t.to(dev) for t in v) if isinstance(v, tuple) else v)
                  for k, v in kw.items()}
        launches.clear()
        out = ol.render(H, W, K, chunk=64, use_viewdirs=True, **on_dev)
        got = seen["rays"]
        assert got.is_cuda and tuple(out[0].shape) == shape + (3,) and tuple(out[1].shape) == shape, [m.shape for m in out[:6]]
        n_launch = list(launches)
        ol.render(H, W, K, chunk=64, use_viewdirs=True, **kw)
        assert not seen["rays"].is_cuda and launches == n_launch
        if exact:
            assert torch.equal(got.cpu(), seen["rays"]), kw.keys()
        else:       # the torch lines on the device: origin, direction, near and far are copies; the view directions are torch's device norm
            assert torch.equal(got.cpu()[:, :8], seen["rays"][:, :8]), kw.keys()
        return n_launch, seen["rays"]

    assert both((H, W), c2w=c2w, near=2.0, far=6.0, ndc=True)[0] == ["gen_rays"]
    assert torch.equal(seen["rays"], torch.from_numpy(fx["render_rays_ndc"]))
    assert both((H, W), c2w=c2w, c2w_staticcam=c2s, near=2.0, far=6.0, ndc=True)[0] == ["gen_rays"]
    o, d = _forward_rays(10, 5)
    o, d = o.reshape(2, 5, 3), d.reshape(2, 5, 3)
    r = torch.cat([o.reshape(-1, 3), d.reshape(-1, 3), torch.zeros(10, 5)], -1)                # columns of an [N, 11] batch go in as they are
    assert not r[:, 3:6].is_contiguous()
    coeff = _coeff(H, W, K[0][0], 1.)
    for shape, rays in (((2, 5), (o, d)), ((10,), (r[:, 0:3], r[:, 3:6]))):
        on_dev = tuple(t.to(dev) for t in rays)
        n_launch, want = both(shape, rays=rays, near=0.0, far=1.0, ndc=True)
        assert n_launch == ["assemble_rays"]
        assert torch.equal(kernels.assemble_rays(*on_dev, 0.0, 1.0, ndc=coeff).cpu(), want)
        # ndc=False: render() keeps the torch lines for given rays (an existing test depends on the bits of torch's device norm); the
        # kernel itself gives the CPU's bits for the same inputs
        n_launch, want = both(shape, exact=False, rays=rays, near=0.5, far=3.0, ndc=False)
        assert n_launch == []
        assert torch.equal(kernels.assemble_rays(*on_dev, 0.5, 3.0).cpu(), want)
    # what else stays on the torch lines: a static camera with given rays, autograd
    launches.clear()
    o48, d48 = (t.reshape(H, W, 3).to(dev) for t in _forward_rays(H * W, 6))
    ol.render(H, W, K, chunk=64, use_viewdirs=True, rays=(o48, d48), near=0., far=1., ndc=True, c2w_staticcam=c2s.to(dev))
    ol.render(H, W, K, chunk=64, use_viewdirs=True, rays=(o.to(dev).requires_grad_(True), d.to(dev)), near=0., far=1., ndc=True)
    assert "assemble_rays" not in launches


def test_launcher_input_rules():
    from intrinsicnerf_amd import kernels
    dev = _dev()
    o, d = (t.to(dev) for t in _forward_rays(8, 2))
    with pytest.raises(ValueError):
        kernels.assemble_rays(o.double(), d.double(), 0., 1.)
    with pytest.raises(ValueError):
        kernels.assemble_rays(o[:, :2], d[:, :2], 0., 1.)
    with pytest.raises(ValueError):
        kernels.assemble_rays(o.t().contiguous().t(), d, 0., 1.)               # inner stride 8
    with pytest.raises(ValueError):
        kernels.ndc_rays(o[0].expand(8, 3), d, (-1., -1., 1.))                 # row stride 0
    with pytest.raises(ValueError):
        kernels.assemble_rays(o[:4], d, 0., 1.)
    with pytest.raises(RuntimeError):
        kernels.assemble_rays(o.cpu(), d, 0., 1.)


def test_ragged_sizes():
    from intrinsicnerf_amd import kernels, object_level as ol
    dev = _dev()
    fl = load_golden("uncurated_object_llff_ndc")
    H, W, focal = 19, 27, 20.3                                                # 513 rays per pose: workgroups straddle poses, the last holds 3 rays
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = torch.from_numpy(fl["c2w"])[None].repeat(3, 1, 1)
    poses[1, :, 3] += torch.tensor([0.25, -0.125, 0.0625])
    poses[2, :, 3] -= torch.tensor([0.1, 0.2, 0.3])
    want = []
    for p in poses:
        ro, rd = ol.get_rays(H, W, K, p)
        want.append(_cpu_batch(ro, rd, 0., 1., ndc=(H, W, K[0][0], 1.)))
    got = kernels.gen_rays(poses.to(dev), H, W, K[0][0], K[1][1], K[0][2], K[1][2], 0., 1., True, ndc=_coeff(H, W, K[0][0], 1.))
    assert tuple(got.shape) == (3 * 513, 11) and torch.equal(got.cpu(), torch.cat(want, 0))
    o, d = _forward_rays(513, 3)
    for n in (1, 255, 256, 257, 513):
        for ndc in (None, (H, W, focal, 1.)):
            got = kernels.assemble_rays(o[:n].to(dev), d[:n].to(dev), 0.25, 1.5, ndc=None if ndc is None else _coeff(*ndc))
            assert torch.equal(got.cpu(), _cpu_batch(o[:n], d[:n], 0.25, 1.5, ndc=ndc)), (n, ndc)
        go, gd = kernels.ndc_rays(o[:n].to(dev), d[:n].to(dev), _coeff(H, W, focal, 1.))
        wo, wd = ol.ndc_rays(H, W, focal, 1., o[:n], d[:n])
        assert torch.equal(go.cpu(), wo) and torch.equal(gd.cpu(), wd), n
    # beyond the last ray nothing is written
    out = kernels.assemble_rays(o[:257].to(dev), d[:257].to(dev), 0., 1.)
    assert out.shape[0] == 257


def test_the_workloads_own_frame():
    """378 x 504 (fern at factor 8) with the LLFF fixture's pose: all 190 512 NDC rays."""
    from intrinsicnerf_amd import kernels, object_level as ol
    dev = _dev()
    fl = load_golden("uncurated_object_llff_ndc")
    H, W = 378, 504
    focal = fl["K"][0][0] * 504 / 16
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    pose = torch.from_numpy(fl["c2w"])
    ro, rd = ol.get_rays(H, W, K, pose)
    want = _cpu_batch(ro, rd, 0., 1., ndc=(H, W, K[0][0], 1.))
    got = kernels.gen_rays(pose.to(dev), H, W, K[0][0], K[1][1], K[0][2], K[1][2], 0., 1., True, ndc=_coeff(H, W, K[0][0], 1.))
    assert tuple(got.shape) == (190512, 11) and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("near", [0.7, 0.9, 1.7])
def test_a_near_plane_that_is_no_power_of_two(near):
    """2. * near / o'_z is reciprocal-then-multiply (Tensor.__rtruediv__), not a division.  o'_z lies within a few ulp of -near, so
    whether the two differ depends on the plane: at 0.7 they happen to coincide on these rays, at 0.9 and 1.7 they differ on
    hundreds and thousands of them - there a true division in the kernel fails this test."""
    from intrinsicnerf_amd import kernels, object_level as ol
    dev = _dev()
    o, d = _forward_rays(4096, 7)
    wo, wd = ol.ndc_rays(378, 504, 407.5, near, o, d)
    qz = (o + (-(near + o[:, 2]) / d[:, 2])[:, None] * d)[:, 2]
    assert torch.equal(wo[:, 2], 1. + qz.reciprocal() * (2. * near))
    if near != 0.7:
        assert int((wo[:, 2] != 1. + torch.full_like(qz, 2. * near) / qz).sum()) > 100                       # the trap is in the data
    go, gd = kernels.ndc_rays(o.to(dev), d.to(dev), _coeff(378, 504, 407.5, near))
    assert torch.equal(go.cpu(), wo) and torch.equal(gd.cpu(), wd)
    go, gd = ol.ndc_rays(378, 504, 407.5, near, o.to(dev), d.to(dev))                                          # the front-end's own call
    assert go.is_cuda and torch.equal(go.cpu(), wo) and torch.equal(gd.cpu(), wd)
    got = kernels.assemble_rays(o.to(dev), d.to(dev), 0., 1., ndc=_coeff(378, 504, 407.5, near))
    assert torch.equal(got.cpu(), _cpu_batch(o, d, 0., 1., ndc=(378, 504, 407.5, near)))


def test_special_values():
    from intrinsicnerf_amd import kernels, object_level as ol
    dev = _dev()
    inf = float("inf")
    near = 0.75
    o = torch.tensor([[0.5, -0.25, 1.0], [0.5, -0.25, 1.0], [0.1, 0.2, -near], [0.1, 0.2, -near], [0.0, 0.0, 0.0], [1.0, 2.0, 3.0],
                      [inf, 0.0, 1.0], [1.0, -inf, 1.0], [1.0, 2.0, inf], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [-0.0, -0.0, -near]])
    d = torch.tensor([[0.3, 0.4, 0.0], [0.3, 0.4, -0.0], [0.3, 0.4, -1.0], [0.0, 0.0, -0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0],
                      [0.1, 0.2, -1.0], [0.1, 0.2, -1.0], [0.1, 0.2, -1.0], [inf, 0.2, -1.0], [0.1, -inf, inf], [-0.0, 0.0, -2.0]])
    wo, wd = ol.ndc_rays(12, 16, 12.9, near, o, d)
    want = _cpu_batch(o, d, 0., 1., ndc=(12, 16, 12.9, near))
    assert torch.isnan(want).any() and torch.isinf(want).any() and (want.view(torch.int32) == -2 ** 31).any()      # NaN, inf and -0 occur
    go, gd = kernels.ndc_rays(o.to(dev), d.to(dev), _coeff(12, 16, 12.9, near))
    assert _same_words(go, wo) and _same_words(gd, wd)
    assert _same_words(kernels.assemble_rays(o.to(dev), d.to(dev), 0., 1., ndc=_coeff(12, 16, 12.9, near)), want)
    assert _same_words(kernels.assemble_rays(o.to(dev), d.to(dev), 0., 1.), _cpu_batch(o, d, 0., 1.))


def test_llff_frame_end_to_end_equals_render_rays_on_the_fixture_rays():
    """render(c2w=<device pose>, ndc=True) hands batchify_rays the fixture's bits, so its maps are those of render_rays on the
    fixture's rays uploaded as they are - map for map, NaN-aware bit for bit."""
    from intrinsicnerf_amd import object_level as ol
    from _cases import uncurated_weights
    from test_dropin_gpu import llff_args, reference_style_create_nerf
    dev = _dev()
    fx = load_golden("uncurated_object_llff_ndc")
    H, W, K, pose = int(fx["H"]), int(fx["W"]), fx["K"], torch.from_numpy(fx["c2w"])
    args = llff_args()
    _, test_kw, model, model_fine = reference_style_create_nerf(args, dev)
    sd_c, sd_f = uncurated_weights(fx)
    model.load_state_dict(sd_c); model_fine.load_state_dict(sd_f)
    with torch.no_grad():
        out = ol.render(H, W, K, chunk=args.chunk, c2w=pose.to(dev)[:3, :4], ndc=True, near=0., far=1., **test_kw)
        kw = {k: v for k, v in test_kw.items() if k not in ("ndc", "near", "far", "use_viewdirs")}
        want = ol.render_rays(torch.from_numpy(fx["rays"]).to(dev), **kw)
    names = ("rgb_map", "disp_map", "acc_map", "albedo_map", "shading_map", "residual_map")
    got = dict(zip(names, out[:6]), **out[6])
    assert set(got) == set(want)
    for k in want:
        a, b = got[k].reshape(want[k].shape), want[k]
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), k


def test_capture_and_replay():
    from intrinsicnerf_amd import kernels
    dev = _dev()
    fl = load_golden("uncurated_object_llff_ndc")
    H, W, K = int(fl["H"]), int(fl["W"]), fl["K"]
    coeff = _coeff(H, W, K[0][0], 1.)
    pose = torch.from_numpy(fl["c2w"]).to(dev)
    o, d = (t.to(dev) for t in _forward_rays(300, 11))
    run = lambda: (kernels.gen_rays(pose, H, W, K[0][0], K[1][1], K[0][2], K[1][2], 0., 1., True, ndc=coeff),
                   kernels.assemble_rays(o, d, 0., 1., ndc=coeff))
    first = [t.clone() for t in run()]                                      # (also loads the code objects before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a, b = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, first[0]) and torch.equal(b, first[1])
    o2, d2 = (t.to(dev) for t in _forward_rays(300, 12))
    pose[:, 3] += torch.tensor([0.5, -0.25, 0.125], device=dev)
    o.copy_(o2); d.copy_(d2)
    graph.replay()
    torch.cuda.synchronize()
    direct = run()
    assert not torch.equal(a, first[0]) and not torch.equal(b, first[1])
    assert torch.equal(a, direct[0]) and torch.equal(b, direct[1])
