"""GPU: the training draws (csrc/draws.h; include/inerf.h, "Training draws").

  * inerf_draw_fill against the NumPy restatement (tests/_draws.py): the uniform streams bit for bit, the normal streams within
    NORMAL_TOL of the fp64 Box-Muller value of the same words, both inside their exact ranges;
  * every drawn entry point against its classic entry point fed with inerf_draw_fill's tensors: bit for bit (a difference can only
    be an indexing or stream mix-up);
  * the front-ends: training-mode renders that do not depend on ``chunk``, a backward that sees its forward's step, a captured
    step that draws anew at every replay, and the guards.

NORMAL_TOL: torch's CPU fp32 evaluation of the same formula differs from fp64 by 1.6e-6 at most over 2^20 word pairs (the rounding
of theta = fp32(2 pi) * u2 alone is worth |z| * 2.4e-7 <= 1.4e-6); the device's logf / sincosf are not libm's: 4 x that.
"""
import warnings

import numpy as np
import pytest
import torch

import _draws

pytestmark = pytest.mark.gpu

NORMAL_TOL = 4 * 1.6e-6
SEED = 0x9E3779B97F4A7C15                 # >= 2^32: both key words are used
BIG_STEP = (3 << 32) + 17                  # >= 2^32: both step words are used


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _precision(monkeypatch):
    monkeypatch.setenv("INERF_PRECISION", "f16x3")


def _state(dev, step=BIG_STEP, seed=SEED):
    from intrinsicnerf_amd import draws
    return draws.DrawState(seed, dev, step=step)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)), what


# ---- inerf_draw_fill against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_per_ray", [1, 3, 4, 5, 63, 64, 65, 192, 1024])
def test_fill_against_the_restatement(dev, n_per_ray):
    from intrinsicnerf_amd import kernels
    ds = _state(dev)
    combos = [(n, b) for n in (1, 7, 257) for b in (0, 5, (1 << 32) - 257)]
    worst = 0.0
    for i, (n_rays, base) in enumerate(combos):
        # the step: a small host value, a host value >= 2^32, or the device counter (which wins over the host field)
        mode = (i + i // 3) % 3                               # every mode with every n_rays and every ray_base
        step = (6, BIG_STEP, BIG_STEP + 1)[mode]
        for stream in range(4):
            a = ds.args(base, 1.0)
            if mode == 2:
                ds.load_state_dict({"seed": SEED, "step": step})
                a.step = 99                                   # ignored: step_dev is set
            else:
                a.step_dev, a.step = None, step
            got = kernels.draw_fill(a, stream, n_rays, n_per_ray, dev).cpu().numpy()
            w = _draws.words(SEED, step, stream, n_rays, 4 * ((n_per_ray + 3) // 4), base)
            if stream in (_draws.JITTER, _draws.U):
                want = _draws.uniform_from(w)[:, :n_per_ray]
                assert np.array_equal(got, want), (stream, n_rays, base, mode)
                assert got.min() >= 0.0 and got.max() < 1.0
            else:
                want = _draws.normal_from(w)[:, :n_per_ray]
                err = float(np.abs(got.astype(np.float64) - want).max())
                worst = max(worst, err)
                assert err <= NORMAL_TOL, (stream, n_rays, base, mode, err)
                assert float(np.abs(got).max()) <= np.float32(_draws.MAX_NORMAL)
    print(f"n_per_ray {n_per_ray}: largest |normal - fp64| = {worst:.3e}")


def test_fill_error_over_many_pairs_and_the_scaling(dev):
    """2^20 word pairs per noise stream in one launch (the figure DESIGN.md quotes), and noise = fp32(z * noise_std), one rounding."""
    ds = _state(dev, step=4)
    for stream in (_draws.NOISE_COARSE, _draws.NOISE_FINE):
        got = ds.fill(stream, 2048, 1024).cpu().numpy()
        want = _draws.normal(SEED, 4, stream, 2048, 1024)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"stream {stream}: largest |normal - fp64| over 2^20 pairs = {err:.3e}")
        assert err <= NORMAL_TOL and float(np.abs(got).max()) <= np.float32(_draws.MAX_NORMAL)
        scaled = ds.fill(stream, 2048, 1024, noise_std=0.37).cpu().numpy()
        assert np.array_equal(scaled, got * np.float32(0.37))
    u = ds.fill(_draws.U, 2048, 1024).cpu().numpy()
    assert np.array_equal(u, _draws.uniform(SEED, 4, _draws.U, 2048, 1024)) and u.max() < 1.0


def test_advance_and_snapshot(dev):
    ds = _state(dev, step=(1 << 32) - 1)
    snap = ds.snapshot()
    before = ds.fill(0, 3, 5)
    ds.advance()
    assert ds.state_dict() == {"seed": SEED, "step": 1 << 32} and int(snap.item()) == (1 << 32) - 1
    after = ds.fill(0, 3, 5)
    assert not torch.equal(before, after)
    from intrinsicnerf_amd import kernels
    _same(kernels.draw_fill(ds.args(step_dev=snap), 0, 3, 5, dev), before, "a snapshot keeps the step it was taken at")
    assert np.array_equal(after.cpu().numpy(), _draws.uniform(SEED, 1 << 32, 0, 3, 5))


# ---- every drawn entry point == its classic entry point fed with draw_fill's tensors -----------------------------------
def _rays(n, seed=0, near=2.0, far=6.0):
    g = torch.Generator().manual_seed(seed)
    d = torch.tensor([[0.0, 0.0, 1.0]]) + 0.2 * torch.randn(n, 3, generator=g)
    view = d / d.norm(dim=-1, keepdim=True)
    o = torch.tensor([[0.3, -0.2, -4.0]]).expand(n, 3)
    return torch.cat([o, d, near * torch.ones(n, 1), far * torch.ones(n, 1), view], -1).contiguous()


BASE = 5


@pytest.mark.parametrize("lindisp", [False, True])
def test_sample_coarse_drawn_equals_classic(dev, lindisp):
    from intrinsicnerf_amd import kernels
    ds = _state(dev)
    n, s = 70, 65                                            # 4 550 samples: several workgroups, no multiple of anything
    rays = _rays(n).to(dev)
    t_vals = torch.linspace(0., 1., s, device=dev)
    want = kernels.sample_coarse(rays, t_vals, ds.fill(_draws.JITTER, n, s, BASE), lindisp)
    _same(kernels.sample_coarse(rays, t_vals, None, lindisp, draw=ds.args(BASE)), want, "z_vals")
    assert not torch.equal(want, kernels.sample_coarse(rays, t_vals, None, lindisp))


def _composite_case(dev, s, ssr, n=9):
    g = torch.Generator().manual_seed(100 * s + ssr)
    c, feat = (5, 128) if ssr else (0, 0)
    raw = torch.randn(n, s, 11 + c + feat, generator=g)
    raw[..., 3] = raw[..., 3] * 2.0 + 0.5                    # densities on both sides of zero: the noise moves samples across the ReLU
    z = torch.sort(2.0 + 4.0 * torch.rand(n, s, generator=g), -1).values
    return raw.to(dev), z.to(dev), _rays(n, seed=s)[:, 3:6].contiguous().to(dev), c, feat


@pytest.mark.parametrize("s", [1, 64, 65, 192])
@pytest.mark.parametrize("ssr", [False, True])
def test_composite_drawn_equals_classic_forward_and_backward(dev, s, ssr):
    from intrinsicnerf_amd import kernels
    ds = _state(dev)
    raw, z, d, c, feat = _composite_case(dev, s, ssr)
    n = raw.shape[0]
    g = torch.Generator().manual_seed(7)
    shapes = {"rgb": (n, 3), "albedo": (n, 3), "residual": (n, 3), "disp": (n,), "acc": (n,), "depth": (n,), "shading": (n,), "weights": (n, s)}
    if ssr:
        shapes.update(sem=(n, c), feat=(n, feat))
    grads = {k: torch.randn(*shape, generator=g).to(dev) for k, shape in shapes.items()}          # every output gradient set
    for fine, stream in ((False, _draws.NOISE_COARSE), (True, _draws.NOISE_FINE)):
        std = 0.7 if fine else 1.0
        noise = ds.fill(stream, n, s, BASE, noise_std=std)
        draw = ds.args(BASE, std, fine=fine)
        for white in (False, True):
            want = kernels.composite(raw, z, d, noise, white, n_classes=c, feat_dim=feat)
            got = kernels.composite(raw, z, d, None, white, n_classes=c, feat_dim=feat, draw=draw)
            assert set(got) == set(want)
            for k in want:
                _same(got[k], want[k], (k, fine, white))
            _same(kernels.composite_backward(raw, z, d, grads, None, white, c, feat, draw=draw),
                  kernels.composite_backward(raw, z, d, grads, noise, white, c, feat), ("d_raw", fine, white))
        plain = kernels.composite(raw, z, d, None, False, n_classes=c, feat_dim=feat)
        assert s == 1 or not torch.equal(plain["weights"], want["weights"])
    coarse, fine = (kernels.composite(raw, z, d, None, draw=ds.args(BASE, 1.0, fine=f))["weights"] for f in (False, True))
    assert s == 1 or not torch.equal(coarse, fine)                                                    # two streams


@pytest.mark.parametrize("sc,ni", [(3, 1), (64, 128), (65, 127)])
def test_sample_fine_drawn_equals_classic(dev, sc, ni):
    from intrinsicnerf_amd import kernels
    ds = _state(dev)
    n = 9
    g = torch.Generator().manual_seed(sc)
    z = torch.sort(2.0 + 4.0 * torch.rand(n, sc, generator=g), -1).values.to(dev)
    w = torch.rand(n, sc, generator=g).pow(4).to(dev)
    want = kernels.sample_fine(z, w, ds.fill(_draws.U, n, ni, BASE), ni)
    got = kernels.sample_fine(z, w, None, ni, draw=ds.args(BASE))
    for name, a, b in zip(("z_samples", "z_merged", "z_std"), got, want):
        _same(a, b, name)


def test_sample_pdf_drawn_equals_classic(dev):
    from intrinsicnerf_amd import kernels
    ds = _state(dev)
    n, nb, ns = 9, 64, 128
    g = torch.Generator().manual_seed(1)
    bins = torch.sort(torch.rand(n, nb, generator=g), -1).values.to(dev)
    w = torch.rand(n, nb - 1, generator=g).to(dev)
    _same(kernels.sample_pdf(bins, w, None, ns, draw=ds.args(BASE)), kernels.sample_pdf(bins, w, ds.fill(_draws.U, n, ns, BASE), ns), "samples")


@pytest.fixture(scope="module")
def nets(dev):
    """Both front-ends with calibrated default-initialised networks, and 40 rays for each (computed once)."""
    from intrinsicnerf_amd import object_level as ol, ssr
    from oracle import calibration as cal
    n, C_ = 40, 5
    rays_o = _rays(n)
    embed, ch = ol.get_embedder(10, 0)
    embed_d, ch_d = ol.get_embedder(4, 0)
    mk = lambda: ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
    net_c, net_f = mk(), mk()
    net_c.load_state_dict(cal.calibrated_default_init("object", 0, 0, rays_o))
    net_f.load_state_dict(cal.calibrated_default_init("object", 0, 1, rays_o))
    g = torch.Generator().manual_seed(2)
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    rays_s = torch.cat([torch.tensor([[0.5, 0.2, 0.1]]).expand(n, 3), d, 0.1 * torch.ones(n, 1), 10 * torch.ones(n, 1), d], -1).contiguous()
    sd = [cal.calibrated_default_init("ssr", C_, lvl, rays_s) for lvl in (0, 1)]

    def renderer(**kw):
        r = ssr.SSRRenderer(C_, white_bkgd=False, endpoint_feat=False, device=dev, **kw)
        r.ssr_net_coarse.load_state_dict(sd[0])
        if r.ssr_net_fine is not None:
            r.ssr_net_fine.load_state_dict(sd[1])
        r.training, r.check_numerics = True, False
        return r

    return {"ol": ol, "ssr": ssr, "object": (net_c, net_f, ol.NetworkQuery(embed, embed_d)), "rays_object": rays_o.to(dev),
            "renderer": renderer, "rays_ssr": rays_s.to(dev), "classes": C_}


@pytest.mark.parametrize("variant", ["object", "ssr"])
def test_render_rays_drawn_equals_classic(dev, nets, variant):
    """inerf_render_rays_drawn against inerf_render_rays on 7 rays at 64 + 128: every map, z_std, the stage tensors and raw_*."""
    from intrinsicnerf_amd import kernels, packing
    ds = _state(dev)
    n, sc, ni, std = 7, 64, 128, 0.8
    if variant == "object":
        net_c, net_f, q = nets["object"]
        desc = nets["ol"]._fusable(net_c, q.embed_fn, q.embeddirs_fn)
        rays = nets["rays_object"][:n].contiguous()
    else:
        r = nets["renderer"]()
        net_c, net_f = r.ssr_net_coarse, r.ssr_net_fine
        desc = nets["ssr"]._fusable(net_c, r.embed_fn, r.embeddirs_fn)
        rays = nets["rays_ssr"][:n].contiguous()
    assert desc is not None
    pc, pf = packing.packed_for_module(net_c, desc, dev), packing.packed_for_module(net_f, desc, dev)
    t_vals = torch.linspace(0., 1., sc, device=dev)
    for want_raw in (False, True):
        kw = dict(white_bkgd=variant == "object", want_raw_coarse=want_raw, want_raw_fine=want_raw, want_stages=True)
        want = kernels.render_rays_fused(desc, pc, pf, rays, sc, ni, t_vals, ds.fill(_draws.U, n, ni, BASE), ds.fill(_draws.JITTER, n, sc, BASE),
                                         ds.fill(_draws.NOISE_COARSE, n, sc, BASE, std), ds.fill(_draws.NOISE_FINE, n, sc + ni, BASE, std), **kw)
        got = kernels.render_rays_fused(desc, pc, pf, rays, sc, ni, t_vals, draw=ds.args(BASE, std, perturb=True), **kw)
        assert set(got) == set(want) and ("raw_fine" in got) == want_raw and "z_std" in got
        for k in want:
            _same(got[k], want[k], (variant, k))
        assert int(got["status"].max()) == 0
    # noise only (perturb == 0: nothing is drawn that the reference does not draw - the shared linspace u stays the caller's)
    u = torch.linspace(0., 1., ni, device=dev)
    want = kernels.render_rays_fused(desc, pc, pf, rays, sc, ni, t_vals, u, None, ds.fill(_draws.NOISE_COARSE, n, sc, BASE, std),
                                     ds.fill(_draws.NOISE_FINE, n, sc + ni, BASE, std), want_stages=True)
    got = kernels.render_rays_fused(desc, pc, pf, rays, sc, ni, t_vals, u, draw=ds.args(BASE, std), want_stages=True)
    for k in want:
        _same(got[k], want[k], (variant, "noise only", k))
    # jitter and u only
    want = kernels.render_rays_fused(desc, pc, pf, rays, sc, ni, t_vals, ds.fill(_draws.U, n, ni, BASE), ds.fill(_draws.JITTER, n, sc, BASE), want_stages=True)
    got = kernels.render_rays_fused(desc, pc, pf, rays, sc, ni, t_vals, draw=ds.args(BASE, 0., perturb=True), want_stages=True)
    for k in want:
        _same(got[k], want[k], (variant, "perturb only", k))


# ---- the front-ends ---------------------------------------------------------------------------------------------------------
STEP0 = 11


def _object_call(nets, dev, chunk, grad, draws="new", **over):
    ol = nets["ol"]
    net_c, net_f, q = nets["object"]
    ds = _state(dev, step=STEP0) if draws == "new" else draws
    kw = dict(network_fn=net_c, network_fine=net_f, network_query_fn=q, N_samples=16, N_importance=16, white_bkgd=True, perturb=1.,
              raw_noise_std=1., retraw=True, draws=ds)
    kw.update(over)
    for p in list(net_c.parameters()) + list(net_f.parameters()):
        p.grad = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.enable_grad() if grad else torch.no_grad():
            ret = ol.batchify_rays(nets["rays_object"], chunk, **kw)
            if grad:
                assert ret["rgb_map"].grad_fn is not None
                (ret["rgb_map"].square().mean() + ret["rgb0"].square().mean() + 0.1 * ret["albedo_map"].abs().mean()
                 + 0.1 * ret["acc_map"].mean()).backward()
    grads = [p.grad.detach().clone() for p in list(net_c.parameters()) + list(net_f.parameters())] if grad else None
    return {k: v.detach() for k, v in ret.items()}, grads, ds


def _ssr_call(nets, dev, chunk, grad, with_draws=True, **over):
    r = nets["renderer"](N_samples=16, N_importance=16, chunk=chunk, **dict(dict(perturb=1., raw_noise_std=1.), **over))
    ds = _state(dev, step=STEP0) if with_draws else None
    r.draws = ds
    params = list(r.ssr_net_coarse.parameters()) + list(r.ssr_net_fine.parameters())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.enable_grad() if grad else torch.no_grad():
            if not grad:
                for p in params:
                    p.requires_grad_(False)
            ret = r.render_rays(nets["rays_ssr"])
            if grad:
                assert ret["rgb_fine"].grad_fn is not None
                (ret["rgb_fine"].square().mean() + ret["rgb_coarse"].square().mean() + 0.1 * ret["sem_logits_fine"].square().mean()
                 + 0.1 * ret["acc_fine"].mean()).backward()
    grads = [p.grad.detach().clone() for p in params] if grad else None
    return {k: v.detach() for k, v in ret.items()}, grads, ds


def _assert_chunk_invariant(call, grad):
    """Every returned tensor bit for bit for chunk = 40, 16 and 7.  The parameter gradients cannot be: each chunk is its own set of
    autograd nodes, every node's weight-gradient products are scaled by that node's largest |dz| and summed over its own points, and
    autograd adds the chunks' gradients in its own order - they are held to the bound tests/test_backward_golden.py uses for parameter
    gradients (2e-4 of the tensor's norm)."""
    ref, ref_grads, ds = call(40)
    assert ds.state_dict()["step"] == STEP0 + 1                           # one advance per top-level call
    assert all(bool(torch.isfinite(v).all()) for k, v in ref.items() if not k.startswith("disp"))
    for chunk in (16, 7):
        got, grads, ds = call(chunk)
        assert ds.state_dict()["step"] == STEP0 + 1
        assert set(got) == set(ref)
        for k in ref:
            _same(got[k], ref[k], (chunk, k))
        if grad:
            assert len(grads) == len(ref_grads)
            for i, (a, b) in enumerate(zip(grads, ref_grads)):
                assert float((a.double() - b.double()).norm()) <= 2e-4 * float(b.double().norm()) + 1e-10, (chunk, i)
    return ref


@pytest.mark.parametrize("grad", [False, True], ids=["fused", "staged-autograd"])
def test_object_level_render_does_not_depend_on_chunk(dev, nets, grad):
    ref = _assert_chunk_invariant(lambda chunk: _object_call(nets, dev, chunk, grad), grad)
    other = _object_call(nets, dev, 40, grad, draws=_state(dev, step=STEP0 + 1))[0]
    assert not torch.equal(other["rgb_map"], ref["rgb_map"]) and not torch.equal(other["z_std"], ref["z_std"])      # the next step draws anew


@pytest.mark.parametrize("grad", [False, True], ids=["fused", "staged-autograd"])
def test_ssr_render_does_not_depend_on_chunk(dev, nets, grad):
    _assert_chunk_invariant(lambda chunk: _ssr_call(nets, dev, chunk, grad), grad)


def test_backward_sees_the_forwards_step(dev):
    from intrinsicnerf_amd import kernels
    raw, z, d, c, feat = _composite_case(dev, 65, True)
    n, s = z.shape
    outs = []
    for advance in (False, True):
        ds = _state(dev, step=STEP0)
        leaf = raw.clone().requires_grad_(True)
        o = kernels.composite(leaf, z, d, None, True, n_classes=c, feat_dim=feat, draw=ds.args(BASE, 1.0, fine=True))
        assert type(o["rgb"].grad_fn).__name__ == "_CompositeFnBackward"
        assert len(o["rgb"].grad_fn.saved_tensors) == 3, "raw, z_vals and rays_d: no noise tensor is kept"
        if advance:
            ds.advance()
            ds.advance()
        (o["rgb"].square().sum() + o["sem"].sum() + o["depth"].sum() + o["feat"].abs().sum()).backward()
        outs.append((o["rgb"].detach(), leaf.grad.clone()))
    _same(outs[0][0], outs[1][0], "forward")
    _same(outs[0][1], outs[1][1], "gradient after advance()")
    ds = _state(dev, step=STEP0)
    leaf = raw.clone().requires_grad_(True)
    o = kernels.composite(leaf, z, d, ds.fill(_draws.NOISE_FINE, n, s, BASE), True, n_classes=c, feat_dim=feat)
    (o["rgb"].square().sum() + o["sem"].sum() + o["depth"].sum() + o["feat"].abs().sum()).backward()
    _same(leaf.grad, outs[0][1], "gradient against the classic node that keeps its noise")


def test_captured_step_draws_anew_at_every_replay(dev, nets, monkeypatch):
    from intrinsicnerf_amd import kernels
    ol = nets["ol"]
    net_c, net_f, q = nets["object"]
    params = list(net_c.parameters()) + list(net_f.parameters())
    rays = nets["rays_object"][:8].contiguous()

    def step_fn(ds):
        for p in params:
            p.grad = None
        ret = ol.render_rays(rays, net_c, q, 8, retraw=True, perturb=1., N_importance=8, network_fine=net_f, white_bkgd=True,
                             raw_noise_std=1., draws=ds)
        (ret["rgb_map"].square().mean() + ret["rgb0"].square().mean()).backward()
        return ret

    def record(ret):
        return {k: v.detach().clone() for k, v in ret.items()}, [p.grad.detach().clone() for p in params]

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eager_ds = _state(dev, step=STEP0)
        eager = [record(step_fn(eager_ds)) for _ in range(2)]
        assert eager_ds.state_dict()["step"] == STEP0 + 2
        ds = _state(dev, step=STEP0)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            step_fn(ds)                                                       # warm-up: allocator pools, lazily built tables
        torch.cuda.current_stream(dev).wait_stream(side)
        ds.load_state_dict({"seed": SEED, "step": STEP0})
        torch.cuda.synchronize(dev)
        rng_before = torch.cuda.get_rng_state(dev)
        monkeypatch.setattr(kernels, "captured_status", [])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ret = step_fn(ds)
        assert ds.state_dict()["step"] == STEP0                                # capturing ran nothing
        replays = []
        for _ in range(2):
            graph.replay()
            replays.append(record(ret))
        assert ds.state_dict()["step"] == STEP0 + 2
    assert torch.equal(torch.cuda.get_rng_state(dev), rng_before), "torch's generator took no part in the captured step"
    for k in ("z_std", "rgb_map", "raw"):                                      # different depths, different noise
        assert not torch.equal(replays[0][0][k], replays[1][0][k]), k
    for i in range(2):
        for k in eager[i][0]:
            _same(replays[i][0][k], eager[i][0][k], (i, k))
        for j, (a, b) in enumerate(zip(replays[i][1], eager[i][1])):
            _same(a, b, (i, "grad", j))


def test_front_end_guards(dev, nets):
    ol = nets["ol"]
    net_c, net_f, q = nets["object"]
    rays = nets["rays_object"][:8]
    ds = _state(dev)
    with pytest.raises(ValueError, match="pytest"):
        ol.render_rays(rays, net_c, q, 16, N_importance=16, network_fine=net_f, perturb=1., pytest=True, draws=ds)
    # nothing to draw: the bits of the call without a DrawState, in both front-ends
    with_ds, _, state = _object_call(nets, dev, 16, False, perturb=0., raw_noise_std=0.)
    assert state.state_dict()["step"] == STEP0                              # nothing drawn: the step counts drawing renders only
    without = _object_call(nets, dev, 16, False, draws=None, perturb=0., raw_noise_std=0.)[0]
    assert set(with_ds) == set(without)
    for k in without:
        _same(with_ds[k], without[k], ("object", k))
    with_ds, _, state = _ssr_call(nets, dev, 16, False, perturb=0., raw_noise_std=0.)
    assert state.state_dict()["step"] == STEP0
    without = _ssr_call(nets, dev, 16, False, with_draws=False, perturb=0., raw_noise_std=0.)[0]
    for k in without:
        _same(with_ds[k], without[k], ("ssr", k))
    # eval mode of the SSR mixin draws nothing either, whatever perturb / raw_noise_std say
    r = nets["renderer"](N_samples=16, N_importance=16, chunk=16, perturb=1., raw_noise_std=1.)
    r.training = False
    with torch.no_grad():
        a = r.render_rays(nets["rays_ssr"])
        r.draws = _state(dev)
        b = r.render_rays(nets["rays_ssr"])
    for k in a:
        _same(a[k], b[k], ("ssr eval", k))
    assert r.draws.state_dict()["step"] == BIG_STEP


def test_graphed_train_step_with_draws(dev, nets):
    """graphs.GraphedTrainStep(draws=...): its warm-up steps leave the counter where it was, every replay draws at the next step and
    equals the eager step there, and a batch that leaves the f16 range is re-run eagerly with the draws of the replay it replaces."""
    from intrinsicnerf_amd import graphs
    ol = nets["ol"]
    q = nets["object"][2]
    rays = nets["rays_object"][:8].contiguous()
    target = torch.rand(8, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    losses = {}
    for mode in ("eager", "graph"):
        net_c, net_f = (type(m)(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True).to(dev) for m in nets["object"][:2])
        net_c.load_state_dict(nets["object"][0].state_dict()); net_f.load_state_dict(nets["object"][1].state_dict())
        params = list(net_c.parameters()) + list(net_f.parameters())
        opt = torch.optim.Adam(params, lr=1e-4, capturable=True)
        ds = _state(dev, step=STEP0)

        def loss_fn(r, t):
            ret = ol.render_rays(r, net_c, q, 8, retraw=True, perturb=1., N_importance=8, network_fine=net_f, white_bkgd=True,
                                 raw_noise_std=1., draws=ds)
            return ((ret["rgb_map"] - t) ** 2).mean() + ((ret["rgb0"] - t) ** 2).mean()

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            step = graphs.GraphedTrainStep(loss_fn, (rays, target), opt, draws=ds) if mode == "graph" else None
            assert ds.state_dict()["step"] == STEP0                       # the warm-up left no trace
            out = []
            for it in range(3):
                if it == 2:
                    with torch.no_grad():
                        net_f.pts_linears[2].weight.mul_(1.0e6)          # far outside the f16 range: the guarded fallback
                if step is None:
                    opt.zero_grad(set_to_none=True)
                    loss = loss_fn(rays, target)
                    loss.backward()
                    opt.step()
                else:
                    loss = step(rays, target)
                out.append(float(loss))
                assert ds.state_dict()["step"] == STEP0 + it + 1
        if step is not None:
            assert step.fallbacks == 1
        losses[mode] = out
    assert np.isfinite(losses["graph"]).all() and losses["graph"][0] != losses["graph"][1]
    assert losses["graph"] == losses["eager"], losses
