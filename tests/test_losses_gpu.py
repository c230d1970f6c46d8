"""GPU: the training losses on csrc/losses.hip against the reference's recorded values (tests/golden/loss_*.npz), on both call
styles - ``compute_intrinsic_loss``'s six scalars inside the trainers' own weighted sum, and the fused step loss - at the
project's plain bound (tests/_losses.py: 1e-4 relative per term, RTOL 1e-4 + 1e-5 of the tensor's scale per gradient tensor; the
generator asserts that the reference's own fp32-vs-fp64 distance is ten times smaller).  Then what the kernels promise beyond
values: bit-identical repeats, no ATen arithmetic around them, capture into a graph, and the gradients that reach the
networks' parameters through the staged training path."""
import warnings

import numpy as np
import pytest
import torch

import _losses
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(k, n) for k in ("object", "ssr") for n in _losses.case_names(k)]


def _weights(case):
    return {name: float(w) for name, w in zip(_losses.TERMS, case["weights"])}


def _ret(kind, levels):
    """The render dictionary the fused loss takes, from a fixture's levels (coarse first)."""
    ret = {}
    if kind == "object":
        tags = ["_map"] if len(levels) == 1 else ["0", "_map"]
        for tag, lv in zip(tags, levels):
            for k in ("rgb", "albedo", "shading", "residual"):
                ret[k + tag] = lv[k]
    else:
        for tag, lv in zip(("_coarse", "_fine"), levels):
            for k in ("rgb", "albedo", "shading", "residual"):
                ret[k + tag] = lv[k]
            ret["sem_logits" + tag] = lv["logits"]
    return ret


def _fused(kind, shared, levels, weights):
    from intrinsicnerf_amd import losses
    if kind == "object":
        return losses.object_step_loss(_ret(kind, levels), shared["gt"], shared["key"], weights, shared["target"])
    return losses.ssr_step_loss(_ret(kind, levels), shared["gt"], shared["key"], weights, shared["target"])


def _check_grads(case, levels, name):
    checked = 0
    for l, lv in enumerate(levels):
        for k, v in lv.items():
            assert v.grad is not None, (name, k, l)
            _losses.assert_gradient(v.grad, case[f"g_{k}{l}"], f"{name} g_{k}{l}")
            checked += 1
    assert checked == sum(1 for k in case if k.startswith("g_"))


@pytest.mark.parametrize("kind,name", CASES)
def test_six_scalars_in_the_trainers_own_sum(kind, name):
    """compute_intrinsic_loss as the launcher binds it: the trainer adds img2mse, the cluster MSE and the cross-entropy itself
    (run_nerf.py:976-1013, trainer.py:923-988) and weighs the six terms - one backward launch per level."""
    from intrinsicnerf_amd import object_level as ol, ssr
    case = _losses.cases(kind)[name]
    shared, levels = _losses.tensors(case, DEV)
    fn = ol.compute_intrinsic_loss if kind == "object" else ssr.compute_intrinsic_loss
    w = case["weights"]
    mse = lambda x, y: torch.mean((x - y) ** 2)
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1)
    total = 0
    for l, lv in enumerate(levels):
        six = fn(lv["albedo"], lv["shading"], lv["residual"], shared["gt"], None, None, shared["key"])
        assert len(six) == 6 and all(t.dim() == 0 for t in six)
        got = torch.stack([t.detach() for t in six]).cpu().numpy()
        print(name, "level", l, "six", got, "want", case[f"terms{l}"][:6])
        _losses.assert_terms(got, case[f"terms{l}"][:6], f"{name} level {l}")
        total = total + sum(float(w[k]) * six[k] for k in range(6)) + float(w[6]) * mse(lv["rgb"], shared["gt"])
        if shared["target"] is not None:
            total = total + float(w[7]) * mse(lv["albedo"], shared["target"])
        if "logits" in lv:
            total = total + float(w[8]) * ce(lv["logits"], shared["key"] - 1)
    total.backward()
    _losses.assert_terms([float(total)], [float(case["total"])], f"{name} total")
    _check_grads(case, levels, name)


@pytest.mark.parametrize("kind,name", CASES)
def test_fused_step_loss(kind, name):
    case = _losses.cases(kind)[name]
    shared, levels = _losses.tensors(case, DEV)
    total, terms = _fused(kind, shared, levels, _weights(case))
    want_present = [t for t, on in zip(_losses.TERMS, _losses.present(shared, levels[0])) if on]
    assert list(terms) == want_present and total.dim() == 0
    for l in range(len(levels)):
        got = np.array([float(terms[t][l]) if t in terms else 0.0 for t in _losses.TERMS])
        print(name, "level", l, "terms", got, "want", case[f"terms{l}"])
        _losses.assert_terms(got, case[f"terms{l}"], f"{name} level {l}")
    _losses.assert_terms([float(total)], [float(case["total"])], f"{name} total")
    total.backward()
    _check_grads(case, levels, name)


def test_gradient_through_a_returned_term():
    """A caller may also differentiate the terms dictionary (logging a term with its own weight): both upstream paths add up."""
    case = _losses.cases("object")["n512_step"]
    shared, levels = _losses.tensors(case, DEV)
    w = _weights(case)
    total, terms = _fused("object", shared, levels, w)
    (total + 0.25 * terms["far"][1] + 0.5 * terms["image"][0]).backward()
    shared2, levels2 = _losses.tensors(case, DEV)
    w0 = dict(w, image=w["image"] + 0.5)
    w1 = dict(w, far=w["far"] + 0.25)
    from intrinsicnerf_amd import losses
    for l, wl in ((0, w0), (1, w1)):          # the same thing from per-level weights: one single-level call each
        lv = levels2[l]
        t, _ = losses.object_step_loss({k + "_map": lv[k] for k in ("rgb", "albedo", "shading", "residual")}, shared2["gt"], shared2["key"], wl,
                                       shared2["target"])
        t.backward()
        for k in lv:
            _losses.assert_gradient(levels[l][k].grad, lv[k].grad.cpu().numpy(), f"level {l} {k}")


@pytest.mark.parametrize("kind,name", [("object", "n2048_mask_target"), ("object", "n384_outer_step"), ("ssr", "n1024_c28_target"), ("ssr", "n255_c5_step")])
def test_three_calls_are_bit_identical(kind, name):
    case = _losses.cases(kind)[name]
    runs = []
    for _ in range(3):
        shared, levels = _losses.tensors(case, DEV)
        total, terms = _fused(kind, shared, levels, _weights(case))
        total.backward()
        runs.append([total.detach().clone()] + [terms[t].detach().clone() for t in terms] + [v.grad.clone() for lv in levels for v in lv.values()])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b) or (torch.isnan(a).all() and torch.isnan(b).all())


ALLOWED = ("aten.empty", "aten.empty_like", "aten.empty_strided", "aten.new_empty", "aten.ones_like", "aten.zeros", "aten.zeros_like",
           "aten.view", "aten._unsafe_view", "aten.reshape", "aten.select", "aten.slice", "aten.detach", "aten.alias", "aten.as_strided",
           "aten.unbind", "aten.expand", "aten.t", "aten.transpose", "aten.permute", "aten.squeeze", "aten.unsqueeze")
# autograd's own copy of a gradient into a LEAF's .grad when it cannot take the tensor over (an artefact of testing on leaves: in a
# training step these gradients go on into the compositing backward); a copy, neither arithmetic nor a reduction
LEAF_COPIES = ("aten.clone",)


@pytest.mark.parametrize("kind,name", [("object", "n512_step"), ("ssr", "n255_c5_step")])
def test_fused_loss_dispatches_no_aten_arithmetic(kind, name):
    """Forward + backward of the fused step loss under a TorchDispatchMode (as conftest.aten_gemm_watch): allocation and view ops
    only - every number comes out of the two HIP launches."""
    from torch.utils._python_dispatch import TorchDispatchMode
    case = _losses.cases(kind)[name]
    shared, levels = _losses.tensors(case, DEV)
    weights = _weights(case)
    _fused(kind, shared, levels, weights)                       # the weights' device copy is made once, outside

    class Watch(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops.append(str(func))
            return func(*args, **(kwargs or {}))

    with Watch() as w:
        total, terms = _fused(kind, shared, levels, weights)
        total.backward()
    other = [op for op in w.ops if not any(op == a or op.startswith(a + ".") for a in ALLOWED + LEAF_COPIES)]
    print(sorted(set(w.ops)))
    assert not other, other
    assert levels[0]["albedo"].grad is not None and float(levels[0]["albedo"].grad.abs().sum()) > 0


def test_empty_and_tiny_batches():
    from intrinsicnerf_amd import losses, object_level as ol
    dev = torch.device(DEV)
    # no ray at all: every mean is empty (NaN, as torch.mean of an empty tensor), nothing to differentiate
    e3, e1 = torch.zeros(0, 3, device=dev, requires_grad=True), torch.zeros(0, device=dev, requires_grad=True)
    six = ol.compute_intrinsic_loss(e3, e1, e3, torch.zeros(0, 3, device=dev), None, None, torch.zeros(0, device=dev))
    assert all(torch.isnan(t) for t in six)
    sum(six).backward()
    assert e3.grad is not None and e3.grad.shape == (0, 3)
    # N < 4: the far term is a mean over nothing; N = 1: so are the pair terms.  Checked against the float64 restatement
    g = torch.Generator().manual_seed(3)
    for n in (1, 2, 3, 4, 5):
        a, s, r, t = (torch.rand(n, 3, generator=g), torch.rand(n, generator=g), torch.rand(n, 3, generator=g) - 0.5, torch.rand(n, 3, generator=g) + 0.1)
        for mask in (torch.ones(n), torch.rand(n, 1, generator=g)):
            want = _losses.level_terms(a.double(), s.double(), r.double(), t.double(), mask.double())[:6]
            got = torch.stack(ol.compute_intrinsic_loss(a.to(dev), s.to(dev), r.to(dev), t.to(dev), None, None, mask.to(dev))).cpu()
            assert torch.isnan(want[4]) == (n < 4) and torch.isnan(want[2]) == (n < 2)
            _losses.assert_terms(got.numpy(), want.numpy(), f"N = {n}, mask {tuple(mask.shape)}")
    # every label void: NaN cross-entropy, zero logits gradient (the fixture n1024_c28_all_void holds the values)
    case = _losses.cases("ssr")["n1024_c28_all_void"]
    shared, levels = _losses.tensors(case, DEV)
    total, terms = _fused("ssr", shared, levels, _weights(case))
    assert torch.isnan(terms["semantic"]).all() and torch.isnan(total)
    total.backward()
    assert float(levels[0]["logits"].grad.abs().max()) == 0.0 and torch.isfinite(levels[0]["albedo"].grad).all()
    with pytest.raises(ValueError):
        losses.compute_intrinsic_loss(levels[0]["albedo"], levels[0]["shading"][:, None], levels[0]["residual"], shared["gt"], None, None, shared["key"])


# ---- through the render: graphs and the staged training path ----
def _object_setup(dev):
    from _cases import case_weights
    from intrinsicnerf_amd import object_level as ol
    fx = load_golden("object_chair_det")
    embed, ch = ol.get_embedder(10, 0); embed_d, ch_d = ol.get_embedder(4, 0)
    mk = lambda: ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
    net_c, net_f = mk(), mk()
    sd_c, sd_f = case_weights(fx)
    net_c.load_state_dict(sd_c); net_f.load_state_dict(sd_f)
    return ol, net_c, net_f, ol.NetworkQuery(embed, embed_d), torch.from_numpy(fx["rays"]).to(dev)


OBJECT_WEIGHTS = {"image": 1.0, "chroma": 1.0, "sparsity": 0.01, "far": 0.01, "shading": 1.0, "residual": 1.0, "intensity": 0.1, "cluster": 0.5}


def test_graphed_step_with_the_fused_loss_equals_the_eager_step(monkeypatch):
    """A GraphedTrainStep whose loss_fn renders a small batch with ol.render and applies the fused loss: replay = the eager step,
    losses and parameters bit for bit, as tests/test_graphs_gpu.py requires of any deterministic step (perturb = 0)."""
    from intrinsicnerf_amd import graphs
    monkeypatch.setenv("INERF_PRECISION", "f16x3")
    dev = torch.device(DEV)
    results = {}
    for mode in ("eager", "graph"):
        ol, net_c, net_f, query, rays = _object_setup(dev)
        n = 12
        batches = [rays[i:i + n] for i in (0, 7, 3)]
        gen = torch.Generator().manual_seed(11)
        targets = [torch.rand(n, 3, generator=gen).to(dev) for _ in batches]
        masks = [(torch.rand(n, 1, generator=gen) > 0.3).float().to(dev) for _ in batches]
        clusters = [torch.rand(n, 3, generator=gen).to(dev) for _ in batches]
        opt = torch.optim.Adam(list(net_c.parameters()) + list(net_f.parameters()), lr=1e-4, capturable=True)

        def loss_fn(r, t, m, c):
            out = ol.render(1, n, None, chunk=1024 * 32, rays=(r[:, 0:3], r[:, 3:6]), ndc=False, near=2., far=6., use_viewdirs=True,
                            network_fn=net_c, network_query_fn=query, N_samples=64, retraw=True, perturb=0.0, N_importance=64, network_fine=net_f,
                            white_bkgd=True)
            return ol.object_step_loss(out, t, m, OBJECT_WEIGHTS, c)[0]

        losses = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if mode == "graph":
                step = graphs.GraphedTrainStep(loss_fn, (batches[0], targets[0], masks[0], clusters[0]), opt)
            for group in opt.param_groups:
                if mode == "eager":
                    group["lr"] = torch.tensor(1e-4, dtype=torch.float32, device=dev)
            for r, t, m, c in zip(batches, targets, masks, clusters):
                if mode == "eager":
                    opt.zero_grad(set_to_none=True)
                    loss = loss_fn(r, t, m, c)
                    loss.backward()
                    opt.step()
                else:
                    loss = step(r, t, m, c)
                losses.append(float(loss))
        if mode == "graph":
            assert step.fallbacks == 0
        results[mode] = (losses, [p.detach().clone() for p in list(net_c.parameters()) + list(net_f.parameters())])
    assert np.isfinite(results["graph"][0]).all()
    assert results["eager"][0] == results["graph"][0], (results["eager"][0], results["graph"][0])
    for a, b in zip(results["eager"][1], results["graph"][1]):
        assert torch.equal(a, b)


def _compare_parameter_gradients(params, run_hip, run_torch):
    """Per tensor, the bound of tests/test_backward_golden.py:176-179: norm to 1e-4, projection onto a random direction to 1e-4 of
    norm * sqrt(numel)."""
    grads = {}
    for tag, run in (("hip", run_hip), ("torch", run_torch)):
        for p in params:
            p.grad = None
        run().backward(retain_graph=True)
        grads[tag] = [p.grad.detach().double().clone() for p in params]
    gen = torch.Generator().manual_seed(0)
    for i, (a, b) in enumerate(zip(grads["hip"], grads["torch"])):
        norm = float(b.norm())
        assert norm > 0, i
        d = torch.randn(b.shape, generator=gen, dtype=torch.float64).to(b.device)
        print(f"parameter {i}: norm {norm:.4e}, |norm diff| {abs(float(a.norm()) - norm):.2e}, |projection diff| {abs(float(((a - b) * d).sum())):.2e}")
        assert abs(float(a.norm()) - norm) <= 1e-4 * norm, i
        assert abs(float(((a - b) * d).sum())) <= 1e-4 * norm * np.sqrt(b.numel()), i


def _torch_total(levels, shared, weights):
    terms = [_losses.level_terms(lv["albedo"], lv["shading"], lv["residual"], shared["gt"], shared["key"], lv["rgb"], shared["target"], lv.get("logits"))
             for lv in levels]
    return _losses.total_of(terms, [weights.get(t, 1.0) for t in _losses.TERMS], shared, levels)


def test_object_training_step_parameter_gradients(monkeypatch):
    monkeypatch.setenv("INERF_PRECISION", "f16x3")
    dev = torch.device(DEV)
    ol, net_c, net_f, query, rays = _object_setup(dev)
    n = rays.shape[0] - rays.shape[0] % 2
    gen = torch.Generator().manual_seed(5)
    shared = {"gt": torch.rand(n, 3, generator=gen).to(dev) * 0.8 + 0.1, "key": (torch.rand(n, 1, generator=gen) > 0.2).float().to(dev),
              "target": torch.rand(n, 3, generator=gen).to(dev)}
    shared["gt"][n // 2:] = (shared["gt"][:n // 2] + 0.02).clamp(0, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ret = ol.render_rays(rays[:n], net_c, query, 64, retraw=True, perturb=1.0, N_importance=128, network_fine=net_f, white_bkgd=True,
                             raw_noise_std=0.0)
    levels = [{"albedo": ret["albedo0"], "shading": ret["shading0"], "residual": ret["residual0"], "rgb": ret["rgb0"]},
              {"albedo": ret["albedo_map"], "shading": ret["shading_map"], "residual": ret["residual_map"], "rgb": ret["rgb_map"]}]
    _compare_parameter_gradients(list(net_c.parameters()) + list(net_f.parameters()),
                                 lambda: ol.object_step_loss(ret, shared["gt"], shared["key"], OBJECT_WEIGHTS, shared["target"])[0],
                                 lambda: _torch_total(levels, shared, OBJECT_WEIGHTS))


def test_ssr_training_step_parameter_gradients(monkeypatch):
    monkeypatch.setenv("INERF_PRECISION", "f16x3")
    from intrinsicnerf_amd import ssr
    dev = torch.device(DEV)
    torch.manual_seed(0)
    n, classes = 256, 28
    r = ssr.SSRRenderer(classes, white_bkgd=False, endpoint_feat=False, device=dev)
    r.training, r.check_numerics = True, False
    gen = torch.Generator().manual_seed(9)
    o = torch.tensor([[0.5, 0.2, 0.1]]).expand(n, 3)
    d = torch.randn(n, 3, generator=gen); d = d / d.norm(dim=-1, keepdim=True)
    rays = torch.cat([o, d, 0.1 * torch.ones(n, 1), 10 * torch.ones(n, 1), d], -1).to(dev)
    labels = torch.randint(0, classes + 1, (n,), generator=gen)
    labels[n // 2:] = torch.where(torch.rand(n // 2, generator=gen) < 0.5, labels[:n // 2], labels[n // 2:])
    shared = {"gt": torch.rand(n, 3, generator=gen).to(dev) * 0.8 + 0.1, "key": labels.to(dev), "target": None}
    shared["gt"][n // 2:] = (shared["gt"][:n // 2] + 0.02).clamp(0, 1)
    weights = {"image": 1.0, "semantic": 0.04, "chroma": 1.0, "residual": 1.0, "sparsity": 0.01, "shading": 1.0, "far": 0.01, "intensity": 0.1}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ret = r.render_rays(rays)
    levels = [{"albedo": ret["albedo" + t], "shading": ret["shading" + t], "residual": ret["residual" + t], "rgb": ret["rgb" + t],
               "logits": ret["sem_logits" + t]} for t in ("_coarse", "_fine")]
    _compare_parameter_gradients(list(r.ssr_net_coarse.parameters()) + list(r.ssr_net_fine.parameters()),
                                 lambda: ssr.ssr_step_loss(ret, shared["gt"], shared["key"], weights)[0],
                                 lambda: _torch_total(levels, shared, weights))
