"""The network backward at every kind of description the C ABI accepts (csrc/layout.h net_supported): reduced encodings
(l_xyz 0..10, l_dir 0..4), the class edges of the scene-level network (1, 2, 4: the dual chain's four-classes-per-step loop and its
scalar tail; 127 / 128 / 129: the semantic product's 128 -> 256 row switch and its padding; 240: the ABI's limit), with and
without the endpoint feature.  Shared by test_backward_descs_cpu.py (the cases are fair) and test_backward_descs_gpu.py.

Judge, as in test_backward_range_gpu.py: fp64 torch autograd through the module's own forward on the fp32 sample positions
(test_backward_golden._torch_reference_grads), fed the same fp32 cotangent; |got - want|_2 <= 2e-4 |want|_2 with NO absolute term
- per parameter tensor and per SLICE whose misplacement a whole-tensor norm can dilute: each class row of semantic_linear.1.weight,
pts_linears.0.weight, the encoding / activation column blocks of pts_linears.5.weight, the feature / direction column blocks of
views_linears.0.weight (the three scatters of csrc/train_api.hip build_table that depend on e = 3 + 6 l_xyz and dv = 3 + 6 l_dir).
ReLU ties (test_backward_golden._relu_tie_points, from the fp64 network alone) get no cotangent; below 1 % of the points."""
import copy
import functools
from collections import namedtuple

import numpy as np
import torch

import _forward_slots as fs
import oracle
from test_backward_golden import _torch_reference_grads

RTOL = 2e-4                       # test_backward_range_gpu.RTOL: the project's bound on a parameter gradient
RAW_RTOL, RAW_ATOL_OF_MAX = 1e-4, 1e-5          # raw: the bound of test_backward_golden._check_network_backward
SMALL = (37, 5)                   # 185 points: two 64-point tiles and a ragged third
ONE_OVER = (13, 5)                # 65 points: one tile and one point
WEIGHTS = dict(seed=21, sigma_gain_log2=3, freq_decay=True)

# a network on a batch: what the fp64 reference depends on
Net = namedtuple("Net", "variant classes endpoint l_xyz l_dir n s")
# ... and the kernels it is run with: the chain form (INERF_DGRAD_KERNEL) and the training forward (INERF_TRAIN_FWD, None: default)
Case = namedtuple("Case", "net chain fwd")


def net_id(net):
    name = "object" if net.variant == "object" else f"ssr{net.classes}" + ("e" if net.endpoint else "")
    return f"{name}-x{net.l_xyz}d{net.l_dir}-{net.n * net.s}pts"


def case_id(case):
    return f"{net_id(case.net)}-{case.chain}-{case.fwd or 'fwd64'}"


def _table():
    cases = []
    for lx, ld in ((0, 0), (0, 4), (10, 0), (6, 2), (9, 3)):
        net = Net("object", 0, False, lx, ld, *SMALL)
        cases += [Case(net, "dual", None), Case(net, "single", None), Case(net, "dual", "t128")]
    ssr = [Net("ssr", c, False, 10, 4, *SMALL) for c in (1, 2, 3, 4, 7, 127, 128, 129, 240)]
    ssr += [Net("ssr", 1, False, 3, 0, *SMALL), Net("ssr", 240, False, 6, 2, *SMALL), Net("ssr", 129, False, 0, 0, *SMALL)]
    for net in ssr:
        cases += [Case(net, "dual", None), Case(net, "single", None)]
    cases.append(Case(Net("ssr", 7, True, 6, 2, *SMALL), "dual", None))          # the one-workgroup forward it always takes
    cases.append(Case(Net("object", 0, False, 6, 2, *ONE_OVER), "dual", None))
    cases.append(Case(Net("ssr", 129, False, 10, 4, *ONE_OVER), "dual", None))
    return cases


CASES = _table()
NETS = list(dict.fromkeys(c.net for c in CASES))
# every description of the table, with the descriptions of the fixed-order test: (variant, classes, l_xyz, l_dir)
DESCRIPTIONS = list(dict.fromkeys([(n.variant, n.classes, n.l_xyz, n.l_dir) for n in NETS]
                                  + [("object", 0, 10, 4), ("ssr", 28, 10, 4)]))


def channels(net):
    return 11 + net.classes + (128 if net.endpoint else 0)


def embedders(net):
    from intrinsicnerf_amd import object_level as ol, ssr
    if net.variant == "object":
        return ol.get_embedder(net.l_xyz, 0)[0], ol.get_embedder(net.l_dir, 0)[0]
    return ssr.get_embedder(net.l_xyz, 0, scalar_factor=10)[0], ssr.get_embedder(net.l_dir, 0, scalar_factor=1)[0]


def module(net):
    """The package's own torch module with the closed-form weights of the range tests, on the CPU."""
    sd = oracle.lcg_state_dict(net.variant, net.classes, l_xyz=net.l_xyz, l_dir=net.l_dir, **WEIGHTS)
    return fs.make_module(net.variant, net.classes, sd, net.l_xyz, net.l_dir)


def batch(net):
    """(rays [n, 11], depths [n, s], cotangent [n, s, channels]) on the CPU: the recipe of test_backward_golden._check_network_backward
    (cotangent on every channel, four decades of scale over the rays)."""
    n, s = net.n, net.s
    g = torch.Generator().manual_seed(7 + n)
    o = torch.rand(n, 3, generator=g) * 2 - 1
    d = torch.randn(n, 3, generator=g)
    rays = torch.cat([o, d, torch.zeros(n, 2), d / d.norm(dim=-1, keepdim=True)], -1)
    z = torch.sort(torch.rand(n, s, generator=g) * 3 + 0.5, -1)[0]
    cot = torch.randn(n, s, channels(net), generator=g) * torch.logspace(-3, 1, n, base=10.0)[:, None, None]
    return rays, z, cot


def autograd(net, mod, rays, z, cot, dtype, ties_out=None):
    """(raw, {name: gradient}) of ``mod`` through torch autograd on the CPU in ``dtype``, on the fp32 sample positions."""
    m = copy.deepcopy(mod).cpu().to(dtype)
    embed, embed_d = embedders(net)
    raw, grads = _torch_reference_grads(m, embed, embed_d, rays.to(dtype), z.to(dtype), cot.to(dtype), net.endpoint, ties_out=ties_out)
    return raw.detach(), {k: v.detach() for k, v in grads.items()}


@functools.lru_cache(maxsize=None)
def reference(net):
    """{"rays", "z", "cot" (fp32, the ties' rows zeroed), "ties" (share of the points), "raw" and "grads" (fp64)} of one network on
    its batch: computed once, shared by the forms and by the CPU and GPU tests, left alone."""
    mod = module(net)
    rays, z, cot = batch(net)
    ties = []
    autograd(net, mod, rays, z, cot, torch.float64, ties_out=ties)
    live = ~ties[0]
    assert 100 * int((~live).sum()) < net.n * net.s, f"{net_id(net)}: {int((~live).sum())} ReLU ties of {net.n * net.s} points"
    cot = cot * live[:, :, None].to(cot.dtype)
    raw, grads = autograd(net, mod, rays, z, cot, torch.float64)
    return {"rays": rays, "z": z, "cot": cot, "ties": float((~live).float().mean()), "raw": raw, "grads": grads}


def slices(net, grads):
    """{label: tensor} of the slices judged beside the whole tensors."""
    e = 3 + 6 * net.l_xyz
    out = {"pts_linears.0.weight[:, :e]": grads["pts_linears.0.weight"],
           "pts_linears.5.weight[:, :e]": grads["pts_linears.5.weight"][:, :e],
           "pts_linears.5.weight[:, e:]": grads["pts_linears.5.weight"][:, e:],
           "views_linears.0.weight[:, :256]": grads["views_linears.0.weight"][:, :256],
           "views_linears.0.weight[:, 256:]": grads["views_linears.0.weight"][:, 256:]}
    assert out["pts_linears.0.weight[:, :e]"].shape[1] == e and out["pts_linears.5.weight[:, e:]"].shape[1] == 256
    assert out["views_linears.0.weight[:, 256:]"].shape[1] == 3 + 6 * net.l_dir
    for c in range(net.classes):
        out[f"semantic_linear.1.weight[{c}]"] = grads["semantic_linear.1.weight"][c]
    return out


def _ratios(got, want, bad):
    worst = (0.0, "")
    for name, w in want.items():
        w = w.double()
        if name not in got or tuple(got[name].shape) != tuple(w.shape):
            bad[name] = f"shape {tuple(got[name].shape) if name in got else None} vs {tuple(w.shape)}"
            continue
        gt = got[name].detach().double().cpu()
        if not bool(torch.isfinite(gt).all()):
            bad[name] = f"{int((~torch.isfinite(gt)).sum())} non-finite of {gt.numel()}"
            continue
        err, wn = float((gt - w).norm()), float(w.norm())
        if wn == 0.0:
            bad[name] = "the reference gradient is identically zero: the case pins nothing here"
            continue
        if not err <= RTOL * wn:
            bad[name] = f"{err / wn:.2e} of its norm"
        if err / wn > worst[0]:
            worst = (err / wn, name)
    return worst


def judge(net, got, tag, what):
    """{tensor or slice: why} of what is beyond 2e-4 of its reference's norm (non-finite and zero-reference ones included); prints
    one line with the worst tensor and the worst slice."""
    want = reference(net)["grads"]
    bad = {}
    missing = sorted(set(want) ^ set(got))
    if missing:
        bad["names"] = f"differ in {missing}"
    tensor = _ratios(got, want, bad)
    have = {k: v for k, v in got.items() if k in want and tuple(v.shape) == tuple(want[k].shape)}
    piece = _ratios(slices(net, have), slices(net, want), bad) if len(have) == len(want) else (float("nan"), "-")
    print(f"{tag} {what}: worst tensor {tensor[0]:.2e} ({tensor[1]}), worst slice {piece[0]:.2e} ({piece[1]}), ties {reference(net)['ties']:.2%}"
          + (f"  BAD: {bad}" if bad else ""))
    return bad, tensor[0], piece[0]


def judge_raw(net, raw, tag, what):
    """raw [n, s, channels] against the fp64 forward: |got - want| <= 1e-4 |want| + 1e-5 max |want|; prints the worst scaled error."""
    want = reference(net)["raw"].double().numpy()
    got = raw.detach().double().cpu().numpy().reshape(want.shape)
    bound = RAW_RTOL * np.abs(want) + RAW_ATOL_OF_MAX * float(np.abs(want).max())
    ratio = np.abs(got - want) / bound
    worst = float(np.nan_to_num(ratio, nan=np.inf).max())
    print(f"{tag} {what}: raw worst {worst:.3f} of its bound")
    return worst


def capi_desc(variant, classes, l_xyz, l_dir):
    from intrinsicnerf_amd import _capi
    ssr = variant == "ssr"
    return _capi.net_desc(_capi.VARIANT_SSR if ssr else _capi.VARIANT_OBJECT, classes, l_xyz, l_dir, 10.0 if ssr else 1.0, _capi.PREC_F16X3)
