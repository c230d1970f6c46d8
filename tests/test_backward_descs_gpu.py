"""The network backward (inerf_mlp_backward: csrc/mlp_bwd.hip, csrc/mlp_wgrad.hip, the reduce / scatter kernels and build_table of
csrc/train_api.hip) at the descriptions of tests/_descs.py: reduced encodings, the class edges 1 / 2 / 4 / 127 / 128 / 129 / 240,
the endpoint feature at a reduced encoding - through kernels.mlp_train + backward(), judged by fp64 autograd at 2e-4 of the norm of
every parameter tensor AND of every slice a misplaced scatter would move (tests/_descs.py; test_backward_descs_cpu.py shows that the
reference's own fp32 arithmetic passes the same judge with a margin of 17 or more).

Forms: ``dual`` - the two-workgroup chain and the default training forward; ``single`` - the eight-wave chain
(INERF_DGRAD_KERNEL=single) behind the one-workgroup training forward (INERF_F16_KERNEL=single); ``dual`` + INERF_TRAIN_FWD=t128 -
the 128-point training forward of the object-level network.

Then: descriptions interleaved in ONE process (the per-description caches - cached() in train_api.hip, packing._tables,
packing._device_packers - looked up with several entries present), and the one-call entry's own contract at C = 129, (0, 0).

Worst figures on an MI355X (records, not thresholds; profiles/backward_descs.txt has every line), |got - want|_2 / |want|_2:
  object-level   a tensor 2.01e-5 (pts_linears.0.bias at (0, 4) and (9, 3)), a slice 1.83e-5 (pts_linears.0.weight at (0, 4))
  scene-level    a tensor 6.62e-5 (pts_linears.0.bias, C = 240 at (6, 2)), a slice 5.25e-5 (pts_linears.0.weight, the same case); at (10, 4)
                 5.66e-5 / 4.48e-5 (C = 129); every class row of semantic_linear.1.weight below both
  raw            at most 0.009 of its bound; the reference's own fp32 autograd: a tensor 4.6e-6, a slice 1.1e-5 (test_backward_descs_cpu.py)
  interleaved    the third run of each triple equals the first bit for bit
No fault was found: every description the C ABI accepts gives gradients inside the bound.

Mutation check (one run, not committed): a scratch build whose build_table wrote the skip layer's activation piece of pts_linears.5.weight
at dst_col0 = 63 instead of e.  It FAILED 21 of the 44 tests here - every case with l_xyz < 10 (object (0, 0), (0, 4), (6, 2), (9, 3) in all
three forms, SSR C = 1 at (3, 0), C = 240 at (6, 2), C = 129 at (0, 0), C = 7 + endpoint at (6, 2), object (6, 2) at 65 points) and the
interleaved test - and passed the 23 with l_xyz = 10, where 63 = e.  The same build PASSED every GPU test that existed before this module
(and the forward, repack and weight-gradient cases added beside it): nothing else ran the backward at another description."""
import ctypes as C

import pytest
import torch

import _descs

pytestmark = pytest.mark.gpu

TAG = "backward_descs | gpu"


def _select(monkeypatch, chain, fwd):
    monkeypatch.setenv("INERF_DGRAD_KERNEL", chain)
    if chain == "single":
        monkeypatch.setenv("INERF_F16_KERNEL", "single")
    else:
        monkeypatch.delenv("INERF_F16_KERNEL", raising=False)
    if fwd:
        monkeypatch.setenv("INERF_TRAIN_FWD", fwd)
    else:
        monkeypatch.delenv("INERF_TRAIN_FWD", raising=False)


def _step(net):
    """One training step of ``net`` on its batch through the front-end's node: (raw [n, s, channels], {name: gradient})."""
    from intrinsicnerf_amd import kernels
    dev = torch.device("cuda:0")
    ref = _descs.reference(net)
    mod = _descs.module(net).to(dev)
    desc = mod.fused_desc()
    assert desc is not None and (desc.l_xyz, desc.l_dir, desc.n_classes) == (net.l_xyz, net.l_dir, net.classes)
    desc.xyz_div = _descs.embedders(net)[0].scalar_factor
    raw = kernels.mlp_train(desc, mod, ref["rays"].to(dev), ref["z"].to(dev), net.endpoint)
    assert type(raw.grad_fn).__name__ == "_FusedMlpFnBackward"
    (raw * ref["cot"].to(dev)).sum().backward()
    assert all(p.grad is not None for p in mod.parameters())
    return raw.detach(), {name: p.grad.detach().clone() for name, p in mod.named_parameters()}


@pytest.mark.parametrize("case", _descs.CASES, ids=_descs.case_id)
def test_network_backward_at_the_description(case, monkeypatch):
    _select(monkeypatch, case.chain, case.fwd)
    raw, got = _step(case.net)
    what = _descs.case_id(case)
    raw_worst = _descs.judge_raw(case.net, raw, TAG, what)
    bad, _, _ = _descs.judge(case.net, got, TAG, what)
    assert not bad, bad
    assert raw_worst <= 1.0, raw_worst


def test_descriptions_interleaved_in_one_process(monkeypatch):
    """(10, 4) -> (6, 2) -> (10, 4) of the object-level network, then C = 28 -> C = 129 -> C = 28 of the scene-level one, default
    forms: every run passes the judge, and the third of each triple equals the first bit for bit, raw and every gradient."""
    _select(monkeypatch, "dual", None)
    obj = [_descs.Net("object", 0, False, lx, ld, *_descs.SMALL) for lx, ld in ((10, 4), (6, 2), (10, 4))]
    ssr = [_descs.Net("ssr", c, False, 10, 4, *_descs.SMALL) for c in (28, 129, 28)]
    bad = {}
    for triple in (obj, ssr):
        runs = []
        for i, net in enumerate(triple):
            raw, got = _step(net)
            what = f"interleaved run {i} {_descs.net_id(net)}"
            if _descs.judge_raw(net, raw, TAG, what) > 1.0:
                bad[(what, "raw")] = "over its bound"
            for name, why in _descs.judge(net, got, TAG, what)[0].items():
                bad[(what, name)] = why
            runs.append((raw, got))
        (raw_a, got_a), _, (raw_c, got_c) = runs
        if not torch.equal(raw_a, raw_c):
            bad[(_descs.net_id(triple[0]), "raw")] = "the third run differs from the first"
        for name in got_a:
            if not torch.equal(got_a[name], got_c[name]):
                bad[(_descs.net_id(triple[0]), name)] = f"the third run differs from the first in {int((got_a[name] != got_c[name]).sum())} elements"
    assert not bad, bad


def test_one_call_contract_at_129_classes_without_encoding():
    """C = 129 at (0, 0), as test_one_call_backward_equals_library_products_of_its_own_buffers does at (10, 4): a workspace one byte short
    is refused with E_WORKSPACE; the empty batch zeroes all inerf_param_floats words."""
    from intrinsicnerf_amd import _capi
    dev = torch.device("cuda:0")
    lib = _capi.lib()
    net = _descs.Net("ssr", 129, False, 0, 0, *_descs.SMALL)
    desc = _descs.capi_desc(net.variant, net.classes, net.l_xyz, net.l_dir)
    n_params = lib.inerf_param_floats(desc)
    assert n_params == sum(p.numel() for p in _descs.module(net).parameters())
    grads = torch.full((n_params + 16,), 7.0, device=dev)
    assert lib.inerf_mlp_backward(desc, None, None, None, None, None, 0, 0, C.c_void_p(grads.data_ptr()), None, 0, None, None) == _capi.OK
    torch.cuda.synchronize()
    assert float(grads[:n_params].abs().max()) == 0.0
    assert bool((grads[n_params:] == 7.0).all()), "the empty batch wrote past the gradient blob"
    p = net.n * net.s
    need = lib.inerf_mlp_backward_workspace_bytes(desc, p)
    assert need > 0
    one = torch.zeros(1, device=dev)
    ptr = C.c_void_p(one.data_ptr())
    rc = lib.inerf_mlp_backward(desc, ptr, ptr, ptr, ptr, ptr, p, 0, C.c_void_p(grads.data_ptr()), ptr, need - 1, None, None)
    assert rc == _capi.E_WORKSPACE
