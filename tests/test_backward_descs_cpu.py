"""The cases of tests/_descs.py are fair: on every network of the table the module's own fp32 autograd (the reference's arithmetic,
on the CPU) passes the judge the HIP backward is held to - fp64 autograd, 2e-4 of the norm of every parameter tensor and of every
slice, no absolute term, no reference gradient identically zero, ReLU ties below 1 % of the points.  The worst ratio per case is
printed: the bound's margin over the reference's own arithmetic is what these lines show, not an assumption.

And, through the C ABI without a GPU: inerf_param_floats and the tensor table agree with the module and with
oracle.state_dict_spec for every description of the table."""
import pytest
import torch

import _descs
import oracle

TAG = "backward_descs | cpu"


@pytest.mark.parametrize("net", _descs.NETS, ids=_descs.net_id)
def test_fp32_autograd_passes_the_judge(net, torch_threads):
    ref = _descs.reference(net)
    assert ref["ties"] < 0.01
    assert tuple(ref["raw"].shape) == (net.n, net.s, _descs.channels(net))
    raw32, got = _descs.autograd(net, _descs.module(net), ref["rays"], ref["z"], ref["cot"], torch.float32)
    bad, tensor, piece = _descs.judge(net, got, TAG, f"{_descs.net_id(net)} fp32 autograd")
    assert not bad, bad
    assert _descs.judge_raw(net, raw32, TAG, _descs.net_id(net)) <= 1.0


def test_the_table_is_the_one_asked_for():
    """5 object descriptions x 3 forms, 12 scene-level networks x 2 forms, the endpoint network, two networks at 65 points."""
    assert len(_descs.CASES) == 15 + 24 + 1 + 2 and len(set(_descs.CASES)) == len(_descs.CASES)
    assert {(n.l_xyz, n.l_dir) for n in _descs.NETS if n.variant == "object"} == {(0, 0), (0, 4), (10, 0), (6, 2), (9, 3)}
    assert {n.classes for n in _descs.NETS if n.variant == "ssr" and (n.l_xyz, n.l_dir) == (10, 4)} == {1, 2, 3, 4, 7, 127, 128, 129, 240}
    assert sum(c.fwd == "t128" for c in _descs.CASES) == 5 and all(c.net.variant == "object" for c in _descs.CASES if c.fwd)
    assert sorted(n.n * n.s for n in _descs.NETS if (n.n, n.s) != _descs.SMALL) == [65, 65]


@pytest.mark.parametrize("variant,classes,l_xyz,l_dir", _descs.DESCRIPTIONS, ids=lambda v: str(v))
def test_parameter_count_and_tensor_table(variant, classes, l_xyz, l_dir):
    from intrinsicnerf_amd import _capi, packing
    desc = _descs.capi_desc(variant, classes, l_xyz, l_dir)
    mod = _descs.module(_descs.Net(variant, classes, False, l_xyz, l_dir, 1, 1))
    assert _capi.lib().inerf_param_floats(desc) == sum(p.numel() for p in mod.parameters())
    table = [(name, (rows, cols) if cols else (rows,)) for name, (rows, cols) in packing.tensor_table(desc)]
    assert table == [(name, tuple(shape)) for name, shape in oracle.state_dict_spec(variant, classes, l_xyz, l_dir)]
    assert table == [(name, tuple(p.shape)) for name, p in mod.named_parameters()]
    got = mod.fused_desc()
    assert got is not None and (got.variant, got.n_classes, got.l_xyz, got.l_dir) == (desc.variant, classes, l_xyz, l_dir)
