"""CPU: the reference of the training forward's activation slots (tests/_forward_slots.py) - that its slots are the module's own
intermediate values where csrc/layout.h SaveSlot says, and that its decoder of a fragment slot's planes is kernels.frag_decode's."""
import pytest
import torch

import _forward_slots as fs
import oracle
from intrinsicnerf_amd import kernels
from intrinsicnerf_amd.object_level import Embedder


@pytest.mark.parametrize("variant,classes,endpoint", [("object", 0, False), ("ssr", 5, True)])
def test_reference_slots_are_the_modules_own_intermediates(variant, classes, endpoint):
    ssr = variant == "ssr"
    xyz_div = 10.0 if ssr else 1.0
    net = fs.make_module(variant, classes, oracle.make_state_dict(variant, classes, seed=1))
    rays, z = fs.rays_and_depths(10, 5, seed=4, origin_scale=3.0 if ssr else 1.0)           # 50 points
    # the module's input by the package's own encoder, on the positions in two fp32 roundings
    x = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    v = rays[:, None, 8:11].expand(10, 5, 3).reshape(-1, 3)
    call = (lambda m, e: m(e, True)) if endpoint else (lambda m, e: m(e))
    s64 = fs.reference_slots(net, rays, z, xyz_div, endpoint)
    s32 = fs.reference_slots(net, rays, z, xyz_div, endpoint, dtype=torch.float32)
    with torch.no_grad():
        x_div = x / torch.full_like(x, xyz_div) if ssr else x                               # the division stays an fp32 one
        emb64 = torch.cat([Embedder(10)(x_div.double()), Embedder(4)(v.double())], -1)
        emb32 = torch.cat([Embedder(10, scalar_factor=xyz_div)(x), Embedder(4)(v)], -1)
        want64 = call(net.double(), emb64)
        want32 = call(net.float(), emb32)
    assert s64["raw"].dtype == torch.float64 and s32["raw"].dtype == torch.float32
    assert torch.equal(s64["emb"], emb64) and torch.equal(s32["emb"], emb32)
    assert torch.equal(s32["raw"], want32), "the fp32 run is not the module's fp32 forward bit for bit"
    assert torch.equal(s64["raw"], want64)
    assert want64.shape == (50, 11 + classes + (128 if endpoint else 0))
    for s, dtype in ((s64, torch.float64), (s32, torch.float32)):
        widths = {slot: s[slot].shape[1] for slot in fs.ACTIVATION_SLOTS}
        assert widths == {0: 64, 1: 32, **{2 + i: 256 for i in range(8)}, 10: 256, 11: 256, 12: 128, 13: 128 if classes else 0}
        assert all(s[slot].dtype == dtype and s[slot].shape[0] == 50 for slot in fs.ACTIVATION_SLOTS)
        # columns 63 / 27 onwards are the zero padding; every post-ReLU slot is non-negative and alive, feat is signed
        assert float(s[0][:, 63:].abs().max()) == 0.0 and float(s[1][:, 27:].abs().max()) == 0.0
        for slot in fs.ACTIVATION_SLOTS:
            if slot > 1 and slot != kernels.SAVE_FEAT and s[slot].shape[1]:
                assert float(s[slot].min()) == 0.0 and float(s[slot].max()) > 0.0
        assert float(s[kernels.SAVE_FEAT].min()) < 0.0
        # from the last slots through the heads: the module's output exactly ...
        assert torch.equal(fs.heads_from_slots(net, s, endpoint), s["raw"])
        # ... and every slot from the slots before it
        for slot, value in fs.chain_from_slots(net, s).items():
            assert torch.equal(value, s[slot]), fs.SLOT_NAMES[slot]
    # the yardstick is a small number, not zero and not an error of the mapping
    for slot in fs.ACTIVATION_SLOTS:
        if s64[slot].shape[1]:
            d = float((s32[slot].double() - s64[slot]).abs().max())
            assert 0.0 < d <= 1e-5 * max(1.0, float(s64[slot].abs().max())), (fs.SLOT_NAMES[slot], d)


def test_positions_are_two_roundings_and_a_true_division():
    # 3 * fl32(1/3) = 1 + 3e-8 rounds to 1: with the product rounded first, -1 + 3 * fl32(1/3) is 0; a fused multiply-add keeps 3e-8
    rays = torch.zeros(2, 11)
    rays[:, 0], rays[:, 3] = -1.0, 3.0
    third = torch.tensor(1.0) / torch.tensor(3.0)
    x = fs.positions(rays, torch.stack([third, third])[:, None], 1.0)
    assert x.dtype == torch.float32 and x.shape == (2, 3)
    assert float(x[0, 0]) == 0.0 and float(torch.tensor(3.0, dtype=torch.float64) * third.double() - 1.0) > 0.0
    # the division by xyz_div is a division: x * fl32(0.1) differs from it at many fp32 x
    rays = torch.zeros(500, 11)
    rays[:, 0:3] = torch.rand(500, 3, generator=torch.Generator().manual_seed(0)) * 12 - 6
    o = rays[:, 0:3].clone()
    x10 = fs.positions(rays, torch.ones(500, 1), 10.0)
    exact = (o.double() / 10.0).float()                                    # the correctly rounded quotient
    assert torch.equal(x10, exact)
    assert int((o * torch.tensor(0.1) != exact).sum()) > 100


@pytest.mark.parametrize("width", [256, 128, 64, 32])
def test_plane_decoder_is_the_fragment_decoder(width):
    g = torch.Generator().manual_seed(width)
    x = torch.randn(100, width, generator=g) * torch.logspace(-3, 1, width)[None, :]
    frag = kernels.frag_encode(x)                                                           # float16 halves, whole tiles
    planes = fs.frag_planes(frag.view(torch.int32), width)
    assert planes.shape == (2, 128, width) and planes.dtype == torch.float16
    assert torch.equal(fs.planes_value(planes)[:100].float(), kernels.frag_decode(frag, 100, width=width))
    assert float(planes[:, 100:].abs().max()) == 0.0
    assert float(planes[1].abs().max()) > 0.0 and bool((planes[1].abs().float() <= planes[0].abs().float() * 2.0 ** -10 + 2.0 ** -24).all())
    sentinel = torch.full((64 * width,), fs.SENTINEL, dtype=torch.int32)
    assert bool((fs.halves_bits(fs.frag_planes(sentinel, width)) == fs.SENTINEL_HALF).all())
    assert bool(torch.isnan(sentinel.view(torch.float32)).all())


def test_sweep_arguments_hold_what_the_sweep_is_about():
    pos, dirs = fs.sweep_arguments(False), fs.sweep_arguments(True)
    assert pos.dtype == torch.float32 and pos.numel() <= 4099 and dirs.numel() <= 4099
    assert float(pos.abs().max()) == 1000.0 and float(dirs.abs().max()) == 5000.0
    import math
    import numpy as np
    for f in range(10):                                        # the fp32 nearest to the quadrant edges, and the value beside it
        for m in (1, -3, 7, 100, 1001, -20860):
            edge = np.float32(m * math.pi / 4 / 2 ** f)
            for args, limit in ((pos, 64.0), (dirs, 4096.0)):
                if abs(float(edge)) < limit / 2:
                    assert bool((args == float(edge)).any()) and bool((args == float(np.nextafter(edge, np.float32(0)))).any())
    for v in (64.0, -64.0, 2.0 ** -126, 1e-40):
        assert bool((pos == torch.tensor(v, dtype=torch.float32)).any())
    assert bool((dirs == 4096.0).any()) and bool((dirs == -4096.0).any()) and not bool((pos == 4096.0).any())
    assert bool(((pos == 0) & torch.signbit(pos)).any()) and bool(((pos == 0) & ~torch.signbit(pos)).any())
    rays, z = fs.sweep_rays(4099)
    moved = torch.zeros(4099, dtype=torch.bool)
    moved[fs.moved_rows(4099)] = True
    assert rays.shape == (4099, 11) and float(rays[~moved, 3:6].abs().max()) == 0.0 and bool((z[~moved] == 1).all())
    # the moved rows: the last whole tile, before the ragged one, every d and z non-trivial, and a fused multiply-add would land on another
    # fp32 position in many of them - by an ulp, which band 9 turns into 512 ulp of the argument
    assert int(moved.sum()) == 64 and fs.moved_rows(4099) == slice(4032, 4096)
    assert float(rays[moved, 3:6].abs().min()) > 0.0 and float(z[moved].min()) >= 2.0
    two, one = fs.positions(rays, z, 1.0), fs.fused_positions(rays, z)
    assert torch.equal(two[~moved], one[~moved])
    differ = (two != one)[moved]
    assert int(differ.sum()) >= 30, int(differ.sum())
    shift = ((two.double() - one.double()).abs() * 512)[moved]
    assert int((shift > 1e-5).sum()) >= 10, int((shift > 1e-5).sum())           # far beyond the sweep's 3.5e-7 in band 9
    for base, args in ((0, pos), (8, dirs)):
        for c in range(3):
            assert set(rays[:, base + c].view(torch.int32).tolist()) == set(args.view(torch.int32).tolist())
        assert not torch.equal(rays[:, base], rays[:, base + 1])
    assert torch.equal(fs.positions(rays, z, 1.0)[~moved], rays[~moved, 0:3])
