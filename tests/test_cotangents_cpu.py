"""The cotangent builders of tests/_cotangents.py are what they claim to be (no GPU): the groups partition the points and sit in
every tile, the denormal groups are denormal and non-zero in fp32, and an opaque ray's compositing gradient runs through the
denormal window into exact zeros."""
import pytest
import torch

import _cotangents as ct
import oracle


@pytest.mark.parametrize("n_points", [185, 64, 1024 * 192])
def test_groups_partition_the_points_and_fill_every_tile(n_points):
    groups = ct.group_index(n_points)
    assert groups.shape == (n_points,) and int(groups.min()) == 0 and int(groups.max()) == ct.GROUPS - 1
    masks = [groups == g for g in range(ct.GROUPS)]
    assert int(sum(m.long() for m in masks).min()) == 1 and int(sum(m.long() for m in masks).max()) == 1      # a partition
    assert ct.tiles_hold_every_group(groups)
    # a masked point belongs to no group; a tile that loses a whole group to the mask is reported
    live = torch.ones(n_points, dtype=torch.bool)
    live[5] = False
    assert int(ct.group_index(n_points, live)[5]) == -1 and ct.tiles_hold_every_group(ct.group_index(n_points, live))
    live[torch.arange(n_points) % ct.GROUPS == 3] = False
    assert not ct.tiles_hold_every_group(ct.group_index(n_points, live))
    assert len(ct.GROUP_NAMES) == len(ct.GROUP_LOG2) == ct.GROUPS
    assert sorted(ct.DENORMAL_GROUPS + (ct.ZERO_GROUP,) + ct.ACCURATE_GROUPS) == list(range(ct.GROUPS))


@pytest.mark.parametrize("channels", [11, 39, 144])
def test_grouped_cotangent_has_the_magnitudes_it_names(channels):
    n = 185
    c0 = ct.base_cotangent(n, channels, seed=3)
    groups = ct.group_index(n)
    cot = ct.grouped_cotangent(c0, groups)
    assert cot.dtype == torch.float32 and cot.shape == (n, channels)
    for g in ct.DENORMAL_GROUPS:
        part = cot[groups == g]
        assert float(part.abs().max()) < ct.F32_MIN_NORMAL, ct.GROUP_NAMES[g]
        assert bool(ct.is_denormal(part).any(1).all()), "every point of a denormal group has a non-zero entry"
        assert float(ct.is_denormal(part).float().mean()) > 0.98          # (|randn| < 2^-10 rounds to 0 at 2^-140: 0.1 %)
        # each point's largest entry is denormal too
        assert bool((part.abs().amax(1) > 0).all())
    edge = cot[groups == 1].abs().amax(1)
    assert float((edge < 2.0 ** -128).float().mean()) > 0.9, "most points of the 2^-130 group lie below the 2^-128 edge"
    for g in (2, 3, 4, 5):
        part = cot[groups == g]
        normal = ~ct.is_denormal(part)             # (at 2^-120 an entry with |randn| < 2^-6 is denormal: about 1 %)
        assert bool((part != 0).all()) and float(normal.float().mean()) > (0.97 if g == 2 else 0.9999)
        assert bool(normal.any(1).all())
        exact = c0[groups == g].float().double() * 2.0 ** ct.GROUP_LOG2[g]
        assert torch.equal(part.double()[normal], exact[normal]), "a power-of-two scaling is exact"
    assert float(cot[groups == ct.ZERO_GROUP].abs().max()) == 0.0
    sig = cot[groups == ct.SIGMA_GROUP]
    assert bool((sig[:, ct.SIGMA_CHANNEL] != 0).all())
    sig[:, ct.SIGMA_CHANNEL] = 0
    assert float(sig.abs().max()) == 0.0
    for g in range(ct.GROUPS):                      # the isolated runs: one group's rows, bit for bit, and nothing else
        alone = ct.grouped_cotangent(c0, groups, only=g)
        assert torch.equal(alone[groups == g], cot[groups == g]) and float(alone[groups != g].abs().max()) == 0.0
    # the parts add up to the whole (disjoint rows)
    assert torch.equal(sum(ct.grouped_cotangent(c0, groups, only=g) for g in range(ct.GROUPS)), cot)


def test_sweep_scalings_are_exact_and_the_precondition_sees_underflow():
    c0 = ct.base_cotangent(64, 11, seed=1)
    for k in ct.SWEEP_LOG2:
        c = ct.scaled(c0, k)
        normal = ~ct.is_denormal(c)                # (at 2^-120 an entry with |randn| < 2^-6 is denormal: about 1 %)
        assert bool(torch.isfinite(c).all()) and bool((c != 0).all()) and float(normal.float().mean()) > (0.97 if k == -120 else 0.9999)
        assert torch.equal((c.double() * 2.0 ** -k)[normal], c0.float().double()[normal]), k         # only the exponent changed
    want = {"w": torch.tensor([1.0, 3.0, 1e-3], dtype=torch.float64)}
    assert ct.scaling_stays_normal(want, 100) and ct.scaling_stays_normal(want, -110)
    assert not ct.scaling_stays_normal(want, 127)            # 3 * 2^127 overflows
    assert not ct.scaling_stays_normal(want, -120)           # 1e-3 * 2^-120 is denormal and 3e-4 of the norm
    assert not ct.scaling_stays_normal(want, -140)           # everything denormal
    assert ct.scaling_stays_normal({"w": torch.tensor([1.0, 1e-9], dtype=torch.float64)}, -125)       # a denormal element of 1e-9 of the norm


def test_head_gradient_max_follows_the_formula():
    g = torch.Generator().manual_seed(2)
    raw = torch.rand(50, 16, generator=g, dtype=torch.float64)
    d_raw = torch.randn(50, 16, generator=g, dtype=torch.float64)
    raw_l = raw.clone().requires_grad_(True)             # autograd through the heads' own definition
    pre = torch.logit(raw_l[:, 4:11])                    # pre-activations of albedo 3, shading 1, residual 3
    pre = pre.detach().requires_grad_(True)
    act = torch.sigmoid(pre)
    rgb = act[:, 0:3] * act[:, 3:4] + act[:, 4:7]
    loss = (rgb * d_raw[:, 0:3]).sum() + (act * d_raw[:, 4:11]).sum()
    (d_pre,) = torch.autograd.grad(loss, pre)
    want = torch.cat([d_pre, d_raw[:, 3:4], d_raw[:, 11:16]], 1).abs().amax(1)
    got = ct.head_gradient_max(raw, d_raw, n_classes=5)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.max())
    only_sigma = torch.zeros_like(d_raw)
    only_sigma[:, 3] = d_raw[:, 3]
    assert torch.equal(ct.head_gradient_max(raw, only_sigma, n_classes=5), d_raw[:, 3].abs())


def test_opaque_rays_give_denormal_and_zero_compositing_gradients():
    """sigma * delta = 1 from sample 20 on: d loss / d raw of an MSE over 1024 rays, from the fp64 compositing, holds at least
    1 % entries of fp32-denormal size and at least 10 % exact or underflowed zeros."""
    g = torch.Generator().manual_seed(4)
    n, s = 1024, 192
    d = torch.randn(n, 3, generator=g)
    z = torch.sort(torch.rand(n, s, generator=g) * 3 + 0.5, -1)[0]
    raw = torch.rand(n, s, 11, generator=g)
    raw[..., 3] = ct.opaque_sigma(z, d)
    assert float(raw[:, :20, 3].abs().max()) == 0.0
    step = raw[:, 20:-1, 3] * (z[:, 21:] - z[:, 20:-1]) * d.norm(dim=-1, keepdim=True)
    assert float(step.max()) < 1.01 and float((step > 0.99).float().mean()) > 0.999      # (two samples closer than 1e-6 step less)
    raw64 = raw.double().requires_grad_(True)
    out = oracle.composite(raw64, z.double(), d.double(), oracle.RenderConfig(variant="object"))
    target = torch.rand(n, 3, generator=g, dtype=torch.float64)
    ((out["rgb"] - target) ** 2).mean().backward()
    denormal, zero = ct.magnitude_classes(raw64.grad)
    assert denormal >= 0.01 and zero >= 0.10, (denormal, zero)
    assert ct.magnitude_classes(torch.tensor([0.0, 1e-50, 1e-40, 1.0, 2.0 ** -126, 2.0 ** -149])) == (2 / 6, 2 / 6)
