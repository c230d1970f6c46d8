"""The cases of tests/_range_guard.py are fair - on the CPU alone, for every (variant, site): only the site passes the guard's limit, every
other split value of the fp64 reference is at most 1/8 of it, no point lies within 1 % of it, the expected words are neither none nor
all, for the head sites of the object-level network the words of live points are a proper, non-empty subset, with gain 1 nothing is
beyond the limit (the site alone makes the case), the fp32 reference puts every point on the side fp64 puts it, the rows are finite -
and the site's fp64 value is gain * relu(u) of the ramp, which is what the persistent-loop cases compute their words from."""
import pytest
import torch

import _range_guard as rg

VARIANTS = [("object", 0, False), ("ssr", 5, False), ("ssr", 33, False), ("ssr", 5, True)]
SHAPE = (24, 32, 4)              # rays, samples, rays per status word: the GPU tests' 768 points in 6 words of 128
CASES = [pytest.param(v, c, e, site, id=f"{v}{c or ''}{'-endpoint' if e else ''}-{site}") for v, c, e in VARIANTS for site in rg.sites(v, c)]


@pytest.mark.parametrize("variant,classes,endpoint,site", CASES)
def test_the_case_is_fair(variant, classes, endpoint, site):
    c = rg.case(variant, classes, endpoint, *SHAPE, site)
    value, beyond = c.site_value(), c.beyond()
    others = c.other_split_max()
    e_all = c.e_all()
    print(f"range_guard | {variant}{classes or ''} {site}: gain {c.gain:.6g}, {int(beyond.sum())} points beyond, largest {float(value.abs().max()) / rg.LIMIT:.4f} of the limit, "
          f"every other split value <= {others:.2e} of it, words {e_all.int().tolist()}")
    assert others <= rg.OTHERS
    assert not bool(c.in_band().any())
    assert bool(e_all.any()) and not bool(e_all.all())
    assert e_all.tolist() == rg.words_of(c.offenders[:, None].expand(c.n, c.s), c.n, c.s, c.status_rays).tolist()
    assert torch.equal(c.beyond(c.slots32), beyond)
    assert bool(torch.isfinite(c.raw64).all()) and bool(torch.isfinite(c.raw32).all())
    if site != rg.ENCODING:
        assert c.gain <= 2.0 ** 11 and float(c.u.max()) - float(c.u.min()) >= 4.0
        assert float((value - c.analytic()).abs().max()) <= 1e-12 * rg.LIMIT
        assert float((c.site_value(c.slots32).double() - value).abs().max()) <= 2e-6 * float(value.abs().max())
        # the site alone makes the case; flipped, a ReLU site clips it away and feature_linear keeps |.|
        unit = rg.case(variant, classes, endpoint, *SHAPE, site, "unit")
        assert not bool(unit.e_all().any()) and unit.other_split_max() <= rg.OTHERS and float(unit.site_value().abs().max()) <= 8.0
        flipped = rg.case(variant, classes, endpoint, *SHAPE, site, "flipped")
        if site in rg.RELU_SITES:
            assert float(flipped.site_value().abs().max()) == 0.0 or site == "pts_linears.0"
            assert not bool(flipped.e_all().any()) and float((flipped.site_value() - flipped.analytic()).abs().max()) <= 1e-12 * rg.LIMIT
        else:
            assert flipped.e_all().tolist() == e_all.tolist() and float(flipped.site_value().max()) == 0.0
        assert flipped.other_split_max() <= rg.OTHERS
        under = rg.case(variant, classes, endpoint, *SHAPE, site, "under")
        assert not bool(under.e_all().any()) and abs(float(under.site_value().abs().max()) / rg.LIMIT - 0.99) < 1e-6
        # the wire leaves the rows alone: those of the network with unit J cut and nothing else (the site's own unit has no consumer)
        ch = 11 + classes                                           # (behind them the endpoint: the views hidden layer itself)
        assert float((unit.raw64[:, :ch] - c.raw64[:, :ch]).abs().max()) <= 1e-9 * float(c.raw64[:, :ch].abs().max())
    else:
        near = c.near_rays[:, None].expand(c.n, c.s).reshape(-1)
        assert bool(((value[near].abs() / rg.LIMIT - 0.99).abs() < 1e-6).all()) and not bool(beyond[near].any())
    if variant == "object" and site in rg.HEAD_SITES:
        e_live = c.e_live(c.raw64[:, 3])
        assert bool(e_live.any()) and bool((e_all & ~e_live).any()) and not bool((e_live & ~e_all).any()), (e_live.tolist(), e_all.tolist())


def test_words_of():
    points = torch.zeros(6, 4, dtype=torch.bool)
    points[2, 3] = points[5, 0] = True
    assert rg.words_of(points, 6, 4, 2).tolist() == [False, True, True]
    assert rg.words_of(points.flatten(), 6, 4, 4).tolist() == [True, True]
