"""CPU: the gate probe's cull margin per network (include/inerf.h INERF_FLAG_GATE_PROBE).

The probe culls a point when s < -kappa S.  With a margin state the listed trunk measures r = |s - sigma| / S on every candidate and
a launch uses kappa = max(2^-9, 8 r_max) once the network has been seen on enough points, 2^-6 before.  Here:

- ``inerf_gate_kappa``, the host export of the one statement of that rule, at its corners;
- the rule on the torch restatement of the probe (``_gate_probe.probe_model``) against the fp64 trunk: r is taken over the candidates
  at 2^-6 alone - what a first launch can see - and with kappa = max(2^-9, 8 r) no culled point has positive fp64 density, on the bench
  networks, the trained fixture and both hold-out families.  The reserve kappa / r_all (r over ALL points) is printed."""
import ctypes as C
import math

import pytest
import torch

import _gate_probe as gp

FLOOR = 2.0 ** -9
N_RAYS = 256


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi.lib()


def test_the_rule_at_its_corners(lib):
    n = 1 << 20
    k = lambda r, obs, need=n: float(lib.inerf_gate_kappa(C.c_float(r), obs, need))
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    assert k(1.0e-3, n - 1) == 2.0 ** -6 and k(0.0, 0) == 2.0 ** -6 and k(2.0 ** -4, n - 1) == 2.0 ** -6      # below min_observed
    assert k(0.0, n) == FLOOR and k(0.0, 10 * n) == FLOOR
    assert k(1.0e-3, n) == f32(8.0 * f32(1.0e-3)) and abs(k(1.0e-3, n) - 8.0e-3) < 1e-9
    assert k(2.0 ** -4, n) == 0.5                                            # no upper clamp at 2^-6
    assert k(2.0 ** -13, n) == FLOOR and k(2.0 ** -12, n) == FLOOR and k(2.0 ** -11, n) == 2.0 ** -8
    for bad in (float("nan"), float("inf")):
        assert k(bad, 10 * n) == 2.0 ** -6
    assert k(1.0e-3, 1, 1) == f32(8.0 * f32(1.0e-3)) and k(1.0e-3, 0, 0) == f32(8.0 * f32(1.0e-3))
    assert lib.inerf_gate_min_observed() >= 1024                             # small launches stay on the constant


def _points(name, dset):
    if name.startswith("bench_"):
        sd, rays = gp.network(name)
        rays = rays[:: rays.shape[0] // N_RAYS][:N_RAYS]
        return sd, gp.positions(rays, gp.sample_depths(rays, 64 if name.endswith("coarse") else 192, seed=7))
    sd, _ = gp.network(name)
    return sd, gp.positions(gp.family_rays(name.rsplit("_", 1)[0]), gp.depth_sets(name)[dset])


CASES = [("bench_coarse", "uniform"), ("bench_fine", "uniform")] + [
    (f"{family}_{lvl}", dset) for family in gp.HOLDOUT_FAMILIES for lvl, dset in (("coarse", "uniform"), ("fine", "uniform"), ("fine", "z_fine"))]


@pytest.mark.parametrize("name,dset", CASES)
def test_the_adapted_margin_culls_no_positive_density(name, dset):
    sd, x = _points(name, dset)
    with torch.no_grad():
        sigma = gp.sigma_fp64(sd, x)
        s, big_s = gp.probe_model(sd, x)
    err = (s - sigma).abs() / big_s
    cand = ~(s < -gp.KAPPA * big_s)                 # what the first launch lists, and so measures
    assert bool(cand.any()) and bool(torch.isfinite(err).all())
    r, r_all = float(err[cand].max()), float(err.max())
    kappa = max(FLOOR, 8.0 * r)
    culled = s < -kappa * big_s
    print(f"{name} on {dset} depths: {x.shape[0]} points, sigma > 0 on {float((sigma > 0).double().mean()):.4f}, candidates at 2^-6 {float(cand.double().mean()):.4f}, "
          f"r over them {r:.3e}, r over all points {r_all:.3e}, kappa = {kappa:.3e} = 2^{math.log2(kappa):.2f}, culled {float(culled.double().mean()):.4f}, "
          f"reserve kappa / r_all = {kappa / r_all:.2f}")
    assert int((culled & (sigma > 0)).sum()) == 0
    assert bool(culled.any())
