"""CPU: the margin of the density gate's probe (INERF_FLAG_GATE_PROBE) on a torch restatement of its arithmetic.

The probe evaluates the trunk on f16 hi operands alone and culls a point when s < -kappa S, S = sum |w_alpha,k| h7_k + |b_alpha|.
kappa = 2^-6 is the smallest power of two >= 8 x the largest |s - sigma| / S measured on the kernels
(profiles/gate_probe_margin.txt); here the same quantity is formed from ``_gate_probe.probe_model`` against the fp64 trunk on the
bench frame's calibrated networks and the trained fixture: every point keeps the factor 8, and no point of positive density is
culled.

kappa was fitted on those networks.  ``test_the_cull_decision_on_trained_and_held_out_networks`` holds the DECISION on every
trained network the project has - the lightly trained fixture and the two hold-out fits of tests/golden/probe_holdout_*.npz (ten
times as many steps on the same scene; a scene of narrow, high densities) - on uniform depths and on the fine pass's own resampled
depths: no culled point has positive fp64 density, and r + D <= kappa with D the recorded model-to-kernel distance, so that the
kernel cannot cull one either.  How much of the factor 8 these networks leave is printed, not asserted."""
import pytest
import torch

import _gate_probe as gp

N_RAYS = 256          # a strided subset of each network's 4096 rays x 64 / 192 depths: 16 384 / 49 152 points per case


@pytest.mark.parametrize("name", ["bench_coarse", "bench_fine", "trained_coarse", "trained_fine"])
def test_probe_keeps_a_factor_of_eight_to_the_margin(name):
    sd, rays = gp.network(name)
    rays = rays[:: rays.shape[0] // N_RAYS][:N_RAYS]
    n_samples = 64 if name.endswith("coarse") else 192
    x = gp.positions(rays, gp.sample_depths(rays, n_samples, seed=7))
    with torch.no_grad():
        sigma = gp.sigma_fp64(sd, x)
        s, big_s = gp.probe_model(sd, x)
    r = float(((s - sigma).abs() / big_s).max())
    culled = s < -gp.KAPPA * big_s
    band = ~culled & (sigma <= 0)
    print(f"{name}: {x.shape[0]} points, sigma > 0 on {float((sigma > 0).float().mean()):.4f}, r = {r:.3e} (8 r / kappa = {8 * r / gp.KAPPA:.3f}), "
          f"culled {float(culled.float().mean()):.4f}, margin band {float(band.float().mean()):.4f}")
    assert 0.05 < float((sigma > 0).float().mean()) < 0.95          # the inputs are fair: both signs are there
    assert bool((8.0 * (s - sigma).abs() <= gp.KAPPA * big_s).all())
    assert not bool((culled & (sigma > 0)).any())
    assert bool(culled.any())                                       # ... and the probe does cull (how much is a matter of speed, not of this test)


HELD_OUT_CASES = [(f"{family}_{lvl}", dset) for family in gp.HOLDOUT_FAMILIES
                  for lvl, dset in (("coarse", "uniform"), ("fine", "uniform"), ("fine", "z_fine"))]


@pytest.mark.parametrize("name,dset", HELD_OUT_CASES)
def test_the_cull_decision_on_trained_and_held_out_networks(name, dset):
    sd, _ = gp.network(name)
    z = gp.depth_sets(name)[dset]
    f = gp.case_figures(sd, gp.positions(gp.family_rays(name.rsplit("_", 1)[0]), z))
    print(gp.format_figures(f"{name} on {dset} depths {tuple(z.shape)}", f))
    assert f["finite"] and f["amax"] <= gp.F16_SAFE                  # the f16x3 path serves these points: no range flag
    assert f["culled_positive"] == 0
    assert f["r"] + gp.MODEL_TO_KERNEL <= gp.KAPPA
    assert f["positive"] >= gp.MIN_SHARE and f["culled"] >= gp.MIN_SHARE      # both sides of the rule are exercised
