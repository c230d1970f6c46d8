#!/usr/bin/env python3
"""Hold-out networks for the density gate's probe margin: trained weights that kappa was NOT fitted to.

    python scripts/fit_synthetic.py --steps 30000 --torch-steps 0 --scene blobs --net-seed 0 --checkpoints 3000,10000,30000 \\
        --save-weights weights/holdout_long.pt                                  (on an MI355X: ten times the trained fixture's steps)
    python scripts/fit_synthetic.py --steps 10000 --torch-steps 0 --scene sharp --net-seed 1 --save-weights weights/holdout_sharp.pt
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_probe_holdout.py long weights/holdout_long.step30000.pt
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_probe_holdout.py sharp weights/holdout_sharp.pt
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_probe_holdout.py --report weights/holdout_long.step3000.pt ...

Runs on the CPU and needs nothing but this repository: the weights come from the project's own trainer, the rays are every 16th of
the held-out 64 x 64 view of scripts/fit_synthetic.py (theta = 40), their fine-pass depths are the oracle's ``z_fine`` on the trained
weights.  A fixture holds what the probe and sigma depend on - pts_linears.* and alpha_linear.* of both networks (493 313 fp32 values
each), the 256 rays and z_fine [256, 192] - as tests/golden/probe_holdout_<name>.npz plus parts probe_holdout_<name>.<n>.npz, each
below 1 MiB (tests/_gate_probe.py holdout_fixture reads them back as one).

Before anything is written the script asserts what tests/test_gate_probe_cpu.py restates: every value finite, no scaled activation
beyond the f16 range flag's 6e4, and on every pair of network and depth set at least 2 % of the points with fp64 sigma > 0 and at
least 2 % culled by the probe model.  ``--report`` prints the same figures for any number of checkpoints and writes nothing (the
r-versus-steps trend of profiles/gate_probe_margin.txt).
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.dirname(HERE), os.path.join(REPO, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _gate_probe as gp  # noqa: E402
import fit_synthetic  # noqa: E402


def load(path):
    ck = torch.load(path, map_location="cpu")
    return tuple({k: v.float().contiguous() for k, v in ck[lvl].items()} for lvl in ("coarse", "fine"))


def cases(sd_c, sd_f):
    """(rays [256, 11], z_fine [256, 192], {case: figures}) of one checkpoint."""
    rays = fit_synthetic.camera_rays(40.0, 64, torch.device("cpu"))[::16].contiguous()
    assert rays.shape == (gp.N_RAYS, 11)
    z_fine = gp.oracle_fine_depths(sd_c, sd_f, rays)
    sets = (("coarse", sd_c, "uniform", gp.sample_depths(rays, 64, seed=7)), ("fine", sd_f, "uniform", gp.sample_depths(rays, 192, seed=7)),
            ("fine", sd_f, "z_fine", z_fine))
    return rays, z_fine, {f"{lvl} on {dset}": gp.case_figures(sd, gp.positions(rays, z)) for lvl, sd, dset, z in sets}


def init_distance(sd, level, net_seed):
    """|theta - theta_init| / |theta_init| over the trunk, theta_init from the trainer's own initialisation."""
    init = fit_synthetic.make_nets(torch.device("cpu"), net_seed)[level].state_dict()
    num = sum(float((sd[k].double() - init[k].double()).square().sum()) for k in gp.TRUNK_KEYS)
    den = sum(float(init[k].double().square().sum()) for k in gp.TRUNK_KEYS)
    return (num / den) ** 0.5


def report(path, net_seed=None):
    sd_c, sd_f = load(path)
    rays, z_fine, figs = cases(sd_c, sd_f)
    for tag, f in figs.items():
        print(gp.format_figures(f"{os.path.basename(path)} {tag}", f))
    if net_seed is not None:
        print(f"{os.path.basename(path)}: trunk weights at relative distance {init_distance(sd_c, 0, net_seed):.3f} (coarse) / "
              f"{init_distance(sd_f, 1, net_seed):.3f} (fine) from their initialisation")
    return sd_c, sd_f, rays, z_fine, figs


def main(argv):
    if argv and argv[0] == "--report":
        for path in argv[1:]:
            report(path)
        return
    which, path = argv
    sd_c, sd_f, rays, z_fine, figs = report(path, gp.HOLDOUT_SEED[which])
    for tag, f in figs.items():
        assert f["finite"], tag
        assert f["amax"] <= gp.F16_SAFE, f"{tag}: the f16 range flag would be raised ({f['amax']:.4g}): take an earlier checkpoint"
        assert f["positive"] >= gp.MIN_SHARE and f["culled"] >= gp.MIN_SHARE, f"{tag}: one side of the rule only"
    assert bool(torch.isfinite(z_fine).all()) and z_fine.shape == (gp.N_RAYS, 192)
    fx = {"rays": rays.numpy(), "z_fine": z_fine.numpy()}
    for lvl, sd in (("coarse", sd_c), ("fine", sd_f)):
        for k in gp.TRUNK_KEYS:
            assert bool(torch.isfinite(sd[k]).all()), k
            fx[f"w_{lvl}/{k}"] = sd[k].numpy().astype(np.float32)
    paths = gp.write_holdout_fixture(which, fx)
    sizes = [os.path.getsize(p) for p in paths]
    assert max(sizes) < 1 << 20 and sum(sizes) < 5 << 20, sizes
    print(f"wrote {len(paths)} parts of probe_holdout_{which}: {sizes} bytes, {sum(sizes)} in all")


if __name__ == "__main__":
    main(sys.argv[1:])
