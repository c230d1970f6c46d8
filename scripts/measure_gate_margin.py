"""The gate probe's margin per network on the bench frame (profiles/gate_margin_bench.txt sections 1 and 2).

The frame's coarse and fine encode+MLP launches, each walked as ray prefixes 1, 2, 4, ... of the 640 000 rays on ONE margin state that is
read between the prefixes (the constant margin kept by INERF_PROBE_MIN_OBS): r over the first n listed points against r over all of
them - the table kProbeMinObserved comes from -, the whole-frame r, and the candidate shares at 2^-6 and at the adapted margin.
    python scripts/measure_gate_margin.py"""
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ["INERF_PROBE_MIN_OBS"] = "1e19"          # keep the constant while measuring
import bench
import __graft_entry__
__graft_entry__.build()
from oracle import calibration as cal
from intrinsicnerf_amd import _capi, kernels, object_level as ol, packing

dev = torch.device("cuda", 0)
K = bench.chair_intrinsics()
ro, rd = ol.get_rays(bench.H, bench.W, K, bench.chair_pose().to(dev))
ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
n = bench.H * bench.W
vd = rd / rd.norm(dim=-1, keepdim=True)
one = torch.ones_like(vd[:, :1])
rays = torch.cat([ro, rd, bench.NEAR * one, bench.FAR * one, vd], -1).contiguous()
sel = torch.arange(0, n, n // bench.PARITY_RAYS + 1, device=dev)[:bench.PARITY_RAYS]
rays_s = rays[sel].cpu()
t0 = time.time()
sd_c = cal.calibrated_default_init("object", 0, 0, rays_s)
sd_f = cal.calibrated_default_init("object", 0, 1, rays_s)
print(f"calibration {time.time() - t0:.1f} s", flush=True)
desc = _capi.net_desc(_capi.VARIANT_OBJECT, precision=_capi.PREC_F16X3)
pc, pf = packing.pack_state_dict(desc, sd_c).to(dev), packing.pack_state_dict(desc, sd_f).to(dev)
S_C, S_I = bench.N_SAMPLES, bench.N_IMPORTANCE
t_vals = torch.linspace(0., 1., S_C, device=dev)
u = torch.linspace(0., 1., S_I, device=dev)          # perturb = 0: sample_pdf's det = True
os.environ["INERF_PROBE_ADAPT"] = "0"
z_c = torch.empty(n, S_C, device=dev)
z_f = torch.empty(n, S_C + S_I, device=dev)
CH = 1 << 17
for b in range(0, n, CH):
    st = kernels.render_rays_fused(desc, pc, pf, rays[b:b + CH].contiguous(), S_C, S_I, t_vals, u, white_bkgd=True, want_stages=True)
    z_c[b:b + CH], z_f[b:b + CH] = st["z_coarse"], st["z_fine"]
torch.cuda.synchronize()
del os.environ["INERF_PROBE_ADAPT"]
print("stage depths ready", flush=True)

bounds = [0] + [1 << k for k in range(0, 20)] + [n]
for tag, packed, z in (("coarse", pc, z_c), ("fine", pf, z_f)):
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    rows = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        kernels.encode_mlp(desc, packed, rays[lo:hi].contiguous(), z[lo:hi].contiguous(), gate_colour=True, gate_probe=True, gate_state=state)
        m = kernels.gate_margin(state)
        rows.append((hi, m["observed"], m["r_max"]))
    r_all, obs_all = rows[-1][2], rows[-1][1]
    pts = n * z.shape[1]
    print(f"== {tag}: {n} rays x {z.shape[1]} = {pts} points, constant margin 2^-6: {obs_all} listed ({obs_all / pts:.4f}), whole-frame r = {r_all:.4e}, 8 r = {8 * r_all:.4e} = 2^{torch.log2(torch.tensor(8 * r_all)).item():.2f}")
    print("   rays_prefix   listed_points   r_over_them   r_all/r")
    for hi, obs, r in rows:
        print(f"   {hi:10d}   {obs:13d}   {r:.4e}   {(r_all / r) if r > 0 else float('inf'):.3f}")
    # the adapted margin: one more whole pass on the same state with the rule switched on
    os.environ["INERF_PROBE_MIN_OBS"] = "1"
    before = kernels.gate_margin(state)
    for lo in range(0, n, CH):
        kernels.encode_mlp(desc, packed, rays[lo:lo + CH].contiguous(), z[lo:lo + CH].contiguous(), gate_colour=True, gate_probe=True, gate_state=state)
    after = kernels.gate_margin(state)
    os.environ["INERF_PROBE_MIN_OBS"] = "1e19"
    listed = after["observed"] - before["observed"]
    print(f"   adapted: margin {after['kappa_in_use']:.4e} = 2^{torch.log2(torch.tensor(after['kappa_in_use'])).item():.2f}, {listed} listed ({listed / pts:.4f}), r_max after {after['r_max']:.4e}", flush=True)
