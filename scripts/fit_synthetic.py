#!/usr/bin/env python3
"""Trained-network evidence: fit the coarse + fine intrinsic NeRF to an ANALYTIC scene through the product
front-end under autograd - the reference's training step (run_nerf.py:868-1027: random ray batch -> render(..., retraw=True)
-> img2mse on rgb_map + rgb0 -> Adam) - and then look at the TRAINED weights, which nothing else in the repo has:

  1. max |activation| per layer against the f16x3 kernel's range guard (7.5e3);
  2. parity of a held-out view against the CPU oracle (== reference): plain 1e-4 on every ray, the rank statistics of
     oracle/calibration.py, and the stage-by-stage strict report of oracle/stagewise.py;
  3. PSNR of the HIP and of the oracle render of that view against the analytic target, and their delta;
  4. whether training with the HIP network backward tracks training with torch's layers (INERF_TRAIN_MLP=torch) over a whole
     run from the same initial weights, batches and jitter: a soak of the forward-save / chain / weight-gradient kernels.

    python scripts/fit_synthetic.py [--steps 3000] [--torch-steps 1500] [--out gpurun_out/r03_trained_network.txt]
                                    [--scene {blobs,sharp}] [--net-seed 0] [--checkpoints 3000,10000 --save-weights W.pt]

The scene: five Gaussian density blobs with their own colours inside the chair camera's [2, 6] depth range, white
background; targets are rendered from the analytic field with 512 midpoint samples per ray (torch, fp64, on the GPU) from
24 poses of the NeRF-synthetic orbit at 100x100 (the data set itself is not available here).

``--scene sharp`` is a second analytic field behind the same two functions: blobs a quarter as wide and ten times as dense, and one
thin slab - a target that drives the weights further from their initialisation than the smooth one does (the hold-out networks of
tests/golden/make_golden_probe_holdout.py).  ``--checkpoints A,B`` saves both networks at those step counts of the one run, next
to ``--save-weights`` (W.pt -> W.stepA.pt, W.stepB.pt).
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

BLOBS = (  # centre xyz, sigma (width), peak density, colour
    ((0.0, 0.0, 0.0), 0.27, 18.0, (0.85, 0.25, 0.20)),
    ((0.7, 0.2, -0.3), 0.18, 25.0, (0.20, 0.70, 0.30)),
    ((-0.6, -0.4, 0.4), 0.21, 20.0, (0.25, 0.35, 0.90)),
    ((0.1, 0.8, 0.5), 0.15, 30.0, (0.90, 0.80, 0.20)),
    ((-0.3, 0.5, -0.7), 0.17, 22.0, (0.70, 0.30, 0.80)),
)
SHARP_BLOBS = tuple((c, 0.25 * s, 10.0 * a, rgb) for c, s, a, rgb in BLOBS)      # narrow and high: the same centres and colours
SHARP_SLABS = (  # centre xyz, unit normal, half-thickness sigma, lateral sigma, peak density, colour
    ((0.0, 0.0, -0.15), (0.0, 0.0, 1.0), 0.02, 0.6, 150.0, (0.55, 0.55, 0.50)),
)
SCENES = {"blobs": (BLOBS, ()), "sharp": (SHARP_BLOBS, SHARP_SLABS)}


def analytic_field(pts, scene="blobs"):
    """(density [..], colour [.., 3]) of the synthetic scene at ``pts[.., 3]`` (any float dtype)."""
    blobs, slabs = SCENES[scene]
    dens, col = 0.0, 0.0
    for c, s, a, rgb in blobs:
        g = a * torch.exp(-((pts - pts.new_tensor(c)) ** 2).sum(-1) / (2.0 * s * s))
        dens = dens + g
        col = col + g[..., None] * pts.new_tensor(rgb)
    for c, nrm, s, lat, a, rgb in slabs:                          # a Gaussian sheet: thin along its normal, wide across it
        rel = pts - pts.new_tensor(c)
        h = (rel * pts.new_tensor(nrm)).sum(-1)
        g = a * torch.exp(-h * h / (2.0 * s * s) - ((rel ** 2).sum(-1) - h * h) / (2.0 * lat * lat))
        dens = dens + g
        col = col + g[..., None] * pts.new_tensor(rgb)
    return dens, col / dens.clamp_min(1e-12)[..., None]


def analytic_render(rays, n=512, scene="blobs"):
    """White-background volume rendering of the analytic field along ``rays[N, 11]`` (fp64, midpoint rule)."""
    r = rays.double()
    o, d, near, far = r[:, 0:3], r[:, 3:6], r[:, 6:7], r[:, 7:8]
    t = (torch.arange(n, device=r.device, dtype=torch.float64) + 0.5) / n
    z = near + (far - near) * t
    dens, col = analytic_field(o[:, None, :] + d[:, None, :] * z[:, :, None], scene)
    delta = (far - near) / n * d.norm(dim=-1, keepdim=True)
    alpha = 1.0 - torch.exp(-dens * delta)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    w = alpha * trans
    return ((w[..., None] * col).sum(1) + (1.0 - w.sum(1, keepdim=True))).float()


def camera_rays(theta_deg, side, dev):
    """[side*side, 11] rays of the orbit camera at ``theta_deg`` (phi -30, radius 4: load_blender.py:29-34), near 2, far 6."""
    from intrinsicnerf_amd import object_level as ol
    focal = 0.5 * side / np.tan(0.5 * bench.CAMERA_ANGLE_X)
    K = np.array([[focal, 0, 0.5 * side], [0, focal, 0.5 * side], [0, 0, 1]])
    ro, rd = ol.get_rays(side, side, K, bench.chair_pose(theta_deg).to(dev))
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    vd = rd / rd.norm(dim=-1, keepdim=True)
    return torch.cat([ro, rd, bench.NEAR * torch.ones_like(vd[:, :1]), bench.FAR * torch.ones_like(vd[:, :1]), vd], -1).contiguous()


def make_nets(dev, seed=0):
    from intrinsicnerf_amd import object_level as ol
    embed, ch = ol.get_embedder(10, 0)
    embed_d, ch_d = ol.get_embedder(4, 0)
    torch.manual_seed(seed)
    mk = lambda: ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
    return mk(), mk(), ol.NetworkQuery(embed, embed_d)


def training_set(dev, n_poses=24, side=100, scene="blobs"):
    rays = torch.cat([camera_rays(360.0 * i / n_poses, side, dev) for i in range(n_poses)], 0)
    target = torch.cat([analytic_render(rays[i:i + 65536], scene=scene) for i in range(0, rays.shape[0], 65536)], 0)
    return rays, target


def fit(net_c, net_f, query, rays, target, steps, batch=2048, lr=5e-4, seed=1, log_every=0, at_step=None):
    """``steps`` training steps as run_nerf.py:868-1027 runs them (no_batching=True branch: a random batch of rays,
    perturb = 1, raw_noise_std = 0, white_bkgd, 64+128; loss = img2mse(rgb_map) + img2mse(rgb0); Adam, the reference's
    exponential lr decay with lrate_decay = 500).  ``at_step``: {step count: callable()}, called once that many steps are done.
    Returns the loss curve."""
    from intrinsicnerf_amd import object_level as ol
    opt = torch.optim.Adam(list(net_c.parameters()) + list(net_f.parameters()), lr=lr, betas=(0.9, 0.999))
    g = torch.Generator(device=rays.device).manual_seed(seed)
    torch.manual_seed(seed)                                       # t_rand of every step (perturb = 1) comes from the global generator
    losses = torch.zeros(steps, device=rays.device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for it in range(steps):
            sel = torch.randint(0, rays.shape[0], (batch,), device=rays.device, generator=g)
            ret = ol.render_rays(rays[sel], net_c, query, bench.N_SAMPLES, retraw=True, perturb=1.0, N_importance=bench.N_IMPORTANCE,
                                 network_fine=net_f, white_bkgd=True, raw_noise_std=0.0)
            loss = ((ret["rgb_map"] - target[sel]) ** 2).mean() + ((ret["rgb0"] - target[sel]) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            for pg in opt.param_groups:                           # run_nerf.py:1021-1026
                pg["lr"] = lr * (0.1 ** ((it + 1) / (500 * 1000)))
            losses[it] = loss.detach()
            if at_step and (it + 1) in at_step:
                at_step[it + 1]()
            if log_every and (it + 1) % log_every == 0:
                print(f"  step {it + 1}: loss {float(loss):.5f}", flush=True)
            if (it + 1) % 100 == 0 and not bool(torch.isfinite(losses[it - 99:it + 1]).all()):
                bad = int(torch.nonzero(~torch.isfinite(losses[:it + 1]))[0])
                raise FloatingPointError(f"the loss became non-finite at step {bad} (mode {os.environ.get('INERF_TRAIN_MLP', 'hip')})")
    return losses.cpu().numpy()


def layer_activation_maxima(net, query, rays, z):
    """max |activation| of every saved layer (include/inerf.h slot list) of ``net`` on the sample points (rays, z)."""
    from intrinsicnerf_amd import _capi, kernels, packing
    desc = net.fused_desc()
    d = _capi.NetDesc(desc.variant, desc.n_classes, desc.l_xyz, desc.l_dir, desc.xyz_div, _capi.PREC_F16X3)
    status = torch.zeros(1, dtype=torch.int32, device=rays.device)
    packed = packing.packed_for_module(net, d, rays.device)
    _, save = kernels.encode_mlp_train(d, packed, rays, z, status=status)
    views = kernels.save_slot_views(d, save, z.numel())
    names = {0: "encoding", 1: "dir encoding", 10: "albedo|shading hidden", 11: "feature", 12: "view hidden"}
    names.update({2 + i: f"pts_linears.{i}" for i in range(8)})
    out = {names[i]: float(v.abs().max()) for i, v in enumerate(views) if i in names}
    return out, bool(int(status.item()) & _capi.STATUS_F16_RANGE)


def evaluate(net_c, net_f, query, dev, side, lines, target_fn=analytic_render):
    """Held-out view (bench.py's pose, theta = 40): HIP render vs CPU oracle on the TRAINED weights."""
    import oracle
    from oracle import calibration as cal, stagewise
    from intrinsicnerf_amd import _capi, kernels, object_level as ol, packing
    rays = camera_rays(40.0, side, dev)
    target = target_fn(rays).cpu().numpy()
    with torch.no_grad():
        got = ol.render_rays(rays, net_c, query, bench.N_SAMPLES, N_importance=bench.N_IMPORTANCE, network_fine=net_f, white_bkgd=True)
    sd_c = {k: v.detach().cpu() for k, v in net_c.state_dict().items()}
    sd_f = {k: v.detach().cpu() for k, v in net_f.state_dict().items()}
    cfg = oracle.RenderConfig(variant="object", n_samples=bench.N_SAMPLES, n_importance=bench.N_IMPORTANCE, white_bkgd=True)
    to64 = lambda sd: {k: v.double() for k, v in sd.items()}
    r_cpu = rays.cpu()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with torch.no_grad():
        o32 = oracle.render_rays(r_cpu, sd_c, sd_f, cfg, stages=True)
        o64 = oracle.render_rays(r_cpu.double(), to64(sd_c), to64(sd_f), cfg, stages=True)
    # 1. activations of both trained networks on the view's own sample points
    lines.append("## 1. max |activation| per layer of the TRAINED networks on the held-out view's sample points (guard: 7.5e3)")
    z_c, z_f = o32["z_coarse"].to(dev), o32["z_fine"].to(dev)
    worst_act = 0.0
    for tag, net, z in (("coarse", net_c, z_c), ("fine", net_f, z_f)):
        acts, tripped = layer_activation_maxima(net, query, rays, z)
        worst_act = max(worst_act, max(v for k, v in acts.items() if "encoding" not in k))
        lines.append(f"{tag:6s} " + "  ".join(f"{k}: {v:.3g}" for k, v in acts.items()) + f"   range word tripped: {tripped}")
    lines.append(f"largest hidden activation: {worst_act:.4g} = {worst_act / 7.5e3:.2%} of the guard")
    # 2. parity of the view
    lines.append(f"## 2. parity of the held-out {side}x{side} view ({rays.shape[0]} rays, nothing filtered) against the CPU oracle, trained weights")
    pairs = (("rgb_map", "rgb_fine"), ("disp_map", "disp_fine"), ("acc_map", "acc_fine"), ("albedo_map", "albedo_fine"),
             ("shading_map", "shading_fine"), ("residual_map", "residual_fine"), ("rgb0", "rgb_coarse"), ("acc0", "acc_coarse"), ("z_std", "z_std"))
    tol = lambda k: 5e-4 if k.startswith("disp") else 1e-4
    summary = {"rays": int(rays.shape[0]), "maps": {}}
    for fk, ok in pairs:
        e = cal.scaled_errors(got[fk].cpu().numpy(), o32[ok].numpy(), tol(ok))
        e_ref = cal.scaled_errors(o32[ok].numpy(), o64[ok].numpy(), tol(ok))
        viol = cal.rank_report(e, e_ref)
        summary["maps"][fk] = {"beyond_plain_tol": int((~(e <= 1)).sum()), "ref_beyond_plain_tol": int((~(e_ref <= 1)).sum()), "rank_violations": viol}
        lines.append(f"{fk:13s} HIP vs oracle32: {cal.summarize(e)}")
        lines.append(f"{'':13s} oracle32 vs 64: {cal.summarize(e_ref)}" + (f"   RANK VIOLATIONS {viol}" if viol else ""))
    ref = {k: v.numpy() for k, v in o32.items() if v is not None}
    d0 = _capi.net_desc(_capi.VARIANT_OBJECT, 0, 10, 4, 1.0)
    st = stagewise.hip_stages(d0, packing.packed_for_module(net_c, d0, dev), packing.packed_for_module(net_f, d0, dev), rays, ref, True)
    per, problems = stagewise.strict_report(st, ref)
    summary["stagewise_violations"] = int(sum(v["violations"] for v in per.values()))
    lines.append("stage-wise strict (every ray, plain tolerance; worst in tolerances): " + "  ".join(f"{k}:{v['worst']:.2g}" for k, v in per.items()))
    lines.append(f"stage-wise violations: {summary['stagewise_violations']}" + ("" if not problems else "   " + "; ".join(problems)))
    # 3. PSNR against the analytic target
    p_hip = stagewise.psnr(got["rgb_map"].cpu().numpy(), target)
    p_o32 = stagewise.psnr(o32["rgb_fine"].numpy(), target)
    p_o64 = stagewise.psnr(o64["rgb_fine"].numpy(), target)
    e2 = float(np.mean((got["rgb_map"].cpu().numpy().astype(np.float64) - o32["rgb_fine"].numpy()) ** 2))
    mse = float(np.mean((o32["rgb_fine"].numpy().astype(np.float64) - target) ** 2))
    kdb = 10.0 / np.log(10.0)
    # MSE(HIP) - MSE(oracle) = mean(e^2) + 2 mean(e r), e = HIP - oracle, r = oracle - target: the first term is systematic, the
    # second averages out over the pixels (scale 2 sqrt(mean(e^2) mean(r^2) / n)) - it dominates on a small view of a barely fitted net
    summary.update(psnr_hip=p_hip, psnr_oracle=p_o32, psnr_delta_db=p_hip - p_o32, worst_activation=worst_act,
                   psnr_delta_systematic_db=-kdb * e2 / mse, psnr_delta_sampling_db=kdb * 2.0 * np.sqrt(e2 * mse / target.size) / mse)
    lines.append("## 3. PSNR of the held-out view against the analytic target (run_nerf_helpers.py:11-12)")
    lines.append(f"PSNR(HIP) = {p_hip:.7f} dB   PSNR(oracle fp32) = {p_o32:.7f} dB   delta = {p_hip - p_o32:+.3e} dB   "
                 f"(oracle fp32 vs fp64: {p_o32 - p_o64:+.3e} dB; budget 1e-4 dB; systematic part {summary['psnr_delta_systematic_db']:+.1e} dB, "
                 f"pixel-sampling scale {summary['psnr_delta_sampling_db']:.1e} dB on {target.size} values)")
    return summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--torch-steps", type=int, default=1500, help="length of the HIP-vs-torch-layers tracking run (0: skip)")
    ap.add_argument("--side", type=int, default=64, help="side of the held-out view")
    ap.add_argument("--out", default=os.path.join(REPO, "gpurun_out", "r03_trained_network.txt"))
    ap.add_argument("--save-weights", default="")
    ap.add_argument("--scene", choices=sorted(SCENES), default="blobs", help="the analytic field to fit")
    ap.add_argument("--net-seed", type=int, default=0, help="seed of the two networks' initialisation")
    ap.add_argument("--checkpoints", default="", help="A,B,C: also save both networks after that many steps (needs --save-weights)")
    a = ap.parse_args()
    checkpoints = sorted({int(c) for c in a.checkpoints.split(",") if c})
    if checkpoints and (not a.save_weights or checkpoints[0] < 1 or checkpoints[-1] > a.steps):
        ap.error("--checkpoints needs --save-weights and step counts in 1 .. --steps")
    import __graft_entry__
    __graft_entry__.build()
    dev = torch.device("cuda:0")
    lines = [f"# scripts/fit_synthetic.py --steps {a.steps} --torch-steps {a.torch_steps} --side {a.side} on {torch.cuda.get_device_name(0)}",
             "# analytic 5-blob scene, 24 poses x 100x100 rays, batch 2048, 64+128 samples, perturb 1, Adam 5e-4; object_level.render_rays under autograd"]
    if a.scene != "blobs" or a.net_seed != 0:
        lines.append(f"# scene {a.scene}, network seed {a.net_seed}")
    rays, target = training_set(dev, scene=a.scene)
    net_c, net_f, query = make_nets(dev, a.net_seed)
    save = lambda path: torch.save({"coarse": net_c.state_dict(), "fine": net_f.state_dict()}, path)
    stem, ext = os.path.splitext(a.save_weights)
    at_step = {c: (lambda c=c: save(f"{stem}.step{c}{ext}")) for c in checkpoints}
    if a.save_weights:
        os.makedirs(os.path.dirname(os.path.abspath(a.save_weights)), exist_ok=True)
    t0 = time.perf_counter()
    losses = fit(net_c, net_f, query, rays, target, a.steps, log_every=max(1, a.steps // 6), at_step=at_step)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    k = max(1, a.steps // 20)
    lines.append(f"## 0. fit: {a.steps} steps in {dt:.1f} s ({dt / a.steps * 1e3:.2f} ms/step); loss (mean of {k} steps) first {losses[:k].mean():.5f} -> last {losses[-k:].mean():.5f}"
                 f"  (train PSNR of the fine map ~ {-10 * np.log10(losses[-k:].mean() / 2):.2f} dB)")
    if a.save_weights:
        save(a.save_weights)
    summary = evaluate(net_c, net_f, query, dev, a.side, lines, target_fn=lambda r: analytic_render(r, scene=a.scene))
    if a.torch_steps > 0:
        lines.append(f"## 4. HIP network backward vs torch layers (INERF_TRAIN_MLP=torch): {a.torch_steps} steps, same initial weights, batches and jitter")
        curves, times = {}, {}
        for mode in ("hip", "torch"):
            os.environ["INERF_TRAIN_MLP"] = mode
            nc, nf, q = make_nets(dev)
            t0 = time.perf_counter()
            curves[mode] = fit(nc, nf, q, rays, target, a.torch_steps)
            torch.cuda.synchronize()
            times[mode] = (time.perf_counter() - t0) / a.torch_steps * 1e3
        os.environ.pop("INERF_TRAIN_MLP", None)
        w = max(1, a.torch_steps // 30)
        sm = lambda c: np.convolve(c, np.ones(w) / w, mode="valid")[::w]
        h, t = sm(curves["hip"]), sm(curves["torch"])
        rel = np.abs(h - t) / t
        lines.append(f"ms/step: hip {times['hip']:.2f}, torch {times['torch']:.2f}")
        lines.append("window-mean loss (hip | torch | rel. diff), windows of %d steps:" % w)
        for i in range(0, len(h), max(1, len(h) // 10)):
            lines.append(f"  steps {i * w:5d}..{i * w + w - 1:5d}: {h[i]:.6f} | {t[i]:.6f} | {rel[i]:.2e}")
        first = int(np.argmax(np.abs(curves["hip"] - curves["torch"]) > 1e-3 * curves["torch"])) if (np.abs(curves["hip"] - curves["torch"]) > 1e-3 * curves["torch"]).any() else a.torch_steps
        lines.append(f"per-step losses agree to 1e-3 relative for the first {first} steps (afterwards the two runs are different samples of the same "
                     f"chaotic optimisation); largest window-mean difference {rel.max():.2e}; final window: hip {h[-1]:.6f}, torch {t[-1]:.6f}")
        summary["tracking_max_window_rel_diff"] = float(rel.max())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return summary


if __name__ == "__main__":
    main()
