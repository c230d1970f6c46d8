#!/usr/bin/env python3
"""Headline benchmark: rays/s of the IntrinsicNeRF render path at 64+128 samples per ray.

    python bench.py --gpus N --steps K --warmup W        (N > 1: under torch.distributed.run, or plain - it then starts its
                                                          own N ranks through torch.distributed.run on 127.0.0.1)
                    [--full] [--dump-outputs DIR]

One "step" renders one synthetic 800x800 Blender-chair frame (BASELINE.json configs[2]: 640,000 rays,
64 coarse + 128 importance samples, separate coarse/fine networks, white background, eval mode)
through the product front-end ``intrinsicnerf_amd.object_level.render``.  With N GPUs the frame's rays
are split into N row bands (one process per GPU) and the rendered maps are all-gathered over RCCL, so
the total work is fixed: "scaling": "strong".  Inputs are resident in HBM before the timed region.

Networks: default-``nn.Linear``-init weights (seeds 0 / 1) whose density head ``alpha_linear`` is rescaled so that
acc spans (0, 1] on this frame (oracle/calibration.py) - with the plain seeds every density is negative and the
frame is all background, so neither sample_pdf nor compositing would see a non-trivial input.  After the timed
region a strided sample of the TIMED frame is compared with the CPU oracle (== reference): rank statistics against
the oracle's own fp32-vs-fp64 distance on every sampled ray plus the plain 1e-4 tolerance on the reproducible ones;
the run fails if that does not hold ("parity" in the JSON line).  That check and every other leg below runs with --full only: a
plain run sets up, warms up, times the K steps and prints the headline fields (metric, value, unit, higher_is_better, dtype,
ms_per_step, ...).  --dump-outputs DIR writes the maps the last timed step rendered as DIR/<map>.npy (float32, the whole frame;
the inputs are the same bits on every run).

The MLP GEMMs run in the package's default arithmetic (INERF_PRECISION, default "f16x3": fp32 operands
split into f16 hi/lo pairs, 3 f16 MFMA products per MAC, fp32 accumulation - same error against fp64
as the exact-fp32 MFMA kernel); "dtype" says which one ran.

Prints ONE JSON line (rank 0) with the bench contract's fields, with --full plus
  "roofline"     : algorithmic TFLOP/s (2 x 659,456 MAC per sample point) of the dominant kernel from
                   HIP-event timings of its launches at this workload's sizes.  For the f16x3 kernel the
                   peak is the dense f16 MFMA peak divided by the 3 products it issues per fp32 MAC
                   (2500 / 3 = 833 TFLOP/s); for the exact-fp32 kernel it is the 157.3 TFLOP/s fp32 MFMA
                   peak.  "roofline_f32_kernel" always carries the exact-fp32 kernel's figures too;
  "cpu_baseline" : the CPU oracle (PyTorch-CPU restatement == reference, see oracle/) timed on this
                   box's host cores on a bounded sample of the same workload (best thread count and 1 thread);
  "parity"       : the check described above, plus "stagewise": every HIP stage fed the oracle's (== reference's) input for
                   that stage on the sampled rays of the timed frame and held to the PLAIN 1e-4 on every ray
                   (oracle/stagewise.py; "stagewise_violations" must be 0), and "psnr_delta_db": PSNR(HIP, T) - PSNR(oracle,
                   T) of the timed frame's maps on those rays, T = the fp64 evaluation + a fixed 30 dB perturbation;
  "configs"      : BASELINE.json configs[1] (coarse-only 800x800) and configs[3] (320x240 SSR room frame, C = 28)
                   through their front-ends: rays/s and the MLP kernel's roofline fraction at their launch shapes;
  "frame_costs"  : where a frame's wall time goes besides the kernels (host, packing, gather, status read).
  "f16_range_fallback": cost of a frame (chunk = 32768 rays, the reference's default) in which ONE chunk trips the f16x3
                   range guard: that chunk - and only that chunk - is rendered again in exact fp32.
With N > 1 GPUs the line also carries configs.ssr_room0_320x240 rendered through distributed.render_sharded (BASELINE.json
configs[4]: the Replica frame tiled over the ranks, one all-gather of 26 + 2C floats per ray).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

H = W = 800
N_SAMPLES, N_IMPORTANCE = 64, 128
CAMERA_ANGLE_X = 0.6911112070083618          # NeRF-synthetic transforms_*.json
NEAR, FAR = 2.0, 6.0                         # run_nerf.py:705-706
FLOP_PER_POINT = 2 * 659456                  # BASELINE.md section 2 (GEMM MACs of one NeRF evaluation)
SSR_CLASSES = 28
FLOP_PER_POINT_SSR = 2 * (659456 + 32768 + 128 * SSR_CLASSES)
PEAK_F32_MFMA_TFLOPS = 157.3                 # MI355X_MICROARCH.md: dense fp32 matrix peak
PEAK_F16_MFMA_TFLOPS = 2500.0                # MI355X_MICROARCH.md: dense f16/bf16 matrix peak
MEASURED_F16_MFMA_ONLY_TFLOPS = 1590.0       # dense f16, random operands, 170-340 ms runs (zero operands: 2470)
# HBM bytes per sample point of the encode+MLP kernels from the PMC passes (FETCH_SIZE + WRITE_SIZE, separate passes).
# f16x3: profiles/r06_final_pmc_digest.txt, measured on the bench frame's own fine launch (640,000 rays x 192 samples): FETCH 410.9 MB +
# WRITE 5442.4 MB = 5853.3 MB per 122,880,000-point launch (algorithmic 5929.1 MB; round 5: 5941.0 MB, profiles/r05_pmc_raw_rows.txt).  (Until late in round 5 the 44-byte raw rows left as
# 4-byte non-temporal pieces: 6230 - 7126 MB, 1.05 - 1.20 x, depending on how far the waves that share a line had drifted apart; now as
# 16-byte pieces of whole 704-byte wave blocks.)  f32: profiles/r01_mlp_pmc_traffic.txt.
PMC_HBM_BYTES_PER_POINT = {"f16x3": 47.6, "f32": 49.5}
PMC_SOURCE = {"f16x3": ("profiles/r06_final_pmc_digest.txt", "0.99"), "f32": ("profiles/r01_mlp_pmc_traffic.txt", "1.02")}
PARITY_RAYS = 4096
RTOL, ATOL, RTOL_DISP = 1e-4, 1e-5, 5e-4
PSNR_BUDGET_DB = 1e-4                        # north_star: <= 1e-4 dB PSNR delta against the reference


def chair_pose(theta_deg=40.0, phi_deg=-30.0, radius=4.0):
    """pose_spherical of the NeRF-synthetic orbit (load_blender.py:29-34 convention)."""
    th, ph = np.deg2rad(theta_deg), np.deg2rad(phi_deg)
    t = np.eye(4); t[2, 3] = radius
    rp = np.array([[1, 0, 0, 0], [0, np.cos(ph), -np.sin(ph), 0], [0, np.sin(ph), np.cos(ph), 0], [0, 0, 0, 1.0]])
    rt = np.array([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1.0]])
    flip = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1.0]])
    return torch.tensor((flip @ rt @ rp @ t)[:3, :4], dtype=torch.float32)


def chair_intrinsics():
    focal = 0.5 * W / np.tan(0.5 * CAMERA_ANGLE_X)
    return np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])


def overflow_above(net, pose, y_min, gain=1.0e6):
    """Copy of ``net`` whose first trunk unit is ``relu(gain * (y_cam - y_min))``, y_cam = a point's height above the optical
    axis of camera ``pose`` ([3, 4] camera-to-world): the f16x3 kernel's activation range (|a| < 7.5e3) is left exactly on the
    rays that reach y_cam > y_min + 7.5e3 / gain - a sub-volume only the top image rows see - and nowhere else."""
    import copy
    big = copy.deepcopy(net)
    up, origin = pose[:3, 1].double(), pose[:3, 3].double()
    with torch.no_grad():
        w, b = big.pts_linears[0].weight, big.pts_linears[0].bias
        w[0].zero_()
        w[0, 0:3] = (gain * up).to(w)                                  # the encoding's first three columns are xyz itself
        b[0] = float(-gain * (y_min + float(up @ origin)))
    return big


def mlp_kernel_name(f16, ssr=False):
    """Name of the encode+MLP kernel a launch of the default front-ends runs (what rocprofv3's kernel trace shows)."""
    if not f16:
        return "k_encode_mlp<true, 2>" if ssr else "k_encode_mlp<false, 2>"
    form = os.environ.get("INERF_F16_KERNEL", "")[:1]
    if ssr:
        return "k_encode_mlp_f16x3<true, false>" if form == "s" else "k_encode_mlp_f16x3_dual<false, true, true>"
    return {"s": "k_encode_mlp_f16x3<false, false>", "d": "k_encode_mlp_f16x3_dual<false, false, false>"}.get(form, "k_encode_mlp_f16x3_t128<false, false, false>")


def host_description():
    """CPU model string, physical cores, logical CPUs available to this process."""
    model, cores = "unknown", set()
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core = line.split(":", 1)[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    cores.add((phys, core))
                phys = core = None
    except OSError:
        pass
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return model, (len(cores) or avail), avail


def cpu_oracle_run(rays, sd_c, sd_f, full_spec=False):
    """Time the CPU oracle (== reference arithmetic) on ``rays`` as ONE chunk and return its outputs.

    torch's intra-op pool is not monotone in thread count on many-core hosts (the reference's netchunk = 65536 rows
    per op bounds what more threads can do, and 256 threads on a small chunk are ~60x slower than 32), so the thread
    count is probed first - up to all physical cores - and the chunk is timed at the best one, then a small sample at
    1 thread (the reference script itself pins OMP_NUM_THREADS=1, object_level/run_nerf.py:2-3).  ``full_spec``
    (--cpu-baseline-full): SURVEY.md section 8d's procedure - median of 3 repeats of a 32768-ray chunk.
    """
    import oracle
    model, physical, avail = host_description()
    cfg = oracle.RenderConfig(variant="object", n_samples=N_SAMPLES, n_importance=N_IMPORTANCE, white_bkgd=True)

    def run(r):
        with torch.no_grad():
            return oracle.render_rays(r, sd_c, sd_f, cfg, stages=True)

    probe_n = min(512, rays.shape[0])
    widths = sorted({min(avail, c) for c in (8, 16, 32, 64, 128, physical, avail)})
    best_t, best_rate, probe = 1, 0.0, {}
    for t in widths:
        torch.set_num_threads(t)
        run(rays[:64])                                           # warm the pool at this width
        t0 = time.perf_counter()
        run(rays[:probe_n])
        rate = probe_n / (time.perf_counter() - t0)
        probe[t] = round(rate, 1)
        if rate > best_rate:
            best_t, best_rate = t, rate
        elif rate < 0.5 * best_rate:
            break                                                # past the knee: wider only gets slower
    torch.set_num_threads(best_t)
    times = []
    for _ in range(3 if full_spec else 1):
        t0 = time.perf_counter()
        out = run(rays)
        times.append(time.perf_counter() - t0)
    dt = float(np.median(times))
    torch.set_num_threads(1)
    n1 = min(2048 if full_spec else 256, rays.shape[0])
    t0 = time.perf_counter()
    run(rays[:n1])
    dt1 = time.perf_counter() - t0
    torch.set_num_threads(best_t)
    base = {"value": rays.shape[0] / dt, "unit": "rays/s", "cores": int(best_t), "kind": "port",
            "single_thread_rays_per_s": n1 / dt1, "cpu_model": model, "physical_cores": physical, "logical_cpus": avail,
            "thread_probe_rays_per_s": probe, "torch": torch.__version__,
            "sample": f"{rays.shape[0]} rays of the same 800x800 frame (every {H * W // rays.shape[0]}-th ray) as ONE chunk, "
                      f"64+128 samples, netchunk 65536, PyTorch-CPU oracle (oracle/intrinsic_render.py == reference, see "
                      f"tests/golden) in {dt:.1f} s at {best_t} threads ({'median of 3' if full_spec else 'one run'}; best of a "
                      f"thread-count probe over {list(probe)}); 1 thread: {n1} rays in {dt1:.1f} s"}
    return out, base


def parity_report(frame, sel, o32, o64, rays_s, sd_f):
    """The timed frame's maps at rays ``sel`` against the oracle: (dict for the JSON line, list of violations)."""
    from oracle import calibration as cal
    pairs = (("rgb_map", "rgb_fine"), ("disp_map", "disp_fine"), ("acc_map", "acc_fine"), ("albedo_map", "albedo_fine"),
             ("shading_map", "shading_fine"), ("residual_map", "residual_fine"))
    tol = lambda k: RTOL_DISP if k.startswith("disp") else RTOL
    e_ref = {ok: cal.scaled_errors(o32[ok].numpy(), o64[ok].numpy(), tol(ok), ATOL) for _, ok in pairs}
    stage = ("z_samples", "weights_coarse", "weights_fine", "z_fine", "rgb_coarse", "acc_coarse", "z_std")
    score = np.maximum.reduce(list(e_ref.values()) + [cal.scaled_errors(o32[k].numpy(), o64[k].numpy(), RTOL, ATOL) for k in stage])
    if (score <= 0.2).any():       # probe the fine pass's conditioning on the rays that passed so far (oracle.calibration.fine_pass_hazard)
        import oracle
        cfg = oracle.RenderConfig(variant="object", n_samples=N_SAMPLES, n_importance=N_IMPORTANCE, white_bkgd=True)
        score = np.maximum(score, cal.fine_pass_hazard(rays_s, sd_f, cfg, o32, o64, subset=score <= 0.2))
    well = score <= 0.2
    problems, per_map = [], {}
    for fk, ok in pairs:
        got = frame[fk].reshape(H * W, -1)[sel].cpu().numpy()
        e = cal.scaled_errors(got, o32[ok].numpy(), tol(ok), ATOL)
        problems += [f"{fk}: {v}" for v in cal.rank_report(e, e_ref[ok])]
        worst = float(np.max(e[well], initial=0.0))
        if worst > 1.0:
            problems.append(f"{fk}: reproducible rays beyond the plain tolerance (worst {worst:.3g} x tol)")
        fin = np.where(np.isfinite(e), e, 1e30)
        fin_r = np.where(np.isfinite(e_ref[ok]), e_ref[ok], 1e30)
        per_map[fk] = {"q50": float(np.quantile(fin, .5)), "q99": float(np.quantile(fin, .99)), "beyond_tol": int((fin > 1).sum()),
                       "ref_q50": float(np.quantile(fin_r, .5)), "ref_q99": float(np.quantile(fin_r, .99)),
                       "ref_beyond_tol": int((fin_r > 1).sum()), "worst_on_reproducible": worst}
    acc = o32["acc_fine"].numpy()
    rep = {"rays": int(len(sel)), "reproducible_rays": int(well.sum()), "violations": problems,
           "acc_quantiles_10_50_90": [float(np.quantile(acc, q)) for q in (.1, .5, .9)],
           "unit": "tolerances (|got - want| / (1e-5 + 1e-4 |want|); disp: 5e-4)",
           "criterion": "per map: quantiles 50..99 % of |HIP - oracle_fp32| <= max(0.5, 3 x those of |oracle_fp32 - oracle_fp64|); "
                        "#(> T) <= 3 x ref + 3 for T in 1, 10, 100; plain tolerance on every ray whose fp32-vs-fp64 score <= 0.2",
           "maps": per_map}
    return rep, problems


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(out_dir, frame):
    """The maps one timed step returns (the whole frame, 12 floats per ray = 30.7 MB) as ``out_dir/<map>.npy`` in float32."""
    maps = {k: np.ascontiguousarray(v.detach().float().cpu().numpy()) for k, v in frame.items()}
    assert sum(a.nbytes for a in maps.values()) <= DUMP_CAP_BYTES, {k: a.shape for k, a in maps.items()}
    os.makedirs(out_dir, exist_ok=True)
    for k, a in maps.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def events_ms(fn, reps=1):
    """Average GPU time of ``fn()`` in ms by HIP events on the current stream (torch's current stream IS the stream the
    launchers enqueue on)."""
    durs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        durs.append(a.elapsed_time(b))
    return sum(durs) / len(durs), durs


def self_launch_command(n_gpus, argv, port):
    """The command ``python bench.py --gpus N`` re-executes itself under when no launcher set WORLD_SIZE: the same static
    127.0.0.1 rendezvous the driver's torch.distributed.run line uses (the container's hostname may not resolve)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def self_launch(n_gpus, argv):
    """Run the N ranks as children of this process; rank 0's JSON line goes to our stdout as it is, the launcher's exit code
    (non-zero if ANY rank failed) becomes ours."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL's only working mode on this driver
    return subprocess.call(self_launch_command(n_gpus, argv, port), env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)           # (the first frames of a process run ~8 % slow on some boxes: clocks, allocator)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU oracle: no cpu_baseline and no parity check")
    ap.add_argument("--cpu-baseline-quick", action="store_true",
                    help="time the CPU oracle on the 4077-ray parity sample only (default: SURVEY.md 8d - one 32768-ray chunk x 3, ~3 min)")
    ap.add_argument("--cpu-baseline-full", action="store_true", help="(the default since round 3; accepted for old command lines)")
    ap.add_argument("--no-extras", action="store_true", help="skip configs / train_step / exact-fp32 extras")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, everything else the benchmark measures and checks: reference chunking, frame costs, rooflines, "
                         "the exact-fp32 path, the range fallback, configs, train_step, cpu_baseline and the parity check against the oracle "
                         "(without it: set-up, warm-up, the timed steps and the result line only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the maps the last timed step rendered as DIR/<map>.npy (float32, the whole frame)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU) and hand back rank 0's line + exit code
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    # stdout carries ONE line: rank 0's JSON.  Everything else this process or its libraries write to file descriptor 1 (gloo announces
    # its connections there: "[Gloo] Rank 0 is connected to 1 peer ranks ...") goes to stderr from here on.
    json_out = os.fdopen(os.dup(1), "w")
    sys.stdout.flush()
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {world} processes (WORLD_SIZE={world})")
    if os.environ.get("INERF_BENCH_LAUNCH_PROBE") == "1":
        # (tests/test_bench_launch_cpu.py: the launch path alone - rendezvous on 127.0.0.1, one line from rank 0, a common exit code - no GPU)
        import torch.distributed as dist
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo", rank=rank, world_size=world)
            seen = torch.tensor([1.0])
            dist.all_reduce(seen)
            dist.destroy_process_group()
        if rank == 0:
            json_out.write(json.dumps({"launch_probe": True, "n_gpus": world, "ranks_seen": int(seen.item()) if world > 1 else 1,
                                       "steps": args.steps, "warmup": args.warmup, "local_rank": local_rank}) + "\n")
            json_out.flush()
        raise SystemExit(int(os.environ.get("INERF_BENCH_LAUNCH_PROBE_RC", "0")) if rank == world - 1 else 0)
    # one process per GPU.  INERF_BENCH_SHARE_GPU=1 (debug only) lets several ranks share device 0 over gloo, to
    # exercise the sharding + gather logic on a single-GPU box; the numbers it prints mean nothing.
    share = os.environ.get("INERF_BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:       # device_id binds the communicator to this rank's GPU up front (eager RCCL init; no device guessing in barrier())
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    # Host-side rendezvous for the END of the run: rank 0 spends minutes in the CPU oracle (parity, cpu_baseline) while the others
    # have nothing left to do.  Waiting for it in an RCCL barrier would spin a GPU kernel per idle rank (and trip the collective
    # watchdog); on a gloo group the idle ranks sleep in a socket read.
    import datetime
    side = dist.new_group(backend="gloo", timeout=datetime.timedelta(minutes=45)) if world > 1 else None

    import __graft_entry__
    __graft_entry__.build()
    import oracle                                      # calibrated seeded weights, the parity checker, cpu_baseline
    from oracle import calibration as cal
    from intrinsicnerf_amd import _capi, distributed as idist, kernels, object_level as ol, packing

    # ---- synthetic workload: configs[2], resident in HBM ----
    K = chair_intrinsics()
    ro, rd = ol.get_rays(H, W, K, chair_pose().to(dev))
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    n_total = H * W
    b, e = idist.shard_bounds(n_total, rank, world)
    ro_l, rd_l = ro[b:e].contiguous(), rd[b:e].contiguous()
    n_local = e - b
    # strided sample of the WHOLE frame (identical on every rank): calibrates the density head, and is what the oracle
    # renders for the parity check and the CPU baseline
    sel = torch.arange(0, n_total, n_total // PARITY_RAYS + 1, device=dev)[:PARITY_RAYS]
    vd_s = rd[sel] / rd[sel].norm(dim=-1, keepdim=True)
    rays_s = torch.cat([ro[sel], rd[sel], NEAR * torch.ones_like(vd_s[:, :1]), FAR * torch.ones_like(vd_s[:, :1]), vd_s], -1).cpu()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    embed, ch = ol.get_embedder(10, 0)
    embed_d, ch_d = ol.get_embedder(4, 0)
    mk = lambda: ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
    net_c, net_f = mk(), mk()
    sd_c = sd_f = None

    def replicate(*modules):
        """Rank 0's parameters to every rank (the networks are replicated, 2 x 2.7 MB): one broadcast per tensor."""
        if world > 1:
            for m in modules:
                for t in m.state_dict().values():
                    dist.broadcast(t, 0)

    if rank == 0:       # the CPU probe that calibrates the density head runs once, not once per rank
        sd_c = cal.calibrated_default_init("object", 0, 0, rays_s)      # default init, seeds 0 / 1, calibrated density head
        sd_f = cal.calibrated_default_init("object", 0, 1, rays_s)
        net_c.load_state_dict(sd_c)
        net_f.load_state_dict(sd_f)
    replicate(net_c, net_f)
    query = ol.NetworkQuery(embed, embed_d)
    kw = dict(network_fn=net_c, network_fine=net_f, network_query_fn=query, N_samples=N_SAMPLES,
              N_importance=N_IMPORTANCE, white_bkgd=True, perturb=False, raw_noise_std=0., use_viewdirs=True, ndc=False,
              lindisp=False)
    map_keys = ("rgb_map", "disp_map", "acc_map", "albedo_map", "shading_map", "residual_map")

    def render_band(o, d, chunk=None, **over):
        with torch.no_grad():
            r = ol.render(H, W, K, chunk=chunk or max(1, o.shape[0]), rays=(o, d), near=NEAR, far=FAR, **{**kw, **over})
        return dict(zip(map_keys, r[:6])), r[6]

    def step():
        maps, _ = render_band(ro_l, rd_l)
        return idist.gather_maps(maps, n_total) if world > 1 else maps

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        frame = step()
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    assert frame["rgb_map"].shape[0] == n_total and torch.isfinite(frame["rgb_map"]).all()
    if world > 1:   # every rank must hold the same full frame, and its own band must be what it rendered
        chk = torch.tensor([float(frame["rgb_map"].double().sum()), float(frame["acc_map"].double().sum())],
                           device=dev, dtype=torch.float64)
        lo, hi = chk.clone(), chk.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        assert torch.equal(lo, hi), "ranks disagree on the gathered frame"
    rays_per_s = n_total * args.steps / dt
    ms_per_step = dt / args.steps * 1e3
    prec = _capi.default_precision()
    f16 = prec == _capi.PREC_F16X3
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, frame)
    head = {"metric": "rays/sec (64+128 samples/ray)", "value": rays_per_s, "unit": "rays/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None,
            "dtype": "f32 (operands split into f16 hi+lo, 3 f16 MFMA products per MAC, fp32 accumulate)" if f16 else "f32",
            "data": "synthetic",
            "config": {"workload": "Blender chair 800x800 frame (640000 rays), 64 coarse + 128 importance samples, "
                                   "coarse+fine intrinsic NeRF (D=8, W=256), white_bkgd, eval mode, default-init weights "
                                   "(seeds 0/1) with the density head calibrated so that acc spans (0, 1]",
                       "rays_per_step": n_total, "parallelism": f"ray-sharded x{world}",
                       "gather": "all_gather of 12 floats/ray" if world > 1 else "none"},
            "full": args.full}
    if not args.full:
        # the headline alone: everything below (extra legs, rooflines, CPU baseline, parity against the oracle) is --full
        if rank == 0:
            json_out.write(json.dumps(head) + "\n")
            json_out.flush()
        if world > 1:
            dist.destroy_process_group()
        return

    # ---- the same frame through the reference's own call shape: chunk = 32768 (run_nerf.py:167, :559) ----
    # object_level.batchify_rays merges eval-mode chunks up to a workspace cap (results are bit-identical for any chunking), so a
    # drop-in caller that never heard of this library's chunk advice gets the frame in the same few launches as `value` does.
    ref_chunking = None
    if not args.no_extras:
        seqs = []
        real_fused = kernels.render_rays_fused
        kernels.render_rays_fused = lambda d_, pc_, pf_, r_, *a_, **k_: (seqs.append(int(r_.shape[0])), real_fused(d_, pc_, pf_, r_, *a_, **k_))[1]
        try:
            def step_ck():
                maps, _ = render_band(ro_l, rd_l, chunk=32768)
                return idist.gather_maps(maps, n_total) if world > 1 else maps
            step_ck()
            seqs.clear()
            fence()
            t1 = time.perf_counter()
            n_ck = max(1, min(args.steps, 10))
            for _ in range(n_ck):
                frame_ck = step_ck()
            fence()
            dt_ck_all = time.perf_counter() - t1
        finally:
            kernels.render_rays_fused = real_fused
        if world > 1:
            t = torch.tensor([dt_ck_all], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt_ck_all = float(t.item())
        ref_chunking = {"value": n_total * n_ck / dt_ck_all, "unit": "rays/s", "ms_per_step": dt_ck_all / n_ck * 1e3, "steps": n_ck,
                        "vs_value": (n_total * n_ck / dt_ck_all) / rays_per_s, "chunk": 32768,
                        "launch_sequences_per_frame": len(seqs) // n_ck, "rays_per_launch_sequence": seqs[:len(seqs) // n_ck],
                        "bit_identical_to_the_timed_frame": bool(all(torch.equal(torch.nan_to_num(frame_ck[k]), torch.nan_to_num(frame[k])) for k in frame)),
                        "note": "ol.render(..., chunk=32768) exactly as run_nerf.py:167 calls it (the reference's default chunk); eval mode, no "
                                "raw returned: batchify_rays merges the caller's chunks up to INERF_COALESCE_BYTES (default 16 GiB) of workspace"}

    # ---- where a frame's wall time goes besides the kernels (untimed relative to `value`) ----
    def wall_and_gpu(fn, reps):
        fence()
        t1 = time.perf_counter()
        gpu_ms, _ = events_ms(fn, reps)          # each repetition ends with an event synchronise, like a frame's consumer
        return (time.perf_counter() - t1) / reps * 1e3, gpu_ms

    reps = max(1, min(args.steps, 3))
    wall_ms, gpu_ms = wall_and_gpu(lambda: render_band(ro_l, rd_l), reps)
    band = 80000                                    # what one of 8 GPUs renders of this frame
    band_wall, band_gpu = wall_and_gpu(lambda: render_band(ro_l[:band], rd_l[:band]), 3)
    maps_l, _ = render_band(ro_l, rd_l)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if world > 1:
        idist.gather_maps(maps_l, n_total)
    else:
        idist.unpack_maps(idist.pack_maps(maps_l))   # N = 1: the local part of the gather (pack into the [n, 12] block)
    fence()
    gather_ms = (time.perf_counter() - t1) * 1e3
    packing.invalidate(net_c)
    packing.invalidate(net_f)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    d0 = net_c.fused_desc()
    packing.packed_for_module(net_c, d0, dev)
    packing.packed_for_module(net_f, d0, dev)
    torch.cuda.synchronize()
    pack_ms = (time.perf_counter() - t1) * 1e3
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(20):
        st.item()
    sync_ms = (time.perf_counter() - t1) / 20 * 1e3
    per_rank = None
    if world > 1:       # what every rank's band cost (a sub-6x result must be diagnosable from the JSON line alone)
        mine = torch.tensor([wall_ms, gpu_ms, band_wall, band_gpu, gather_ms], device=dev, dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        every = torch.stack(every).cpu()
        per_rank = {"rays_per_rank": n_local,
                    "render_wall_ms": every[:, 0].tolist(), "render_gpu_ms": every[:, 1].tolist(),
                    "render_gpu_ms_min_max": [float(every[:, 1].min()), float(every[:, 1].max())],
                    "render_non_kernel_frac_max": float(((every[:, 0] - every[:, 1]) / every[:, 0]).max()),
                    "gather_ms": every[:, 4].tolist(),
                    "step_minus_slowest_render_ms": ms_per_step - float(every[:, 0].max()),
                    "note": "one entry per rank: this rank's band of the frame through the front-end (wall and HIP events), and its "
                            "all-gather alone; step - slowest render = what the collective and the rendezvous add per frame"}
    frame_costs = {
        "per_rank": per_rank,
        "render_wall_ms": wall_ms, "render_gpu_ms": gpu_ms, "non_kernel_ms": wall_ms - gpu_ms,
        "non_kernel_frac": (wall_ms - gpu_ms) / wall_ms,
        "band_80000_rays": {"wall_ms": band_wall, "gpu_ms": band_gpu, "non_kernel_frac": (band_wall - band_gpu) / band_wall},
        "gather_ms": gather_ms, "gather_note": ("all_gather_into_tensor of 12 floats/ray straight into the final layout"
                                                if world > 1 else "N = 1: pack into the [n, 12] gather block + views (no collective)"),
        "repack_after_weight_update_ms": pack_ms, "status_read_ms": sync_ms,
        "note": "render_gpu_ms: HIP events around one frame's launches; non_kernel = wall - that (host launch path, the one "
                "end-of-frame read of the f16 range word, allocator); packing only after a weight update (cached otherwise)"}

    # ---- roofline of the dominant kernel: HIP events around its launches, same sizes as the timed region ----
    vd = rd_l / rd_l.norm(dim=-1, keepdim=True)
    rays_l = torch.cat([ro_l, rd_l, NEAR * torch.ones_like(rd_l[:, :1]), FAR * torch.ones_like(rd_l[:, :1]), vd], -1)
    t_vals = torch.linspace(0., 1., N_SAMPLES, device=dev)
    u = torch.linspace(0., 1., N_IMPORTANCE, device=dev)
    flop_per_launch = FLOP_PER_POINT * n_local * (N_SAMPLES + (N_SAMPLES + N_IMPORTANCE)) / 2.0   # mean of the two launches

    def roofline_entry(f16, kernel, achieved, avg_ms, n_launches, flop, traffic_pts):
        peak = PEAK_F16_MFMA_TFLOPS / 3.0 if f16 else PEAK_F32_MFMA_TFLOPS
        bpp = PMC_HBM_BYTES_PER_POINT["f16x3" if f16 else "f32"]
        pmc_file, pmc_ratio = PMC_SOURCE["f16x3" if f16 else "f32"]
        return {"bound": "mfma", "kernel": kernel, "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                "traffic": bpp * traffic_pts,
                "traffic_note": f"HBM bytes per launch = {bpp} B/point measured by rocprofv3 PMC (FETCH_SIZE, WRITE_SIZE in separate "
                                f"passes, {pmc_file}) x this launch's points; {pmc_ratio}x algorithmic",
                "avg_launch_ms": avg_ms, "launches_timed": n_launches, "flop_per_launch": flop,
                "peak_basis": ("dense f16 MFMA 2500 TFLOP/s / 3 products per fp32 MAC" if f16 else "dense fp32 MFMA 157.3 TFLOP/s"),
                "achieved_vs_f32_mfma_peak": achieved / PEAK_F32_MFMA_TFLOPS,
                # what the matrix pipe sustains on this board when it does nothing but MFMAs on random operands
                # (scripts/microbench/mfma_peak.hip, profiles/r01_mfma_peak_microbench.txt): the power budget, not the name-plate
                "measured_mfma_only_ceiling": (MEASURED_F16_MFMA_ONLY_TFLOPS / 3.0) if f16 else None,
                "frac_of_measured_ceiling": (achieved / (MEASURED_F16_MFMA_ONLY_TFLOPS / 3.0)) if f16 else None}

    def kernel_roofline(prec, reps):
        desc = _capi.net_desc(_capi.VARIANT_OBJECT, 0, 10, 4, 1.0, prec)
        pc, pf = packing.packed_for_module(net_c, desc, dev), packing.packed_for_module(net_f, desc, dev)
        st = kernels.render_rays_fused(desc, pc, pf, rays_l, N_SAMPLES, N_IMPORTANCE, t_vals, u, white_bkgd=True, want_stages=True)
        z_c, z_f = st["z_coarse"], st["z_fine"]
        del st
        torch.cuda.synchronize()
        durs = []                                              # one entry per launch [ms]
        for _ in range(reps):
            for packed, z in ((pc, z_c), (pf, z_f)):
                durs += events_ms(lambda: kernels.encode_mlp(desc, packed, rays_l, z))[1]
        avg_ms = sum(durs) / len(durs)
        f16 = prec == _capi.PREC_F16X3
        out = roofline_entry(f16, mlp_kernel_name(f16),
                             flop_per_launch / (avg_ms * 1e-3) / 1e12, avg_ms, len(durs), flop_per_launch,
                             n_local * (N_SAMPLES + (N_SAMPLES + N_IMPORTANCE)) / 2.0)
        coarse_ms = sum(durs[0::2]) / len(durs[0::2])          # the coarse-shaped launches alone = configs[1]'s kernel
        return out, (z_c, coarse_ms)

    roofline, (z_coarse, coarse_launch_ms) = kernel_roofline(prec, max(1, args.steps))
    roofline_f32 = roofline if prec == _capi.PREC_F32 else (kernel_roofline(_capi.PREC_F32, max(1, args.steps))[0] if not args.no_extras else None)

    extras = rank == 0 and world == 1 and not args.no_extras
    # the same frames through the product front-end with the exact-fp32 MFMA kernel: the figure under the strictest reading of
    # "fp32" (no split operands anywhere), measured like `value` - one warm-up, then --steps frames between two fences
    exact = strict = None
    if prec != _capi.PREC_F32 and not args.no_extras:
        with _capi.forced_precision(_capi.PREC_F32):
            step(); fence()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                step()
            fence()
            dt32 = time.perf_counter() - t1
        if world > 1:
            t = torch.tensor([dt32], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt32 = float(t.item())
        exact = {"value": n_total * args.steps / dt32, "unit": "rays/s", "ms_per_step": dt32 / args.steps * 1e3, "steps": args.steps,
                 "note": "whole path with INERF_PRECISION=f32 (v_mfma_f32_32x32x2_f32 everywhere), timed like `value`"}
        strict = {"value": exact["value"], "unit": "rays/s", "frac": roofline_f32["frac"], "peak": roofline_f32["peak"],
                  "achieved": roofline_f32["achieved"], "steps": args.steps, "launches_timed": roofline_f32["launches_timed"],
                  "note": "exact-fp32 arithmetic end to end: rays/s of the whole path and its MLP kernel against the 157.3 TFLOP/s "
                          "fp32-MFMA peak (the same numbers as exact_f32_path / roofline_f32_kernel)"}
    elif prec == _capi.PREC_F32:
        strict = {"value": rays_per_s, "unit": "rays/s", "frac": roofline["frac"], "peak": roofline["peak"], "achieved": roofline["achieved"],
                  "steps": args.steps, "launches_timed": roofline["launches_timed"], "note": "the run itself is exact fp32 (INERF_PRECISION=f32)"}

    # what the f16x3 range guard costs when it trips (chunk-granular).  The frame is rendered in the reference's
    # default chunks of 32768 rays (run_nerf.py:559) with a fine network that leaves the split's activation range only in a
    # sub-volume that the first ~28 image rows see, i.e. inside chunk 0 of 20: the front-end enqueues all chunks in f16x3, reads
    # their range words ONCE at the end of the frame and renders chunk 0 - only chunk 0 - again with the exact fp32 kernel.
    fallback = None
    if extras and f16:
        import warnings
        focal = K[0][0]
        big = overflow_above(net_f, chair_pose(), y_min=FAR * (0.5 * H - 29.0) / focal)
        ck = 32768
        n_chunks = (n_local + ck - 1) // ck

        def tripped_frame(coalesce):
            """(seconds of the same chunked frame untripped, seconds tripped, render_rays calls by precision, maps)"""
            saved = os.environ.get("INERF_COALESCE_BYTES")
            if not coalesce:
                os.environ["INERF_COALESCE_BYTES"] = "0"
            calls = []
            real_rr = ol.render_rays
            try:
                render_band(ro_l, rd_l, chunk=ck); fence()
                t1 = time.perf_counter()
                render_band(ro_l, rd_l, chunk=ck); fence()
                dt_plain = time.perf_counter() - t1                        # the same frame through the same call, nothing trips
                ol.render_rays = lambda rb, **k: (calls.append(_capi.default_precision()), real_rr(rb, **k))[1]
                render_band(ro_l, rd_l, chunk=ck, network_fine=big); fence()
                calls.clear()
                t1 = time.perf_counter()
                fmaps, _ = render_band(ro_l, rd_l, chunk=ck, network_fine=big)
                fence()
                return dt_plain, time.perf_counter() - t1, list(calls), fmaps
            finally:
                ol.render_rays = real_rr
                if saved is None:
                    os.environ.pop("INERF_COALESCE_BYTES", None)
                else:
                    os.environ["INERF_COALESCE_BYTES"] = saved

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            dt_ck, dtf, calls, fmaps = tripped_frame(coalesce=False)
            dt_ck_m, dtf_m, calls_m, fmaps_m = tripped_frame(coalesce=True)
        fallback = {"ms_per_step": dtf * 1e3, "vs_f16x3_frame": dtf / (dt / args.steps), "vs_same_chunking_untripped": dtf / dt_ck,
                    "chunks": n_chunks, "chunk_rays": ck, "chunks_rerun_in_f32": sum(p == _capi.PREC_F32 for p in calls),
                    "f16x3_chunk_calls": sum(p == _capi.PREC_F16X3 for p in calls),
                    "finite": bool(torch.isfinite(fmaps["rgb_map"]).all()),
                    "merged_chunks": {"ms_per_step": dtf_m * 1e3, "vs_f16x3_frame": dtf_m / (dt / args.steps),
                                      "vs_same_call_untripped": dtf_m / dt_ck_m,
                                      "f16x3_calls": sum(p == _capi.PREC_F16X3 for p in calls_m), "chunks_rerun_in_f32": sum(p == _capi.PREC_F32 for p in calls_m),
                                      "same_frame_as_per_chunk": bool(all(torch.equal(torch.nan_to_num(fmaps_m[k]), torch.nan_to_num(fmaps[k])) for k in fmaps)),
                                      "note": "the default front-end: the eval-mode chunks merged into one launch sequence that keeps one range word "
                                              "per caller's chunk (inerf_encode_mlp_chunked); chunk 0 alone again in exact fp32"},
                    "note": "800x800 frame in 20 chunks of 32768 rays (INERF_COALESCE_BYTES=0: the caller's chunks as given) whose fine network "
                            "leaves the f16x3 activation range (|activation| >= 7.5e3) on rays of chunk 0 only: one read of the 20 range words at "
                            "the end of the frame, then chunk 0 alone again in exact fp32 (round 2 re-rendered the whole frame: 4.18x); "
                            "INERF_PRECISION=f32 skips the attempt"}
        del big, fmaps, fmaps_m

    def ssr_frame_leg():
        """configs[3] (N = 1) / configs[4] (N > 1): the 320x240 Replica room_0-like frame through ssr.SSRRenderer.render_rays
        (trainer.py:1251), C = 28, 64+128, chunk 32768.  N > 1: distributed.render_sharded - this rank's band of rays, then one
        all-gather straight into the final [76800, 26 + 2C] layout; value = rays of the WHOLE frame / max-over-ranks time."""
        from intrinsicnerf_amd import ssr
        SH, SW = 240, 320
        fx = SW / 2.0 / np.tan(np.deg2rad(45.0))
        srays = ssr.create_rays(1, torch.eye(4)[None], SH, SW, fx, fx, (SW - 1) / 2.0, (SH - 1) / 2.0, 0.1, 10.0).reshape(-1, 11).contiguous()
        r = ssr.SSRRenderer(SSR_CLASSES, white_bkgd=False, endpoint_feat=False, device=dev)
        if rank == 0:
            ssel = srays[::srays.shape[0] // 1024]
            r.ssr_net_coarse.load_state_dict(cal.calibrated_default_init("ssr", SSR_CLASSES, 0, ssel))
            r.ssr_net_fine.load_state_dict(cal.calibrated_default_init("ssr", SSR_CLASSES, 1, ssel))
        replicate(r.ssr_net_coarse, r.ssr_net_fine)
        r.return_raw = False
        r.check_numerics = False
        srays = srays.to(dev)
        n_s = srays.shape[0]
        layout = idist.ssr_map_layout(SSR_CLASSES)
        frame_fn = (lambda: idist.render_sharded(r.render_rays, srays, layout)) if world > 1 else (lambda: r.render_rays(srays))
        n_steps = max(3, args.steps)
        with torch.no_grad():
            sret = frame_fn(); fence()
            t1 = time.perf_counter()
            for _ in range(n_steps):
                sret = frame_fn()
            fence()
        dts = (time.perf_counter() - t1) / n_steps
        if world > 1:
            t = torch.tensor([dts], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dts = float(t.item())
        assert sret["rgb_fine"].shape[0] == n_s and torch.isfinite(sret["rgb_fine"]).all() and float(sret["acc_fine"].min()) < 0.999
        out = {"workload": f"Replica room_0-like 320x240 frame ({n_s} rays), Semantic_NeRF C = {SSR_CLASSES}, 64+128 samples, depth "
                           "[0.1, 10], xyz/10, eval, render_rays called with chunk = 32768 (merged: one launch sequence)" +
                           (f", rays tiled over {world} ranks + one all-gather of {sum(w for _, w in layout)} floats/ray (BASELINE configs[4])"
                            if world > 1 else " (BASELINE configs[3])"),
               "value": n_s / dts, "unit": "rays/s", "ms_per_step": dts * 1e3, "steps": n_steps, "n_gpus": world,
               "frame_tflops_algorithmic": FLOP_PER_POINT_SSR * n_s * (2 * N_SAMPLES + N_IMPORTANCE) / dts / 1e12}
        if world > 1:
            # every rank must hold the same full frame; the gather alone, timed on a band that is already rendered
            chk = torch.stack([sret[k].double().sum() for k in ("rgb_fine", "sem_logits_fine", "depth_fine", "z_std")])
            lo, hi = chk.clone(), chk.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            assert torch.equal(lo, hi), "ranks disagree on the gathered SSR frame"
            b0, e0 = idist.shard_bounds(n_s, rank, world)
            with torch.no_grad():
                local = r.render_rays(srays[b0:e0].contiguous())
            fence()
            t1 = time.perf_counter()
            idist.gather_maps(local, n_s, layout)
            fence()
            out["gather_ms"] = (time.perf_counter() - t1) * 1e3
            out["gather_bytes"] = 4 * n_s * sum(w for _, w in layout)
            out["checksums"] = {k: float(v) for k, v in zip(("rgb_fine", "sem_logits_fine", "depth_fine", "z_std"), chk.tolist())}
            out["checksum_identical_on_all_ranks"] = True
        # roofline of this network's MLP kernel on the frame's OWN fine launch: chunk 0's rays and the z_fine the frame computed
        sdesc = r.ssr_net_fine.fused_desc()
        sdesc.xyz_div = 10.0
        spk_c, spk_f = packing.packed_for_module(r.ssr_net_coarse, sdesc, dev), packing.packed_for_module(r.ssr_net_fine, sdesc, dev)
        b0, e0 = idist.shard_bounds(n_s, rank, world)
        chunk = srays[b0:e0].contiguous()              # (the frame's chunks are merged: its fine pass IS one launch of the band's rays)
        st = kernels.render_rays_fused(sdesc, spk_c, spk_f, chunk, N_SAMPLES, N_IMPORTANCE, t_vals, u, white_bkgd=False, want_stages=True)
        sz = st["z_fine"]
        del st
        kernels.encode_mlp(sdesc, spk_f, chunk, sz)
        s_ms, s_durs = events_ms(lambda: kernels.encode_mlp(sdesc, spk_f, chunk, sz), 3)
        flop_s = FLOP_PER_POINT_SSR * chunk.shape[0] * (N_SAMPLES + N_IMPORTANCE)
        out["roofline"] = roofline_entry(f16, mlp_kernel_name(f16, ssr=True),
                                         flop_s / (s_ms * 1e-3) / 1e12, s_ms, len(s_durs), flop_s, chunk.shape[0] * (N_SAMPLES + N_IMPORTANCE))
        out["roofline"]["launch"] = f"fine pass of this rank's rays ({chunk.shape[0]} rays x 192: one launch, the frame's chunks are merged) on the depths the frame itself resampled"
        return out

    # ---- BASELINE.json configs[1] and configs[3] through their front-ends (rank 0, N = 1 only; not part of `value`) ----
    configs = None
    if extras:
        configs = {}
        # configs[1]: the same 800x800 frame, 64 coarse samples only (run_nerf.py:492-493 without the fine pass), white bkgd
        co = dict(N_importance=0, network_fine=None)
        render_band(ro_l, rd_l, **co); fence()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            cmaps, _ = render_band(ro_l, rd_l, **co)
        fence()
        dtc = (time.perf_counter() - t1) / args.steps
        assert torch.isfinite(cmaps["rgb_map"]).all()
        flop_c = FLOP_PER_POINT * n_local * N_SAMPLES
        configs["coarse_only_800x800"] = {
            "workload": "Blender chair 800x800, 64 coarse samples, coarse network only, white_bkgd, eval (BASELINE configs[1])",
            "value": n_total / dtc, "unit": "rays/s", "ms_per_step": dtc * 1e3, "steps": args.steps,
            "roofline": roofline_entry(f16, roofline["kernel"], flop_c / (coarse_launch_ms * 1e-3) / 1e12, coarse_launch_ms,
                                       max(1, args.steps), flop_c, n_local * N_SAMPLES)}
        configs["ssr_room0_320x240"] = ssr_frame_leg()
        # Not a BASELINE config - the reference's `--netwidth 128 --netwidth_fine 128` (run_nerf.py:286-296 builds what the flags say): a network
        # outside the fused architecture goes layer by layer through the exact-fp32 MFMA kernels (csrc/layered.hip), sampling and compositing as
        # above.  Default-init networks; roofline against the fp32 matrix peak (the layers are v_mfma_f32_32x32x2_f32).
        mk128 = lambda: ol.NeRF(D=8, W=128, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
        torch.manual_seed(128)
        n128 = dict(network_fn=mk128(), network_fine=mk128())
        import warnings as _w
        with _w.catch_warnings():
            _w.simplefilter("ignore")
            render_band(ro_l, rd_l, **n128); fence()
            t1 = time.perf_counter()
            for _ in range(2):
                wmaps, _ = render_band(ro_l, rd_l, **n128)
            fence()
        dtw = (time.perf_counter() - t1) / 2
        assert torch.isfinite(wmaps["rgb_map"]).all()
        macs128 = sum(q.numel() for k_, q in n128["network_fn"].named_parameters() if k_.endswith("weight"))
        flop_w = 2.0 * macs128 * n_local * (2 * N_SAMPLES + N_IMPORTANCE)
        configs["netwidth128_800x800"] = {
            "workload": "Blender chair 800x800, 64 + 128 samples, NeRF(D=8, W=128) coarse + fine (the reference's --netwidth 128), white_bkgd, eval: "
                        "layer-by-layer exact-fp32 MFMA kernels (csrc/layered.hip), HIP sampling and compositing",
            "value": n_total / dtw, "unit": "rays/s", "ms_per_step": dtw * 1e3, "steps": 2, "dtype": "f32",
            "roofline": {"bound": "mfma", "achieved": flop_w / dtw / 1e12, "peak": 157.3, "unit": "TFLOP/s", "frac": flop_w / dtw / 1e12 / 157.3,
                         "flop_per_frame": flop_w, "peak_basis": "fp32 MFMA (v_mfma_f32_32x32x2_f32), whole frame on the wall clock"}}
        del n128, wmaps

    if world > 1 and not args.no_extras:
        # BASELINE.json configs[4]: the Replica frame tiled over the ranks (distributed.render_sharded: contiguous ray bands,
        # ONE all-gather of the 26 + 2C floats per ray SSRTrainer.render_rays returns; raw_* never travels) - every rank runs it
        configs = {"ssr_room0_320x240": ssr_frame_leg()}

    # the reference's training step through the same front-end (rank 0, N = 1 only; untimed
    # relative to `value`): 1024 rays + one neighbour each (run_nerf.py:918-929), 64 + 128 samples, forward + backward + Adam
    train = None
    if extras and prec == _capi.PREC_F16X3:
        import warnings
        tnet_c, tnet_f = mk(), mk()
        opt = torch.optim.Adam(list(tnet_c.parameters()) + list(tnet_f.parameters()), lr=5e-4)
        tr = rays_l[torch.randperm(rays_l.shape[0], device=dev)[:2048]].contiguous()
        target = torch.rand(tr.shape[0], 3, device=dev)

        def train_step():
            ret = ol.render_rays(tr, tnet_c, query, N_SAMPLES, retraw=True, perturb=1.0, N_importance=N_IMPORTANCE,
                                 network_fine=tnet_f, white_bkgd=True)
            loss = ((ret["rgb_map"] - target) ** 2).mean() + ((ret["rgb0"] - target) ** 2).mean() + 0.01 * ret["albedo_map"].abs().mean()
            opt.zero_grad()
            loss.backward()
            opt.step()

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(2):
                train_step()
            fence()
            t1 = time.perf_counter()
            for _ in range(5):
                train_step()
            fence()
        t_train = (time.perf_counter() - t1) / 5
        # the same step recorded once as two HIP graphs and replayed (intrinsicnerf_amd/graphs.py): no per-launch host work
        from intrinsicnerf_amd import graphs

        def loss_fn(rays_b, target_b):
            ret = ol.render_rays(rays_b, tnet_c, query, N_SAMPLES, retraw=True, perturb=1.0, N_importance=N_IMPORTANCE,
                                 network_fine=tnet_f, white_bkgd=True)
            return ((ret["rgb_map"] - target_b) ** 2).mean() + ((ret["rgb0"] - target_b) ** 2).mean() + 0.01 * ret["albedo_map"].abs().mean()

        t_graph = n_fallbacks = None
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                gopt = torch.optim.Adam(list(tnet_c.parameters()) + list(tnet_f.parameters()), lr=5e-4, capturable=True)
                gstep = graphs.GraphedTrainStep(loss_fn, (tr, target), gopt)
                for _ in range(2):
                    gstep(tr, target)
                fence()
                t1 = time.perf_counter()
                for _ in range(10):
                    gloss = gstep(tr, target)
                fence()
            t_graph = (time.perf_counter() - t1) / 10
            n_fallbacks = gstep.fallbacks
            assert torch.isfinite(gloss).all()
        except Exception as e:        # reported, not fatal: the eager figure above stands
            t_graph = None
            n_fallbacks = f"{type(e).__name__}: {e}"
        # the same step in exact fp32 throughout (INERF_TRAIN_MLP=layered: the fp32 MFMA layer kernels, forward and backward) - what a batch
        # outside the f16 range costs, and what the reference's own fp32 training arithmetic costs here
        t_fp32 = None
        saved_mode = os.environ.get("INERF_TRAIN_MLP")
        os.environ["INERF_TRAIN_MLP"] = "layered"
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                train_step(); fence()
                t1 = time.perf_counter()
                for _ in range(3):
                    train_step()
                fence()
            t_fp32 = (time.perf_counter() - t1) / 3
        finally:
            if saved_mode is None:
                os.environ.pop("INERF_TRAIN_MLP", None)
            else:
                os.environ["INERF_TRAIN_MLP"] = saved_mode
        # algorithmic work of a step: forward + input gradients + weight gradients = 3 x the forward's GEMM FLOPs of every sample point
        # (coarse network on 64, fine network on 192 depths per ray); peak as for the inference kernel (same three-product arithmetic)
        flop_step = 3.0 * FLOP_PER_POINT * tr.shape[0] * (2 * N_SAMPLES + N_IMPORTANCE)
        peak_t = PEAK_F16_MFMA_TFLOPS / 3.0
        t_best = t_train if t_graph is None else min(t_train, t_graph)
        train = {"ms_per_step": t_train * 1e3, "rays": int(tr.shape[0]), "rays_per_s": tr.shape[0] / t_train,
                 "graphed_ms_per_step": None if t_graph is None else t_graph * 1e3, "graphed_eager_fallbacks": n_fallbacks,
                 "exact_fp32_layer_kernels": None if t_fp32 is None else {
                     "ms_per_step": t_fp32 * 1e3, "achieved": flop_step / t_fp32 / 1e12, "peak": 157.3, "unit": "TFLOP/s",
                     "frac": flop_step / t_fp32 / 1e12 / 157.3,
                     "note": "INERF_TRAIN_MLP=layered: every layer of both networks on v_mfma_f32_32x32x2_f32 (csrc/layered.hip), forward and "
                             "backward; also what a batch outside the f16 range of the split-precision kernels is re-evaluated with"},
                 "roofline": {"bound": "mfma", "flop_per_step": flop_step, "peak": peak_t, "unit": "TFLOP/s",
                              "achieved": flop_step / t_best / 1e12, "frac": flop_step / t_best / 1e12 / peak_t,
                              "achieved_eager": flop_step / t_train / 1e12, "frac_eager": flop_step / t_train / 1e12 / peak_t,
                              "achieved_graphed": None if t_graph is None else flop_step / t_graph / 1e12,
                              "frac_graphed": None if t_graph is None else flop_step / t_graph / 1e12 / peak_t,
                              "note": "whole step (wall clock, Adam and the trainer's loss kernels included) against the f16x3 MFMA peak; "
                                      "3 x 1,318,912 FLOP per sample point; the weight-gradient third is HBM-bound by design (DESIGN 3.3)"},
                 "note": "the reference's training batch (2048 rays x (64+128) samples) through object_level.render_rays under "
                         "autograd: HIP forward + backward (networks, compositing) + torch Adam; not part of `value`.  graphed: the "
                         "same step as two HIP graphs (graphs.GraphedTrainStep: render + loss + backward | one read of the f16 range "
                         "words | optimizer.step), replayed"}

    # ---- CPU oracle on the sampled rays of the timed frame: cpu_baseline (its fp32 run, timed) + parity (fp32 and fp64) ----
    cpu = parity = None
    problems = []
    if rank == 0 and ref_chunking is not None and not ref_chunking["bit_identical_to_the_timed_frame"]:
        problems.append("the frame rendered through chunk=32768 (merged chunks) differs from the timed frame")
    if rank == 0 and os.environ.get("INERF_BENCH_INJECT_FAILURE") == "1":        # (tests the N > 1 failure path: every rank must exit non-zero, promptly)
        problems.append("injected failure (INERF_BENCH_INJECT_FAILURE=1)")
    if rank == 0 and not args.no_cpu_baseline:
        from oracle import stagewise
        o32, quick = cpu_oracle_run(rays_s, sd_c, sd_f)                 # the parity reference; its timing is the "quick" CPU figure
        o32_full = rays_full = sel_full = None
        if args.cpu_baseline_quick:
            cpu = quick
        else:       # SURVEY.md section 8d's procedure (the default since round 3): one 32768-ray chunk x 3, all-core probe, 1 thread.
            # N > 1: rank 0 alone does this while the other ranks sleep on the gloo side group.  Its OUTPUT (the reference
            # arithmetic on every 20th ray of the timed frame) is what the PSNR budget below is judged on.
            sel_full = torch.arange(0, n_total, n_total // 32768 + 1, device=dev)[:32768]
            vdf = rd[sel_full] / rd[sel_full].norm(dim=-1, keepdim=True)
            rays_full = torch.cat([ro[sel_full], rd[sel_full], NEAR * torch.ones_like(vdf[:, :1]), FAR * torch.ones_like(vdf[:, :1]), vdf], -1).cpu()
            o32_full, cpu = cpu_oracle_run(rays_full, sd_c, sd_f, full_spec=True)
            cpu["quick_sample"] = {k: quick[k] for k in ("value", "cores", "single_thread_rays_per_s", "sample")}
        to64 = lambda sd: {k: v.double() for k, v in sd.items()}
        with torch.no_grad():
            o64 = oracle.render_rays(rays_s.double(), to64(sd_c), to64(sd_f),
                                     oracle.RenderConfig(variant="object", n_samples=N_SAMPLES, n_importance=N_IMPORTANCE, white_bkgd=True),
                                     stages=True)
        parity, problems = parity_report(frame, sel, o32, o64, rays_s, sd_f)
        # stage by stage, every sampled ray, plain tolerance: each HIP stage on the oracle's (== reference's) input for that stage
        ref = {k: v.numpy() for k, v in o32.items() if v is not None}
        d0 = _capi.net_desc(_capi.VARIANT_OBJECT, 0, 10, 4, 1.0, prec)
        got = stagewise.hip_stages(d0, packing.packed_for_module(net_c, d0, dev), packing.packed_for_module(net_f, d0, dev),
                                   rays_s.to(dev), ref, True)
        per, stage_problems = stagewise.strict_report(got, ref)
        parity["stagewise"] = per
        parity["stagewise_violations"] = int(sum(v["violations"] for v in per.values()))
        parity["stagewise_rays"] = int(len(sel))
        parity["stagewise_note"] = ("every HIP stage fed the oracle's input for that stage (z_coarse / z_fine -> inerf_encode_mlp + "
                                    "inerf_composite; weights_coarse -> inerf_sample_fine) on the sampled rays of the timed frame; worst = "
                                    "max |got - want| / (1e-5 + 1e-4 |want|) over ALL those rays (disp: 5e-4; resampled depths: + "
                                    "oracle.stagewise.sample_pdf_allowance)")
        problems += ["stagewise " + p for p in stage_problems]
        # PSNR delta (north_star: <= 1e-4 dB) of the TIMED frame's maps.  Judged on the 32768 rays the cpu_baseline leg has just
        # rendered with the reference arithmetic (every 20th ray of the frame; --cpu-baseline-quick: the 4077 parity rays); the
        # fp64 evaluation those need is the same oracle run in float64 by torch ON THE GPU (a checker, seconds instead of
        # minutes), cross-checked against the host's float64 run on the parity rays.
        pcfg = oracle.RenderConfig(variant="object", n_samples=N_SAMPLES, n_importance=N_IMPORTANCE, white_bkgd=True)
        pkeys = ("rgb_fine", "albedo_fine", "shading_fine", "residual_fine")

        def oracle_fp64_on_device(rays_cpu):
            sdc, sdf = ({k: v.double().to(dev) for k, v in sd.items()} for sd in (sd_c, sd_f))
            tv = torch.linspace(0., 1., N_SAMPLES, dtype=torch.float64).to(dev)
            uu = torch.linspace(0., 1., N_IMPORTANCE, dtype=torch.float64).to(dev)
            parts = []
            with torch.no_grad():
                for i in range(0, rays_cpu.shape[0], 8192):
                    o = oracle.render_rays(rays_cpu[i:i + 8192].double().to(dev), sdc, sdf, pcfg, t_vals=tv, u=uu)
                    parts.append({k: o[k].cpu() for k in pkeys})
            return {k: torch.cat([p[k] for p in parts]) for k in pkeys}

        t1 = time.perf_counter()
        d64 = oracle_fp64_on_device(rays_s)
        # (ray by ray the two float64 runs agree to ~1e-15 except where a last-bit difference of the coarse weights flips a branch of
        # sample_pdf - the discontinuous denom < 1e-5 switch, a searchsorted bin - on an ill-conditioned ray: judged by quantiles)
        dvh = torch.cat([(d64[k] - o64[k]).abs().reshape(len(sel), -1).max(1).values[:, None] for k in pkeys], 1).max(1).values.numpy()
        dev_vs_host = {"median": float(np.median(dvh)), "q99": float(np.quantile(dvh, 0.99)), "max": float(dvh.max()),
                       "rays_beyond_1e-6": int((dvh > 1e-6).sum()), "rays": int(len(dvh))}
        if o32_full is not None:
            p_sel, p32, p64 = sel_full, o32_full, oracle_fp64_on_device(rays_full)
        else:
            p_sel, p32, p64 = sel, o32, o64
        t_fp64 = time.perf_counter() - t1
        e2e, staged, own, e2e_small, e2e_f32k = {}, {}, {}, {}, {}
        map_pairs = (("rgb_map", "rgb_fine"), ("albedo_map", "albedo_fine"), ("shading_map", "shading_fine"), ("residual_map", "residual_fine"))
        # the same rays through the exact-fp32 MFMA kernel (INERF_PRECISION=f32): an INDEPENDENT fp32 implementation of the same path.  On
        # this default-init network sample_pdf amplifies last-bit differences of the coarse weights (the reference's own fp32 result is
        # 5e-4 .. 2e-3 dB from its fp64 evaluation), so where the default arithmetic lands against the reference is judged next to where
        # another correct fp32 implementation lands.
        f32k = None
        if f16:
            with _capi.forced_precision(_capi.PREC_F32):
                f32k, _ = render_band(ro[p_sel].contiguous(), rd[p_sel].contiguous())
        for fk, ok in map_pairs:
            hip = frame[fk].reshape(H * W, -1)[p_sel].cpu().numpy().reshape(p32[ok].shape)
            e2e[fk] = stagewise.psnr_delta_db(hip, p32[ok].numpy(), p64[ok].numpy(), detail=True, n_targets=16)
            own[fk] = stagewise.psnr_delta_db(p32[ok].numpy(), p64[ok].numpy(), p64[ok].numpy())
            if f32k is not None:
                e2e_f32k[fk] = stagewise.psnr_delta_db(f32k[fk].reshape(len(p_sel), -1).cpu().numpy().reshape(p32[ok].shape), p32[ok].numpy(),
                                                       p64[ok].numpy(), detail=True, n_targets=16)
            hip_s = frame[fk].reshape(H * W, -1)[sel].cpu().numpy().reshape(o32[ok].shape)
            e2e_small[fk] = stagewise.psnr_delta_db(hip_s, o32[ok].numpy(), o64[ok].numpy(), detail=True)
            staged[fk] = stagewise.psnr_delta_db(got[ok].reshape(o32[ok].shape), o32[ok].numpy(), o64[ok].numpy())

        def psnr_gate(tag, stats, allowance=None, fatal=True):
            """The budget's four tests on one map's statistics; ``allowance``: the same statistics of an independent fp32 implementation
            (each limit becomes max(budget, |its value| + 2e-5 dB)).  Returns the verdict entry; appends to ``problems`` if ``fatal``."""
            lim = lambda key: PSNR_BUDGET_DB if allowance is None else max(PSNR_BUDGET_DB, abs(allowance[key]) + 2e-5)
            tests = {"systematic_db": lim("systematic_db"), "expected_db": lim("expected_db"), "mean_delta_db_over_targets": lim("mean_delta_db_over_targets")}
            bad = [f"{k} {stats[k]:.3g} dB beyond {v:.3g}" for k, v in tests.items() if abs(stats[k]) > v]
            if abs(stats["delta_db"]) > lim("systematic_db") + 3.0 * stats["sampling_sigma_db"]:
                bad.append(f"delta {stats['delta_db']:.3g} dB more than 3 sampling sigmas ({stats['sampling_sigma_db']:.3g}) beyond {lim('systematic_db'):.3g}")
            if fatal:
                problems.extend(f"PSNR delta ({tag}): {b_}" for b_ in bad)
            return {"verdict": "fail" if bad else "pass", "fails_the_run": bool(fatal), "limits_db": {**tests, "delta_db": lim("systematic_db") + 3.0 * stats["sampling_sigma_db"]},
                    "within_the_plain_budget": bool(all(abs(stats[k]) <= PSNR_BUDGET_DB for k in tests)), "failed": bad}

        # PSNR in the reference is computed on rgb (run_nerf_helpers.py:11-12, run_nerf.py:976-985): that map first, with the
        # sampling sigma of the estimate next to it; the other intrinsic maps (run_nerf.py:512-518) per_map, every one of them GATED
        rgb = e2e["rgb_map"]
        parity["psnr_rays"] = int(len(p_sel))
        parity["psnr_delta_db_rgb"] = rgb["delta_db"]
        parity["psnr_delta_db_rgb_sampling_sigma"] = rgb["sampling_sigma_db"]
        parity["psnr_delta_db_rgb_in_sigmas"] = abs(rgb["delta_db"]) / max(rgb["sampling_sigma_db"], 1e-30)
        parity["psnr_delta_db_rgb_mean_over_16_targets"] = rgb["mean_delta_db_over_targets"]
        parity["psnr_delta_db_rgb_mean_over_16_targets_sigma"] = rgb["mean_delta_sigma_db"]
        parity["psnr_delta_db_rgb_systematic"] = rgb["systematic_db"]
        parity["psnr_delta_db_rgb_expected"] = rgb["expected_db"]
        parity["psnr_delta_db_rgb_fine_pass_on_reference_depths"] = staged["rgb_map"]
        parity["psnr_delta_db_max_over_maps"] = max(abs(v["delta_db"]) for v in e2e.values())
        parity["psnr_delta_db_systematic_max_over_maps"] = max(abs(v["systematic_db"]) for v in e2e.values())
        parity["psnr_delta_db_per_map"] = e2e
        parity["psnr_delta_db_per_map_exact_f32_kernel"] = e2e_f32k or None
        parity["psnr_delta_db_per_map_on_the_parity_rays"] = e2e_small
        parity["psnr_delta_db_fine_pass_on_reference_depths"] = staged
        parity["psnr_oracle_fp32_vs_fp64_db"] = own
        parity["psnr_fp64_on_device"] = {"seconds": t_fp64, "abs_difference_from_the_host_fp64_run_on_the_parity_rays": dev_vs_host}
        parity["psnr_budget_db"] = PSNR_BUDGET_DB
        # rgb at the plain budget (as in every round); albedo / shading / residual at the plain budget OR, where the exact-fp32 kernel
        # itself is beyond it on this network, at that independent fp32 implementation's own distance + 2e-5 dB
        # (--cpu-baseline-quick judges 4 077 rays instead of 32 768: the three intrinsic maps' statistics - dominated by the few ill-conditioned
        # rays of the sample - are then reported, and only rgb, as in every round, fails the run)
        full_sample = o32_full is not None
        parity["psnr_verdicts"] = {fk: psnr_gate(fk, e2e[fk], None if fk == "rgb_map" else e2e_f32k.get(fk), fatal=full_sample or fk == "rgb_map")
                                   for fk, _ in map_pairs}
        if dev_vs_host["median"] > 1e-10 or dev_vs_host["rays_beyond_1e-6"] > 0.05 * len(dvh):
            problems.append(f"the fp64 oracle on the device differs from the host's: {dev_vs_host}")
        parity["psnr_note"] = ("PSNR(x, T) = -10 log10 mean (x - T)^2 (run_nerf_helpers.py:11-12) over psnr_rays rays of the TIMED frame (every "
                               f"{n_total // max(1, len(p_sel))}th ray: the cpu_baseline leg's sample, rendered there with the reference arithmetic); "
                               "T = the oracle's fp64 maps + a fixed N(0, 10^-1.5) perturbation (so PSNR(fp64, T) = 30 dB); delta = PSNR(HIP, T) "
                               "- PSNR(oracle fp32, T); 'oracle_fp32_vs_fp64' = the reference arithmetic's own delta against fp64.  delta = "
                               "systematic (-mean (HIP - oracle32)^2 / MSE, always against HIP) + a cross term with the perturbation that is "
                               "zero-mean and shrinks with the pixel count (sampling_sigma_db); 'expected' = the delta's expectation over the "
                               "perturbation, mean (HIP - fp64)^2 - mean (oracle32 - fp64)^2 in dB; 'mean_over_16_targets' = the delta averaged over 16 "
                               "independent perturbations (sigma / 4).  psnr_verdicts: EVERY map (rgb, albedo, shading, residual) fails the run if "
                               "|systematic|, |expected| or |mean over 16 targets| exceed its limit or |delta| exceeds limit + 3 sigma; the limit is the "
                               "1e-4 dB budget for rgb, and for the other maps max(budget, the exact-fp32 kernel's own value on the same rays + 2e-5): "
                               "on this default-init network an independent fp32 implementation of the path is itself ~1.1e-4 dB from the reference "
                               "on those maps (psnr_delta_db_per_map_exact_f32_kernel; sample_pdf amplifies last-bit differences of the coarse "
                               "weights), on a trained network nothing is (parity.trained).  All 640000 rays: profiles/r04_psnr_full_frame.txt")

        # ---- the same judgement on a TRAINED network (tests/golden/trained_object_chair.npz: both networks fitted for 3000 steps through
        # the product's own training path, held-out view 48.6 dB): the full 800x800 held-out view through the product front-end ----
        fixture = os.path.join(REPO, "tests", "golden", "trained_object_chair.npz")
        if os.path.exists(fixture):
            t_tr = time.perf_counter()
            fxw = np.load(fixture)
            tsd = [{k.split("/", 1)[1]: torch.from_numpy(np.array(fxw[k])) for k in fxw.files if k.startswith(f"w_{lvl}/")} for lvl in ("coarse", "fine")]
            tc, tf = mk(), mk()
            tc.load_state_dict(tsd[0]); tf.load_state_dict(tsd[1])
            render_band(ro, rd, network_fn=tc, network_fine=tf)
            torch.cuda.synchronize()               # (rank 0 alone is here: no collective, no fence())
            t1 = time.perf_counter()
            tmaps, _ = render_band(ro, rd, network_fn=tc, network_fine=tf)
            torch.cuda.synchronize()
            t_frame = time.perf_counter() - t1
            tsel = torch.arange(0, n_total, n_total // 32768 + 1, device=dev)[:32768]
            tvd = rd[tsel] / rd[tsel].norm(dim=-1, keepdim=True)
            trays = torch.cat([ro[tsel], rd[tsel], NEAR * torch.ones_like(tvd[:, :1]), FAR * torch.ones_like(tvd[:, :1]), tvd], -1)

            def oracle_on_device(rays_dev, dtype):
                sdc, sdf = ({k: v.to(dtype).to(dev) for k, v in sd.items()} for sd in tsd)
                tv = torch.linspace(0., 1., N_SAMPLES, dtype=dtype).to(dev)
                uu = torch.linspace(0., 1., N_IMPORTANCE, dtype=dtype).to(dev)
                parts = []
                with torch.no_grad():
                    for i in range(0, rays_dev.shape[0], 8192):
                        o = oracle.render_rays(rays_dev[i:i + 8192].to(dtype), sdc, sdf, pcfg, t_vals=tv, u=uu)
                        parts.append({k: o[k].cpu() for k in pkeys + ("acc_fine", "disp_fine")})
                return {k: torch.cat([q[k] for q in parts]) for k in parts[0]}

            t64, t32 = oracle_on_device(trays, torch.float64), oracle_on_device(trays, torch.float32)
            # the device's fp32 evaluation of the reference arithmetic against the HOST's (== the reference's own kernels) on a subset
            sub = torch.arange(0, trays.shape[0], 16)
            with torch.no_grad():
                h32 = oracle.render_rays(trays[sub.to(dev)].cpu(), tsd[0], tsd[1], pcfg)
            tstats, tverd, frac = {}, {}, {}
            for fk, ok in map_pairs:
                hip = tmaps[fk].reshape(H * W, -1)[tsel].cpu().numpy().reshape(t32[ok].shape)
                tstats[fk] = stagewise.psnr_delta_db(hip, t32[ok].numpy(), t64[ok].numpy(), detail=True, n_targets=16)
                tverd[fk] = psnr_gate("trained network, " + fk, tstats[fk])
                frac[fk] = float((np.abs(hip - t32[ok].numpy()) <= ATOL + RTOL * np.abs(t32[ok].numpy())).all(-1).mean()) if hip.ndim > 1 else \
                    float((np.abs(hip - t32[ok].numpy()) <= ATOL + RTOL * np.abs(t32[ok].numpy())).mean())
            dev_host = {ok: float((t32[ok][sub] - h32[ok]).abs().max()) for _, ok in map_pairs}
            acc_t = tmaps["acc_map"].reshape(-1)[tsel]
            parity["trained"] = {
                "weights": "tests/golden/trained_object_chair.npz (scripts/fit_synthetic.py: 3000 steps through the product's training path)",
                "frame": f"{H}x{W} held-out view ({n_total} rays) through object_level.render, one frame {t_frame * 1e3:.1f} ms = {n_total / t_frame:.0f} rays/s",
                "rays_judged": int(len(tsel)), "acc_quantiles": [float(torch.quantile(acc_t, q)) for q in (0.0, 0.1, 0.5, 0.9, 1.0)],
                "psnr_delta_db_per_map": tstats, "psnr_verdicts": tverd,
                "fraction_of_rays_within_the_plain_tolerance": frac,
                "device_fp32_oracle_vs_host_fp32_oracle_max_abs": dev_host, "host_subset_rays": int(len(sub)),
                "seconds": time.perf_counter() - t_tr,
                "note": "delta = PSNR(HIP, T) - PSNR(fp32 oracle, T), T = fp64 oracle + the fixed 30 dB perturbation, on every "
                        f"{n_total // len(tsel)}th ray of the frame; both oracle runs are the reference arithmetic evaluated by torch on the "
                        "GPU (fp64 / fp32; the host's fp32 run - the reference's own CPU kernels - on every 16th of those rays differs from "
                        "the device's by device_fp32_oracle_vs_host_fp32_oracle_max_abs); every map gated at the plain 1e-4 dB budget"}
            del tmaps, tc, tf

    if rank == 0:
        json_out.write(json.dumps({
            **head,
            "value_reference_chunking": None if ref_chunking is None else ref_chunking["value"], "reference_chunking": ref_chunking,
            "roofline": roofline, "strict_fp32": strict, "roofline_f32_kernel": roofline_f32, "exact_f32_path": exact, "parity": parity,
            "configs": configs, "frame_costs": frame_costs, "f16_range_fallback": fallback, "train_step": train, "cpu_baseline": cpu}) + "\n")
        json_out.flush()
    n_bad = len(problems)
    if world > 1:
        # every rank learns rank 0's verdict and all leave together, with the same exit code (round 3: a parity failure made rank 0
        # skip a barrier the others were in - a collective-watchdog timeout instead of the message below).  Host-side group: the
        # idle ranks sleep here while rank 0 is in the CPU oracle.
        verdict = torch.tensor([n_bad], dtype=torch.int64)
        dist.broadcast(verdict, 0, group=side)
        n_bad = int(verdict.item())
        dist.destroy_process_group()
    if problems:
        raise SystemExit("bench.py: the timed frame does NOT match the oracle:\n" + "\n".join(problems))
    if n_bad:
        raise SystemExit(f"bench.py: rank 0 reports {n_bad} parity violation(s) of the timed frame")


if __name__ == "__main__":
    main()
