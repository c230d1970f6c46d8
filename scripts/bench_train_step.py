#!/usr/bin/env python3
"""Training-step timing through the object-level front-end (staged path: HIP sampling / compositing with HIP backward,
network layers through torch autograd) and the compositing kernels' HBM rates.

    python scripts/bench_train_step.py [--rays 2048] [--iters 10] [--ssr C] [--loss intrinsic] [--optimizer inerf] [--batch inerf]
``--loss intrinsic`` times the step with the loss the reference trains with (compute_intrinsic_loss on both levels, image and
cluster MSE, the SSR cross-entropy) instead of the default stand-in loss - once as torch expressions (scripts/torch_losses.py)
and once on the two launches of csrc/losses.hip, alternating in the same process.
``--optimizer inerf`` (with ``--loss intrinsic``) adds a third step to that alternation: the HIP loss with ``optim.Adam``
(csrc/adam.hip) in place of torch.optim.Adam over the same parameters - the step next to it is its parent figure on the same box.
``--draws kernel`` (with ``--loss intrinsic``) adds the last step of that alternation once more with the random tensors of the render
(jitter, inverse-CDF variates, density noise) drawn inside the kernels (``draws.DrawState``, csrc/draws.h) instead of by torch's
generator - the step next to it is its parent figure - and, with ``--graph``, both of them as HIP graphs (graphs.GraphedTrainStep).
``--count-launches`` prints the number of device kernels one step of each kind launches (torch.profiler).
``--batch inerf`` times the whole object-level step with its batch assembled per iteration - once by the trainer's host + torch
expressions (scripts/torch_batches.py: image upload, whole-frame rays, host permutation, gathers) and once by
``batches.ObjectBatcher.next()`` (csrc/batch.hip) - alternating in the same process; 100 images of 400 x 400 (``--frame``).
The batch is the reference's: N_rand = 1024 rays plus one neighbour each (run_nerf.py:918-929), 64 + 128 samples.
"""
import argparse
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

__graft_entry__.build()
from intrinsicnerf_amd import kernels, object_level as ol  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=2048)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--ssr", type=int, default=-1, help="C >= 0: the SSR network with C classes through ssr.SSRRenderer instead")
ap.add_argument("--loss", choices=("mse", "intrinsic"), default="mse", help="intrinsic: the reference's full loss, as torch expressions and in HIP")
ap.add_argument("--optimizer", choices=("torch", "inerf"), default="torch", help="inerf: also time the step with optim.Adam (needs --loss intrinsic)")
ap.add_argument("--batch", choices=("fixed", "inerf"), default="fixed", help="inerf: assemble the batch every step, reference expressions against batches.ObjectBatcher")
ap.add_argument("--frame", type=int, default=400, help="frame size of --batch inerf")
ap.add_argument("--draws", choices=("torch", "kernel"), default="torch", help="kernel: also time the step with the render's random tensors drawn in the kernels (needs --loss intrinsic)")
ap.add_argument("--graph", action="store_true", help="with --draws kernel: also time both steps as HIP graphs")
ap.add_argument("--count-launches", action="store_true", help="print the device kernels per step of every timed kind")
a = ap.parse_args()
if a.draws == "kernel" and a.loss != "intrinsic":
    raise SystemExit("--draws kernel is timed next to torch's generator inside the --loss intrinsic alternation")
if a.graph and a.draws != "kernel":
    raise SystemExit("--graph times the graphed steps of --draws kernel")
if a.optimizer == "inerf" and a.loss != "intrinsic":
    raise SystemExit("--optimizer inerf is timed next to torch.optim.Adam inside the --loss intrinsic alternation")
if a.batch == "inerf" and (a.ssr >= 0 or a.loss != "mse" or a.optimizer != "torch"):
    raise SystemExit("--batch inerf times the object-level step with the stand-in loss and torch.optim.Adam: not with --ssr, --loss intrinsic or --optimizer inerf")
LOSS_WEIGHTS = {"image": 1.0, "chroma": 1.0, "sparsity": 0.01, "far": 0.01, "shading": 1.0, "residual": 1.0, "intensity": 0.1, "cluster": 1.0,
                "semantic": 0.04}


def time_both(steps, iters, what, label="intrinsic loss as"):
    """``steps``: {name: step function}; warms every one up, then times them in alternating rounds and prints the medians."""
    import statistics
    for fn in steps.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in steps}
    for _ in range(5):
        for k, fn in steps.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) / iters * 1e3)
    for k, v in times.items():
        print(f"{what}, {label} {k}: {statistics.median(v):.2f} ms per step (rounds: {', '.join(f'{x:.2f}' for x in v)})")
    if a.count_launches:
        from torch.profiler import ProfilerActivity, profile
        for k, fn in steps.items():
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            kernels_seen = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                            and "memset" not in e.name.lower()]
            print(f"{what}, {label} {k}: {len(kernels_seen)} device kernels per step")


def add_draws_steps(steps, make_step, make_opt, example_inputs, dev):
    """--draws kernel: the last step of ``steps`` again with a DrawState; --graph: that step and its parent as HIP graphs.
    ``make_step(draws)`` -> (loss_fn(*inputs) that renders with ``draws`` and returns the loss, eager step function using ``opt``)."""
    from intrinsicnerf_amd import draws, graphs
    base = list(steps)[-1]
    state = draws.DrawState(torch.initial_seed(), dev)
    steps[base + " + kernel draws"] = make_step(state, make_opt())[1]
    if a.graph:
        for name, st in ((base + ", graphed", None), (base + " + kernel draws, graphed", draws.DrawState(torch.initial_seed(), dev))):
            opt_g = make_opt()
            g = graphs.GraphedTrainStep(make_step(st, opt_g)[0], example_inputs, opt_g, draws=st)
            steps[name] = (lambda g=g: g(*example_inputs))


dev = torch.device("cuda:0")
torch.manual_seed(0)
if a.ssr >= 0:          # trainer.py:876-991: 1024 rays (512 + neighbours), depth range [0.1, 10], semantic cross-entropy + photometric loss
    from intrinsicnerf_amd import ssr
    n = a.rays
    r = ssr.SSRRenderer(a.ssr, white_bkgd=False, endpoint_feat=False, device=dev)
    r.training, r.check_numerics = True, False
    opt = torch.optim.Adam(list(r.ssr_net_coarse.parameters()) + list(r.ssr_net_fine.parameters()), lr=5e-4)
    o = torch.tensor([[0.5, 0.2, 0.1]]).expand(n, 3)
    d = torch.randn(n, 3); d = d / d.norm(dim=-1, keepdim=True)
    rays = torch.cat([o, d, 0.1 * torch.ones(n, 1), 10 * torch.ones(n, 1), d], -1).to(dev)
    target = torch.rand(n, 3, device=dev)
    labels = torch.randint(0, max(a.ssr, 1), (n,), device=dev)

    def sstep():
        ret = r.render_rays(rays)
        loss = ((ret["rgb_fine"] - target) ** 2).mean() + ((ret["rgb_coarse"] - target) ** 2).mean()
        if a.ssr > 0:
            loss = loss + 0.04 * torch.nn.functional.cross_entropy(ret["sem_logits_fine"], labels) \
                + 0.04 * torch.nn.functional.cross_entropy(ret["sem_logits_coarse"], labels)
        opt.zero_grad(); loss.backward(); opt.step()

    if a.loss == "intrinsic":
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import torch_losses
        cluster_target = torch.rand(n, 3, device=dev)
        target[n // 2:] = (target[:n // 2] + 0.02).clamp(0, 1)          # neighbours: similar colours, as the reference's batches
        labels = torch.randint(0, a.ssr + 1, (n,), device=dev)            # unshifted: 0 = void

        def istep(hip, opt=opt):
            ret = r.render_rays(rays)
            if hip:
                loss = ssr.ssr_step_loss(ret, target, labels, LOSS_WEIGHTS, cluster_target, semantic=a.ssr > 0)[0]
            else:
                levels = [{k: ret[k + t] for k in ("albedo", "shading", "residual", "rgb")} for t in ("_coarse", "_fine")]
                if a.ssr > 0:
                    levels[0]["logits"], levels[1]["logits"] = ret["sem_logits_coarse"], ret["sem_logits_fine"]
                loss = torch_losses.step_loss(levels, target, labels, LOSS_WEIGHTS, cluster_target, semantic=a.ssr > 0)
            opt.zero_grad(); loss.backward(); opt.step()

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            steps = {"torch expressions": lambda: istep(False), "HIP launches": lambda: istep(True)}
            if a.optimizer == "inerf":
                from intrinsicnerf_amd import optim
                opt_inerf = optim.Adam(list(r.ssr_net_coarse.parameters()) + list(r.ssr_net_fine.parameters()), lr=5e-4)
                steps["HIP launches + optim.Adam"] = lambda: istep(True, opt_inerf)
            if a.draws == "kernel":
                def make_opt():
                    params = list(r.ssr_net_coarse.parameters()) + list(r.ssr_net_fine.parameters())
                    if a.optimizer == "inerf":
                        from intrinsicnerf_amd import optim
                        return optim.Adam(params, lr=5e-4)
                    return torch.optim.Adam(params, lr=5e-4, capturable=a.graph)

                def make_step(state, opt_d):
                    def loss_fn(rb, tg):
                        r.draws = state
                        try:
                            ret = r.render_rays(rb)
                        finally:
                            r.draws = None
                        return ssr.ssr_step_loss(ret, tg, labels, LOSS_WEIGHTS, cluster_target, semantic=a.ssr > 0)[0]

                    def eager():
                        loss = loss_fn(rays, target)
                        opt_d.zero_grad(); loss.backward(); opt_d.step()
                    return loss_fn, eager
                add_draws_steps(steps, make_step, make_opt, (rays, target), dev)
            time_both(steps, a.iters,
                      f"SSR training step (C = {a.ssr}), {n} rays x (64+128) samples")
        sys.exit(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(10):
            sstep()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.iters):
            sstep()
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / a.iters
    print(f"SSR training step (C = {a.ssr}): {n} rays x (64+128) samples: {dt * 1e3:.1f} ms -> {n / dt:.0f} rays/s "
          f"[{os.environ.get('INERF_TRAIN_MLP', 'hip')} network backward]")
    sys.exit(0)
embed, ch = ol.get_embedder(10, 0); embed_d, ch_d = ol.get_embedder(4, 0)
mk = lambda: ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
net_c, net_f = mk(), mk()
opt = torch.optim.Adam(list(net_c.parameters()) + list(net_f.parameters()), lr=5e-4)
n = a.rays
o = torch.tensor([[2.5, 1.5, 2.0]]).expand(n, 3)
d = -o / o.norm(dim=-1, keepdim=True) + 0.2 * torch.randn(n, 3)
rays = torch.cat([o, d, 2 * torch.ones(n, 1), 6 * torch.ones(n, 1), d / d.norm(dim=-1, keepdim=True)], -1).to(dev)
target = torch.rand(n, 3, device=dev)
q = ol.NetworkQuery(embed, embed_d)


def step():
    ret = ol.render_rays(rays, net_c, q, 64, retraw=True, perturb=1.0, N_importance=128, network_fine=net_f, white_bkgd=True,
                         raw_noise_std=0.0)
    loss = ((ret["rgb_map"] - target) ** 2).mean() + ((ret["rgb0"] - target) ** 2).mean() \
        + 0.01 * ret["albedo_map"].abs().mean() + 0.01 * (ret["shading_map"] - 0.5).pow(2).mean() + 0.01 * ret["residual_map"].abs().mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss.detach()) if False else loss


if a.batch == "inerf":
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch_batches
    from intrinsicnerf_amd import batches
    rng = np.random.RandomState(0)
    size, n_img = a.frame, 100
    images = rng.rand(n_img, size, size, 3).astype(np.float32)
    masks = (rng.rand(n_img, size, size, 1) > 0.3).astype(np.float32)
    poses = np.tile(np.eye(4, dtype=np.float32), (n_img, 1, 1))
    poses[:, :3, 3] = np.array([2.5, 1.5, 2.0], dtype=np.float32) + 0.1 * rng.randn(n_img, 3).astype(np.float32)
    focal = 0.5 * size / np.tan(0.5 * 0.6911112070083618)
    K = np.array([[focal, 0, 0.5 * size], [0, focal, 0.5 * size], [0, 0, 1]])
    batcher = batches.ObjectBatcher(images, masks, poses, K, np.arange(n_img), n // 2, device=dev)
    it = [0]

    def from_reference():
        it[0] += 1
        return torch_batches.object_batch(it[0], images, masks, poses, K, np.arange(n_img), n // 2, 0, 0.5, dev)

    def fed_step(get):
        (rays_o, rays_d), target_s, target_m = get()                       # render()'s assembly of the batch (run_nerf.py:99-128)
        viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
        batch = torch.cat([rays_o, rays_d, 2 * torch.ones_like(rays_d[:, :1]), 6 * torch.ones_like(rays_d[:, :1]), viewdirs], -1)
        ret = ol.render_rays(batch, net_c, q, 64, retraw=True, perturb=1.0, N_importance=128, network_fine=net_f, white_bkgd=True,
                             raw_noise_std=0.0)
        loss = (((ret["rgb_map"] - target_s) ** 2) * target_m).mean() + ((ret["rgb0"] - target_s) ** 2).mean()
        opt.zero_grad(); loss.backward(); opt.step()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        time_both({"the reference's expressions": lambda: fed_step(from_reference), "batches.ObjectBatcher": lambda: fed_step(batcher.next)},
                  a.iters, f"training step (staged path), {n} rays x (64+128) samples, {size} x {size} frames", label="batch from")
    sys.exit(0)
if a.loss == "intrinsic":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch_losses
    mask = (torch.rand(n, 1, device=dev) > 0.2).float()               # target_m = images[..., -1:] (run_nerf.py:703)
    cluster_target = torch.rand(n, 3, device=dev)
    target[n // 2:] = (target[:n // 2] + 0.02).clamp(0, 1)

    def istep(hip, opt=opt):
        ret = ol.render_rays(rays, net_c, q, 64, retraw=True, perturb=1.0, N_importance=128, network_fine=net_f, white_bkgd=True,
                             raw_noise_std=0.0)
        if hip:
            loss = ol.object_step_loss(ret, target, mask, LOSS_WEIGHTS, cluster_target)[0]
        else:
            levels = [{"albedo": ret["albedo0"], "shading": ret["shading0"], "residual": ret["residual0"], "rgb": ret["rgb0"]},
                      {"albedo": ret["albedo_map"], "shading": ret["shading_map"], "residual": ret["residual_map"], "rgb": ret["rgb_map"]}]
            loss = torch_losses.step_loss(levels, target, mask, LOSS_WEIGHTS, cluster_target)
        opt.zero_grad(); loss.backward(); opt.step()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        steps = {"torch expressions": lambda: istep(False), "HIP launches": lambda: istep(True)}
        if a.optimizer == "inerf":
            from intrinsicnerf_amd import optim
            opt_inerf = optim.Adam(list(net_c.parameters()) + list(net_f.parameters()), lr=5e-4)
            steps["HIP launches + optim.Adam"] = lambda: istep(True, opt_inerf)
        if a.draws == "kernel":
            def make_opt():
                params = list(net_c.parameters()) + list(net_f.parameters())
                if a.optimizer == "inerf":
                    from intrinsicnerf_amd import optim
                    return optim.Adam(params, lr=5e-4)
                return torch.optim.Adam(params, lr=5e-4, capturable=a.graph)

            def make_step(state, opt_d):
                def loss_fn(rb, tg):
                    ret = ol.render_rays(rb, net_c, q, 64, retraw=True, perturb=1.0, N_importance=128, network_fine=net_f, white_bkgd=True,
                                         raw_noise_std=0.0, draws=state)
                    return ol.object_step_loss(ret, tg, mask, LOSS_WEIGHTS, cluster_target)[0]

                def eager():
                    loss = loss_fn(rays, target)
                    opt_d.zero_grad(); loss.backward(); opt_d.step()
                return loss_fn, eager
            add_draws_steps(steps, make_step, make_opt, (rays, target), dev)
        time_both(steps, a.iters,
                  f"training step (staged path), {n} rays x (64+128) samples")
    sys.exit(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for _ in range(10):          # the caching allocator needs a few steps to settle on the step's multi-GB blocks (3 warm-ups measured
        step()                   # 13.1 ms where the steady state is 11.4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.iters
print(f"training step (staged path): {n} rays x (64+128) samples: {dt * 1e3:.1f} ms -> {n / dt:.0f} rays/s")

# compositing kernels alone, fine-pass shape
s, chn = 192, 11
raw = torch.rand(n * 16, s, chn, device=dev)
z = torch.sort(torch.rand(n * 16, s, device=dev) * 4 + 2, -1)[0]
dd = torch.randn(n * 16, 3, device=dev)
grads = {k: torch.randn(n * 16, 3, device=dev) for k in ("rgb", "albedo", "residual")}
grads.update({k: torch.randn(n * 16, device=dev) for k in ("acc", "depth", "shading")})
# ... and with density noise: read from a tensor (the classic form) against regenerated in the kernel (draws.h: a Philox block per lane)
from intrinsicnerf_amd import draws as inerf_draws  # noqa: E402
state = inerf_draws.DrawState(1, dev)
noise = state.fill(inerf_draws.NOISE_FINE, n * 16, s)
drawn = state.args(0, 1.0, fine=True)
for name, fn, nbytes in (("k_composite", lambda: kernels.composite(raw, z, dd, None, True), raw.numel() * 4 + 2 * z.numel() * 4),
                         ("k_composite, noise tensor", lambda: kernels.composite(raw, z, dd, noise, True), raw.numel() * 4 + 3 * z.numel() * 4),
                         ("k_composite, drawn noise", lambda: kernels.composite(raw, z, dd, None, True, draw=drawn), raw.numel() * 4 + 2 * z.numel() * 4),
                         ("k_composite_bwd", lambda: kernels.composite_backward(raw, z, dd, grads, None, True), 2 * raw.numel() * 4 + z.numel() * 4),
                         ("k_composite_bwd, noise tensor", lambda: kernels.composite_backward(raw, z, dd, grads, noise, True), 2 * raw.numel() * 4 + 2 * z.numel() * 4),
                         ("k_composite_bwd, drawn noise", lambda: kernels.composite_backward(raw, z, dd, grads, None, True, draw=drawn), 2 * raw.numel() * 4 + z.numel() * 4)):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fn()
    e1.record(); e1.synchronize()
    ms = e0.elapsed_time(e1) / 20
    print(f"{name}: {n * 16} rays x {s} samples x {chn} ch: {ms:.3f} ms -> {nbytes / ms / 1e6:.0f} GB/s algorithmic")
