"""``optimizer.step()`` of both reference trainers on the library's own launch (csrc/adam.hip, ``inerf_adam_step``).

``Adam`` stands where the trainers build ``torch.optim.Adam(params=grad_vars, lr=..., betas=(0.9, 0.999))`` (run_nerf.py:304,
trainer.py:842): same constructor keywords, same per-parameter state (``step``, ``exp_avg``, ``exp_avg_sq``), and a
``state_dict()`` that reads as an eager ``torch.optim.Adam`` wrote it, so the reference's checkpoints (run_nerf.py:1041,
trainer.py:1046) load into this class and this class's into torch's.  ``--inerf-adam`` of ``intrinsicnerf_amd.launch`` puts it
in place of the optimizer ``create_nerf`` / ``create_ssr`` built.

One call of the library per parameter group updates every tensor of the group that has a gradient: the arithmetic is torch's
eager single-tensor form with the three per-tensor scalars formed in fp64 (on the device, from the tensor's own step count),
and it is the SAME arithmetic launched directly and replayed from a ``graphs.GraphedTrainStep`` - torch's eager and
``capturable`` forms differ from each other there.  The learning rate is taken in fp32 in both modes (a float in the group,
or the 0-dim device tensor ``GraphedTrainStep`` puts there).

While the optimizer steps, every ``state[p]["step"]`` is a 0-dim fp32 tensor on the parameter's device (torch's capturable
layout: the kernel advances it); ``state_dict()`` hands host copies out, and a loaded state whose counts are on the host is
moved over by the next ``step()``.  There is no CPU path: parameters that are not fp32 on a HIP device raise at ``step()``.
"""
import ctypes as C

import torch

from . import _capi


class _Table:
    """The argument block of one group's call and everything that keeps its pointers alive."""

    def __init__(self, live, key):
        n = len(live)
        self.key = key
        self.params = [p for p, _, _ in live]
        self.keep = [(g, st["step"], st["exp_avg"], st["exp_avg_sq"]) for _, g, st in live]
        self.device = self.params[0].device
        ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        self.arrays = [ptrs(self.params), ptrs([k[0] for k in self.keep]), ptrs([k[2] for k in self.keep]),
                       ptrs([k[3] for k in self.keep]), ptrs([k[1] for k in self.keep]),
                       (C.c_int64 * n)(*[p.numel() for p in self.params])]
        a = self.args = _capi.AdamArgs()
        a.n_tensors = n
        a.params, a.grads, a.exp_avg, a.exp_avg_sq, a.steps, a.counts = (C.cast(x, C.c_void_p) for x in self.arrays)
        self.ref = C.byref(a)


def _key(live):
    # addresses of parameter and gradient (zero_grad(set_to_none=True) reallocates gradients; `p.data = ...` moves a parameter),
    # identity of the state tensors (load_state_dict and GraphedTrainStep replace them; the table holds the old ones alive, so
    # an id cannot be reused while it is compared)
    return [x for p, g, st in live for x in (p.data_ptr(), g.data_ptr(), id(st.get("step")), id(st.get("exp_avg")), id(st.get("exp_avg_sq")))]


class Adam(torch.optim.Optimizer):
    """``Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)`` - torch.optim.Adam's update as one HIP launch per group.

    ``weight_decay``, ``amsgrad`` and ``maximize`` are accepted so that a call written for torch.optim.Adam reads the same,
    and raise ``ValueError`` unless they are off: neither trainer uses them and the kernel does not implement them."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
        if weight_decay != 0:
            raise ValueError(f"weight_decay={weight_decay!r} is not supported by intrinsicnerf_amd.optim.Adam (the trainers use 0)")
        if amsgrad:
            raise ValueError("amsgrad=True is not supported by intrinsicnerf_amd.optim.Adam")
        if maximize:
            raise ValueError("maximize=True is not supported by intrinsicnerf_amd.optim.Adam")
        # torch's own constructor checks lr / betas / eps and names the group keys of THIS torch version: a state_dict of this
        # class then has exactly the param_groups entries an eager torch.optim.Adam writes
        probe = torch.optim.Adam([torch.zeros(1)], lr=float(lr) if isinstance(lr, torch.Tensor) else lr, betas=betas, eps=eps)
        defaults = dict(probe.defaults)
        defaults["lr"] = lr
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not eps > 0.0:
            raise ValueError(f"betas={betas!r}, eps={eps!r}: the kernel takes betas in [0, 1) and eps > 0")
        super().__init__(params, defaults)
        self._tables = {}

    # ---- state ----
    def _check_group(self, group):
        if group.get("weight_decay", 0) != 0:
            raise ValueError("weight_decay != 0 is not supported by intrinsicnerf_amd.optim.Adam")
        for name in ("amsgrad", "maximize"):
            if group.get(name, False):
                raise ValueError(f"{name}=True is not supported by intrinsicnerf_amd.optim.Adam")

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        self._tables = {}

    def state_dict(self):
        """As an eager ``torch.optim.Adam`` writes it: float learning rates, ``capturable: False``, step counts as 0-dim fp32
        tensors on the host (one transfer for all of them).  Moments are the live tensors, as in torch."""
        sd = super().state_dict()
        groups = []
        for g in sd["param_groups"]:
            g = dict(g)
            if isinstance(g.get("lr"), torch.Tensor):
                g["lr"] = float(g["lr"].item())
            g["capturable"] = False
            groups.append(g)
        on_device = [(k, st["step"]) for k, st in sd["state"].items() if isinstance(st.get("step"), torch.Tensor) and st["step"].device.type != "cpu"]
        host = {}
        if on_device:
            flat = torch.stack([s.detach().reshape(()).float() for _, s in on_device]).cpu()
            host = {k: flat[i].clone() for i, (k, _) in enumerate(on_device)}
        state = {k: {n: (host[k] if n == "step" and k in host else v) for n, v in st.items()} for k, st in sd["state"].items()}
        return {"state": state, "param_groups": groups}

    # ---- the step ----
    def _prepare(self, p, g, st):
        """Bring one parameter's state into the form the kernel reads (called when the table is rebuilt, never per step)."""
        if not p.is_cuda:
            raise RuntimeError(f"a parameter lives on {p.device}: intrinsicnerf_amd runs only on a HIP device (no CPU / eager fallback exists)")
        if p.dtype != torch.float32 or g.dtype != torch.float32:
            raise ValueError(f"parameters and gradients must be float32, got {p.dtype} / {g.dtype}")
        if g.is_sparse or g.device != p.device or g.shape != p.shape:
            raise ValueError("a gradient must be a dense tensor of its parameter's shape on its parameter's device")
        if not p.is_contiguous() or not g.is_contiguous():
            raise ValueError("parameters and gradients must be contiguous")
        capturing = torch.cuda.is_current_stream_capturing()
        if "exp_avg" not in st:
            if capturing:
                raise RuntimeError("optimizer state would be created during graph capture: take one eager step first (GraphedTrainStep's warm-up does)")
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            return
        step = st["step"]
        if not isinstance(step, torch.Tensor) or step.device != p.device or step.dtype != torch.float32 or step.dim() != 0:
            if capturing:
                raise RuntimeError("a step count is not on the device during graph capture")
            st["step"] = torch.as_tensor(step, dtype=torch.float32).reshape(()).to(p.device).clone()
        for name in ("exp_avg", "exp_avg_sq"):
            t = st[name]
            if t.device != p.device or t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous():
                if capturing:
                    raise RuntimeError(f"{name} is not a contiguous float32 tensor on the device during graph capture")
                st[name] = t.to(p.device, torch.float32).reshape(p.shape).contiguous()

    def _group_table(self, index, group):
        live = []
        for p in group["params"]:
            g = p.grad
            if g is not None:                              # no gradient: step count, moments and value stay as they are
                live.append((p, g, self.state[p]))
        if not live:
            return None
        table = self._tables.get(index)
        if table is None or table.key != _key(live):
            self._check_group(group)
            for p, g, st in live:
                self._prepare(p, g, st)
            if len({p.device for p, _, _ in live}) != 1:
                raise ValueError("the parameters of one group must live on one device")
            table = self._tables[index] = _Table(live, _key(live))
        return table

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _capi.lib()
        for index, group in enumerate(self.param_groups):
            table = self._group_table(index, group)
            if table is None:
                continue
            a, lr = table.args, group["lr"]
            if isinstance(lr, torch.Tensor):
                if lr.device != table.device or lr.dtype != torch.float32 or lr.numel() != 1:
                    raise ValueError("a tensor learning rate must be one float32 on the parameters' device")
                table.lr = lr                              # (kept alive with the table)
                a.lr, a.lr_dev = 0.0, lr.data_ptr()
            else:
                a.lr, a.lr_dev = float(lr), None
            a.beta1, a.beta2 = group["betas"]
            a.eps = group["eps"]
            with torch.cuda.device(table.device):
                stream = C.c_void_p(torch.cuda.current_stream(table.device).cuda_stream)
                _capi.check(lib.inerf_adam_step(table.ref, stream), "inerf_adam_step")
            # in-place through the raw pointers: tell autograd (saved-tensor checks) and packing.packed_for_module's cache key
            torch.autograd.graph.increment_version(table.params)
        return loss


def from_torch(optimizer):
    """``Adam`` over the parameter groups of a ``torch.optim.Adam`` - same ``lr / betas / eps`` per group, its state (moments and
    step counts, e.g. loaded from a checkpoint) carried over.  What ``--inerf-adam`` does to the optimizer the reference's
    ``create_nerf`` / ``create_ssr`` built; an ``Adam`` of this module is returned as it is."""
    if isinstance(optimizer, Adam):
        return optimizer
    if not isinstance(optimizer, torch.optim.Adam):
        raise TypeError(f"expected a torch.optim.Adam, got {type(optimizer).__name__}")
    keys = ("params", "lr", "betas", "eps", "weight_decay", "amsgrad", "maximize")
    groups = [{k: g[k] for k in keys if k in g} for g in optimizer.param_groups]
    for g in groups:                                       # (named here: the constructor takes group options as they are)
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("weight_decay / amsgrad / maximize are not supported by intrinsicnerf_amd.optim.Adam")
    new = Adam(groups)
    new.load_state_dict(optimizer.state_dict())
    return new
