"""Training draws: the stratified jitter, the density noise of both passes and the inverse-CDF variates of a training-mode render,
drawn inside the HIP kernels (csrc/draws.h; include/inerf.h, "Training draws") instead of by ``torch.rand`` / ``torch.randn``.

A sample's draw is a pure function of ``(seed, step, stream, global ray index, sample index)``: a batch renders to the same bits
for any ``chunk``, the backward of the compositing regenerates its noise from the step it saw, and a captured training step draws
anew at every replay because the step counter lives on the device.  Opt-in: pass a ``DrawState`` as ``draws=`` to
``object_level.render`` / ``render_rays`` or set ``SSRRenderMixin.draws``.  torch's own random streams are not reproduced.
"""
import torch

from . import _capi, kernels

JITTER, NOISE_COARSE, U, NOISE_FINE = (_capi.DRAW_STREAM_JITTER, _capi.DRAW_STREAM_NOISE_COARSE, _capi.DRAW_STREAM_U,
                                       _capi.DRAW_STREAM_NOISE_FINE)


class DrawState:
    """Seed and device-resident step counter of the training draws.

    ``args()`` gives the ``inerf_draw_args`` of one launch, ``advance()`` moves to the next step (one launch, capturable; the
    front-ends call it once per top-level render call, after the last chunk), ``snapshot()`` freezes the current step for a
    backward pass, ``fill()`` materialises a stream as the tensor the classic entry points take."""

    def __init__(self, seed, device, step=0):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"DrawState on {device}: intrinsicnerf_amd runs only on a HIP device (no CPU / eager fallback exists)")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = device
        self.step_dev = torch.tensor([int(step)], dtype=torch.int64, device=device)

    def args(self, ray_base=0, noise_std=0., perturb=False, fine=False, step_dev=None):
        """``inerf_draw_args`` reading the step from the device counter (or from ``step_dev``, a ``snapshot()``)."""
        t = self.step_dev if step_dev is None else step_dev
        a = _capi.DrawArgs(self.seed, 0, t.data_ptr(), int(ray_base), float(noise_std),
                           (_capi.DRAW_PERTURB if perturb else 0) | (_capi.DRAW_FINE if fine else 0))
        a.step_tensor = t          # keeps the counter alive; kernels.freeze_draw copies it for a backward node
        return a

    def advance(self):
        """step += 1 on the device (its own one-workgroup launch on the current stream)."""
        kernels.draw_advance(self.step_dev)

    def snapshot(self):
        """An 8-byte device copy of the current step: what a backward node passes as ``step_dev``, so that it sees the forward's
        step even after ``advance()``.  Capturable."""
        return self.step_dev.clone()

    def fill(self, stream, n_rays, n, ray_base=0, noise_std=1.):
        """Stream ``stream`` (0 jitter, 1 coarse noise, 2 u, 3 fine noise) as a ``[n_rays, n]`` tensor; the noise streams scaled
        by ``noise_std``."""
        return kernels.draw_fill(self.args(ray_base, noise_std), stream, n_rays, n, self.device)

    def state_dict(self):
        """Seed and step (one host read of the counter - not for use inside a captured step)."""
        return {"seed": self.seed, "step": int(self.step_dev.item())}

    def load_state_dict(self, state):
        self.seed = int(state["seed"]) & 0xFFFFFFFFFFFFFFFF
        self.step_dev.copy_(torch.tensor([int(state["step"])], dtype=torch.int64))
