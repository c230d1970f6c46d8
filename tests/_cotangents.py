"""Cotangents (d loss / d raw) over the range a trained scene gives the network backward (csrc/mlp_bwd.hip, csrc/mlp_wgrad.hip):
uniform power-of-two scalings, eight magnitude groups interleaved inside every 64-point tile, and an opaque ray's density column.
Everything is built on the CPU (torch's CPU kernels keep fp32 denormals; a copy to the device keeps the bits) - plain helpers,
checked by tests/test_cotangents_cpu.py and used by tests/test_backward_range_gpu.py."""
import torch

TILE = 64                                    # points per tile of the chain (csrc/layout.h kTilePoints)
F32_MIN_NORMAL = 2.0 ** -126
F32_MIN_DENORMAL = 2.0 ** -149

# the uniform sweep: c0 * 2^k
SWEEP_LOG2 = (-120, -100, -60, -20, 0, 20, 60, 100)

# group of a point = point index mod 8, so every tile holds every group
GROUPS = 8
GROUP_NAMES = ("2^-140", "2^-130", "2^-120", "2^-40", "1", "2^30", "zero", "sigma only, 2^-10")
GROUP_LOG2 = (-140, -130, -120, -40, 0, 30, None, -10)
DENORMAL_GROUPS = (0, 1)                     # every entry below fp32's smallest normal; group 1 sits below the 2^-128 edge
ZERO_GROUP = 6
SIGMA_GROUP = 7                              # channel 3 only (sigma has no activation inside the network)
ACCURATE_GROUPS = (2, 3, 4, 5, 7)            # neither denormal nor zero: judged against fp64 on their own
SIGMA_CHANNEL = 3


def base_cotangent(n_points, channels, seed):
    """c0: fp64 standard normal [n_points, channels], every channel live."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n_points, channels, generator=g, dtype=torch.float64)


def scaled(c0, log2):
    """(c0 * 2^log2) as fp32.  Exact (a change of exponent) wherever the result is a normal fp32 number."""
    return (c0.double() * 2.0 ** log2).float()


def group_index(n_points, live=None):
    """Group of every point (index mod 8); -1 for the points ``live`` (bool [n_points]) leaves out - the ReLU ties, which get
    no cotangent and so belong to no group."""
    idx = torch.arange(n_points) % GROUPS
    if live is not None:
        idx = torch.where(live.reshape(-1).cpu(), idx, torch.full_like(idx, -1))
    return idx


def tiles_hold_every_group(groups):
    """True when every 64-point tile (the last, ragged one too) holds at least one point of each of the eight groups."""
    n = groups.numel()
    for t0 in range(0, n, TILE):
        if set(range(GROUPS)) - set(groups[t0:t0 + TILE].tolist()):
            return False
    return True


def grouped_cotangent(c0, groups, only=None):
    """fp32 [n_points, channels]: c0 scaled group by group (GROUP_LOG2); points of group -1 and of the zero group get 0; the sigma
    group keeps channel 3 only.  ``only``: a group number - every other group's points are zeroed (the isolated runs)."""
    out = torch.zeros(c0.shape, dtype=torch.float32)
    for g in range(GROUPS):
        if g == ZERO_GROUP or (only is not None and g != only):
            continue
        rows = groups == g
        part = scaled(c0[rows], GROUP_LOG2[g])
        if g == SIGMA_GROUP:
            keep = torch.zeros_like(part)
            keep[:, SIGMA_CHANNEL] = part[:, SIGMA_CHANNEL]
            part = keep
        out[rows] = part
    return out


def is_denormal(x):
    """Elementwise: a non-zero fp32 value below the smallest normal."""
    a = x.abs()
    return (a > 0) & (a < F32_MIN_NORMAL)


def scaling_stays_normal(want64, log2):
    """The precondition of the bit-for-bit scaling check, from the fp64 reference gradients ``want64`` (dict of tensors) of c0:
    scaled by 2^log2 and cast to fp32 no element overflows, and the elements that land below fp32's normal range carry less
    than 1e-6 of their tensor's norm."""
    for w in want64.values():
        w = w.double() * 2.0 ** log2
        if not bool(torch.isfinite(w.float()).all()):
            return False
        small = w.abs() < F32_MIN_NORMAL
        if float((w * small).norm()) >= 1e-6 * float(w.norm()):
            return False
    return True


def opaque_sigma(z, rays_d, first=20):
    """Density column [n, s] (fp32) of rays that meet an opaque surface at sample ``first``: 0 in front of it, then
    sigma * delta = 1 per sample (delta = the sample spacing times |rays_d|, as raw2outputs forms it), so the transmittance
    falls by e per sample - through fp32's denormal window about 88 samples later, then to exact 0."""
    delta = (z[:, 1:] - z[:, :-1]) * rays_d.norm(dim=-1, keepdim=True)
    delta = torch.cat([delta, delta[:, -1:]], -1)
    sigma = 1.0 / delta.clamp_min(1e-6)
    sigma[:, :first] = 0.0
    return sigma.float()


def magnitude_classes(x64):
    """Shares of the entries of an fp64 tensor that, as fp32, are denormal (2^-149 <= |x| < 2^-126) and that are exact or
    underflowed zeros (|x| < 2^-150: below half the smallest denormal)."""
    a = x64.double().abs()
    n = float(a.numel())
    return float(((a >= F32_MIN_DENORMAL) & (a < F32_MIN_NORMAL)).sum()) / n, float((a < F32_MIN_DENORMAL / 2).sum()) / n


def head_gradient_max(raw, d_raw, n_classes=0, endpoint_dim=0):
    """m = max |pre-activation gradient of a head| per point, in fp64, by the formula of head_gradients (csrc/mlp_bwd.hip):
    rgb = albedo * shading + residual through the sigmoids' derivatives, sigma as it is, the semantic logits and the endpoint
    feature as they are.  raw / d_raw: [n_points, channels]."""
    r, g = raw.double(), d_raw.double()
    sh = r[:, 7:8]
    a, rs = r[:, 4:7], r[:, 8:11]
    d_albedo = (g[:, 0:3] * sh + g[:, 4:7]) * (a * (1 - a))
    d_shading = (g[:, 7:8] + (g[:, 0:3] * a).sum(1, keepdim=True)) * (sh * (1 - sh))
    d_res = (g[:, 0:3] + g[:, 8:11]) * (rs * (1 - rs))
    parts = [d_albedo, d_shading, d_res, g[:, 3:4]]
    if n_classes:
        parts.append(g[:, 11:11 + n_classes])
    if endpoint_dim:
        parts.append(g[:, g.shape[1] - endpoint_dim:])
    return torch.cat(parts, 1).abs().amax(1)
