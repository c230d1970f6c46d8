"""Networks and rays that leave the f16 range at ONE chosen site of the f16x3 forward kernels, and the status words to expect.

A SITE is a place where a value is split into f16 halves as a GEMM operand: the position encoding, pts_linears.0 .. 7, feature_linear
(no ReLU: both signs count), views_linears.0, albedo_linear1, the shading hidden layer (``shading1``: test_linear1 of the object-level
network, shading_linear1 of SSR) and semantic_linear.0.0 (SSR).  The guard's limit is 6.0e4 on the scaled value, LIMIT = 7.5e3 on the
activation (kF16Safe / kActScale, csrc/mlp_f16_dev.h, csrc/layout.h).

``wire``: unit J of every 256-wide trunk layer is cut out of the ``sharp`` network of tests/_raw_rows.py (its column zeroed in every
consumer) and turned into a wire - pts_linears.0 row J reads encoding column 0 (the raw, divided coordinate) with weight 1 and bias
-X0, row J of every later layer reads unit J with weight 1 - which the site multiplies by ``gain`` into one unit whose own consumers
are zeroed; behind the site the wire is cut.  The site's activation is  gain * relu(u),  u = x / xyz_div - X0  per point, and nothing
else in the network sees it: the raw rows are those of the network without unit J.  Every wire weight is 1 (exact in every form).

``layout``: rays whose u runs from -1 at depth 2 to ``top_r`` at the last depth (exactly 6), top_r above T for the rays that are to
offend and below it for the others - the gap around T is MADE, not hoped for: a point whose fp64 u lies within 1.5 BAND of T is moved
to 2 BAND on its side, and the tests assert that none is left within BAND.  gain = LIMIT / T with T = 4 (gain 1875 <= 2^11: the other weights of the
site's GEMM keep their lo halves under the GEMM's power-of-two scale); the SSR encoder divides by 10, so its origins lie ten times as
far out.

The ENCODING site needs no wire: the rays of one group sit at |x / xyz_div| = 1.01 LIMIT (expected set), those of a second group at
0.99 LIMIT and ordinary rays (expected clear); the raw coordinate's own consumers (column 0 of pts_linears.0 and of the skip layer)
are zeroed so that the trunk stays far inside the range.  The direction encoding is bounded by 1 and has no case."""
import functools

import torch

import _forward_slots as fs
import _raw_rows as rr
from intrinsicnerf_amd import kernels

LIMIT = 7.5e3                    # kF16Safe / kActScale: the guard's limit on an (unscaled) activation
BAND = 0.01                      # no point's fp64 activation within 1 % of the limit on either side: ten times the largest relative
                                 # distance between what a form compares (a hi half towards zero: 2^-10; the probe's hi-only values:
                                 # 1e-3) and the exact value
OTHERS = 1.0 / 8                 # every other split value stays below this share of the limit
J = 200                          # the trunk unit that becomes the wire
K = 100                          # the unit of a 128-wide hidden layer a head site gains into
X0 = 0.5                         # the ramp starts at x / xyz_div = X0
T = 4.0                          # u at the limit: gain = LIMIT / T = 1875 <= 2^11
GAIN = LIMIT / T
TRUNK_SITES = tuple(f"pts_linears.{i}" for i in range(8))
HEAD_SITES = ("feature_linear", "views_linears.0", "albedo_linear1", "shading1")
ENCODING = "encoding"
SEMANTIC = "semantic_linear.0.0"
RELU_SITES = TRUNK_SITES + ("views_linears.0", "albedo_linear1", "shading1", SEMANTIC)


def sites(variant, classes):
    return (ENCODING,) + TRUNK_SITES + HEAD_SITES + ((SEMANTIC,) if variant == "ssr" and classes else ())


def layer_of(variant, site):
    """the state dict's name of a site's layer"""
    if site == "shading1":
        return "shading_linear1" if variant == "ssr" else "test_linear1"
    return site


def site_slot(site):
    """(slot of tests/_forward_slots.py, column) that holds the site's gained unit"""
    if site in TRUNK_SITES:
        return kernels.SAVE_H0 + int(site[-1]), J
    return {"feature_linear": (kernels.SAVE_FEAT, J), "views_linears.0": (kernels.SAVE_VH, K), "albedo_linear1": (kernels.SAVE_AS1H, K),
            "shading1": (kernels.SAVE_AS1H, 128 + K), SEMANTIC: (kernels.SAVE_SEMH, K)}[site]


# ---------------------------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------------------------
def _row(sd, layer, row, col=None, weight=0.0):
    """row ``row`` of ``layer`` reads column ``col`` alone, with ``weight`` and bias 0 (col None: nothing)"""
    sd[layer + ".weight"][row].zero_()
    sd[layer + ".bias"][row] = 0.0
    if col is not None:
        sd[layer + ".weight"][row, col] = weight


def wire(variant, classes, sd, site, gain):
    """``sd`` (changed in place and returned) with unit J cut out, wired from encoding column 0 up to ``site`` and multiplied by
    ``gain`` (its sign included) there.  site None: the cut alone."""
    ssr = variant == "ssr"
    enc_ch = sd["pts_linears.0.weight"].shape[1]
    shading1 = layer_of(variant, "shading1")
    res, alb2, sh2 = ("residual_linear" if ssr else "shading_linear"), "albedo_linear2", ("shading_linear2" if ssr else "test_linear2")
    hidden = ["albedo_linear1", shading1] + ([SEMANTIC] if ssr and classes else [])
    col_of = lambda layer: (enc_ch + J) if layer == 5 else J            # (pts_linears.5 reads [enc | h4])
    # the cut: unit J's column in every consumer, its own rows
    for layer in range(1, 8):
        sd[f"pts_linears.{layer}.weight"][:, col_of(layer)] = 0.0
    for name in ["alpha_linear", "feature_linear"] + hidden:
        sd[name + ".weight"][:, J] = 0.0
    for layer in range(8):
        _row(sd, f"pts_linears.{layer}", J)
    if site is None:
        return sd
    assert site != ENCODING and gain != 0.0
    last = int(site[-1]) if site in TRUNK_SITES else 7                  # the wire's last trunk layer
    for layer in range(last + 1):
        g = gain if site == f"pts_linears.{layer}" else 1.0
        _row(sd, f"pts_linears.{layer}", J, 0 if layer == 0 else col_of(layer), g)
        if layer == 0:
            sd["pts_linears.0.bias"][J] = -g * X0
    if site == "feature_linear":
        _row(sd, "feature_linear", J, J, gain)
        sd["views_linears.0.weight"][:, J] = 0.0
    elif site == "views_linears.0":
        _row(sd, "feature_linear", J, J, 1.0)
        sd["views_linears.0.weight"][:, J] = 0.0
        _row(sd, "views_linears.0", K, J, gain)
        sd[res + ".weight"][:, K] = 0.0
    elif site in ("albedo_linear1", "shading1", SEMANTIC):
        name = layer_of(variant, site)
        _row(sd, name, K, J, gain)
        sd[{"albedo_linear1": alb2, shading1: sh2, SEMANTIC: "semantic_linear.1"}[name] + ".weight"][:, K] = 0.0
    return sd


def cut_raw_coordinate(sd):
    """the encoding site: column 0 of the encoding (the raw, divided x) reaches no layer"""
    enc_ch = sd["pts_linears.0.weight"].shape[1]
    assert sd["pts_linears.5.weight"].shape[1] == enc_ch + 256
    sd["pts_linears.0.weight"][:, 0] = 0.0
    sd["pts_linears.5.weight"][:, 0] = 0.0
    return sd


# ---------------------------------------------------------------------------------------------------------------------
# the rays
# ---------------------------------------------------------------------------------------------------------------------
def ramp(rays, z, div):
    """fp64 [n, s]: u = x / xyz_div - X0 of the fp32 positions the kernels form"""
    return fs.positions(rays, z, div)[:, 0].double().reshape(z.shape) - X0


def layout(n, s, div, offenders, seed=0, t=T):
    """(rays [n, 11], z [n, s]) with u from -1 (depth 2) to top_r (depth 6, the ray's last): top_r in [1.05, 1.3] t for the rays of
    ``offenders`` (bool [n]), in [0.5, 0.95] t for the others; no point within BAND of t."""
    g = torch.Generator().manual_seed(1000 + seed)
    rays, z = fs.rays_and_depths(n, s, seed=seed, origin_scale=div)
    z[:, -1] = 6.0
    top = torch.where(offenders, 1.05 + 0.25 * torch.rand(n, generator=g), 0.5 + 0.45 * torch.rand(n, generator=g)).double() * t
    dx = (top + 1.0) * div / 4.0
    rays[:, 3] = dx.float()
    rays[:, 0] = ((X0 - 1.0) * div - 2.0 * dx).float()
    for _ in range(4):
        u = ramp(rays, z, div)
        inside = ((u / t - 1.0).abs() <= 1.5 * BAND)
        inside[:, -1] = False                                           # (top_r is outside by construction)
        if not bool(inside.any()):
            break
        target = torch.where(u >= t, (1.0 + 2.0 * BAND) * t, (1.0 - 2.0 * BAND) * t)
        moved = z.double() + (target - u) * div / rays[:, 3:4].double()
        z = torch.where(inside, moved.float(), z)
    z = torch.sort(z, -1)[0].contiguous()
    assert float(z.min()) >= 1.5 and float(z[:, -1].max()) == 6.0 and bool((z[:, -1] == 6.0).all())
    return rays.contiguous(), z


def encoding_layout(n, s, div, set_rays, near_rays, seed=0):
    """rays of ``set_rays`` at x / div = +-1.01 LIMIT, of ``near_rays`` at +-0.99 LIMIT (d_x = 0: every point of the ray), the rest
    ordinary"""
    rays, z = fs.rays_and_depths(n, s, seed=seed, origin_scale=div)
    sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)
    for mask, level in ((set_rays, 1.01), (near_rays, 0.99)):
        rays[mask, 0] = (sign * level * LIMIT * div)[mask]
        rays[mask, 3] = 0.0
    return rays.contiguous(), z


def default_offenders(n, status_rays):
    """one ray in each of words 1 and 4, two in word 3 (words: ``status_rays`` rays each; at least 6 of them)"""
    words = n // status_rays
    assert words >= 6 and n % status_rays == 0
    mask = torch.zeros(n, dtype=torch.bool)
    for word, ray in ((1, 0), (3, 0), (3, status_rays - 1), (4, status_rays // 2)):
        mask[word * status_rays + ray] = True
    return mask


def words_of(points, n, s, status_rays):
    """bool [ceil(n / status_rays)]: the words that own a ray with a point of ``points`` (bool [n * s] or [n, s])"""
    per_ray = points.reshape(n, s).any(-1)
    out = torch.zeros(-(-n // status_rays), dtype=torch.bool)
    out[per_ray.nonzero().flatten() // status_rays] = True
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a case
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One (variant, site) case at one gain: weights, rays, the fp64 and fp32 slots and rows, the site's value per point."""

    def __init__(self, variant, classes, endpoint, n, s, status_rays, site, gain=None, level=None, seed=0, offenders=None):
        """``gain``: the site's gain with its sign (None: GAIN); ``level``: instead, the gain that brings the LARGEST activation to
        ``level`` * LIMIT (0.99: nothing leaves the range).  The encoding site takes neither."""
        self.variant, self.classes, self.endpoint, self.n, self.s, self.status_rays, self.site = variant, classes, endpoint, n, s, status_rays, site
        assert (s * status_rays) % 128 == 0, "a 64- or 128-point tile would straddle two status words"
        self.div = 10.0 if variant == "ssr" else 1.0
        self.words = -(-n // status_rays)
        offenders = default_offenders(n, status_rays) if offenders is None else offenders
        sd = rr.weights(variant, classes, "sharp")
        if site == ENCODING:
            near = torch.roll(offenders, 1)                             # the ray after each offender: 0.99 LIMIT
            assert not bool((near & offenders).any()) and gain is None
            if level is not None:                                       # nothing beyond the limit: the 0.99 group alone
                assert level == 0.99
                offenders = torch.zeros_like(offenders)
            self.rays, self.z = encoding_layout(n, s, self.div, offenders, near, seed)
            self.near_rays = near
            cut_raw_coordinate(sd)
            self.gain = 1.0
        else:
            self.rays, self.z = layout(n, s, self.div, offenders, seed)
            self.u = ramp(self.rays, self.z, self.div)
            self.gain = GAIN if gain is None else float(gain)
            if level is not None:
                self.gain = level * LIMIT / float(self.u.max())
            wire(variant, classes, sd, site, self.gain)
        self.offenders = offenders
        make = functools.partial(fs.make_module, variant, classes)
        slots64 = fs.reference_slots(make(sd), self.rays, self.z, self.div, endpoint)
        rr._centre_sharp(variant, classes, sd, slots64)                 # the output layers alone change: sigma of both signs
        self.sd = sd
        self.slots64 = fs.reference_slots(make(sd), self.rays, self.z, self.div, endpoint)
        self.slots32 = fs.reference_slots(make(sd), self.rays, self.z, self.div, endpoint, dtype=torch.float32)
        self.raw64, self.raw32 = self.slots64["raw"], self.slots32["raw"]

    # the site's value per point
    def site_value(self, slots=None):
        slots = self.slots64 if slots is None else slots
        if self.site == ENCODING:
            return slots[kernels.SAVE_ENC][:, 0]
        slot, col = site_slot(self.site)
        return slots[slot][:, col]

    def analytic(self):
        """fp64 [n * s]: what the wire should deliver - relu(gain * relu(u)) at a ReLU site (pts_linears.0, which has no ReLU in front
        of it: relu(gain * u) - flipped, the clipped part of the ramp, at most |gain| (1 + 1e-6)), gain * relu(u) at feature_linear"""
        if self.site == "pts_linears.0":
            return torch.relu(self.gain * self.u).flatten()
        v = self.gain * torch.relu(self.u).flatten()
        return torch.relu(v) if self.site in RELU_SITES else v

    def beyond(self, slots=None):
        return self.site_value(slots).abs() > LIMIT

    def in_band(self):
        return ((self.site_value().abs() / LIMIT - 1.0).abs() <= BAND)

    def other_split_max(self):
        """the largest |split value| / LIMIT over every slot of the fp64 reference, the site's own unit left out"""
        worst = 0.0
        skip = (kernels.SAVE_ENC, 0) if self.site == ENCODING else site_slot(self.site)
        for slot in fs.ACTIVATION_SLOTS:
            v = self.slots64[slot].abs()
            if not v.numel():
                continue
            if slot == skip[0]:
                v = v.clone()
                v[:, skip[1]] = 0.0
            worst = max(worst, float(v.max()))
        return worst / LIMIT

    def e_all(self):
        return words_of(self.beyond(), self.n, self.s, self.status_rays)

    def e_live(self, sigma):
        """``sigma`` [n * s]: the words that own a ray with a point beyond the limit whose density is positive"""
        return words_of(self.beyond() & (sigma.detach().cpu().flatten() > 0), self.n, self.s, self.status_rays)

    def clear_rows(self, words_set):
        """bool [n * s]: the points of the rays whose word is not in ``words_set`` (bool [words])"""
        ray_word = torch.arange(self.n) // self.status_rays
        return (~words_set[ray_word])[:, None].expand(self.n, self.s).reshape(-1)


@functools.lru_cache(maxsize=None)
def case(variant, classes, endpoint, n, s, status_rays, site, kind="over", seed=0):
    """``kind``: ``over`` (GAIN), ``flipped`` (-GAIN), ``under`` (the largest activation at 0.99 LIMIT), ``unit`` (gain 1)"""
    kw = {"over": {}, "flipped": {"gain": -GAIN}, "under": {"level": 0.99}, "unit": {"gain": 1.0}}[kind]
    return Case(variant, classes, endpoint, n, s, status_rays, site, seed=seed, **kw)


def wire_words(n, s, div, status_rays, offenders, seed=0):
    """(rays, z, expected words) of a wire case from the ramp alone - for point counts whose fp64 slots would take too long (the
    persistent loops); tests/test_range_guard_cpu.py shows that the site's fp64 slot is GAIN * relu(u) to 1e-12 relative."""
    rays, z = layout(n, s, div, offenders, seed)
    u = ramp(rays, z, div)
    assert not bool(((GAIN * torch.relu(u) / LIMIT - 1.0).abs() <= BAND).any())
    return rays, z, words_of(GAIN * torch.relu(u) > LIMIT, n, s, status_rays)


def lattice(div, dim=16):
    """(t, scale, transform) of a ``dim``^3 lattice whose x / xyz_div - X0 grows along the lattice order (x is the slowest index) from
    -1 to 5 in steps of 0.4: slab 12 at 0.95 T, slab 13 at 1.05 T; y and z as an ordinary box"""
    t = torch.linspace(-1.0, 1.0, steps=dim)
    return t, [3.0 * div, 1.0, 1.0], [1.0, 0.0, 0.0, (2.0 + X0) * div, 0.0, 1.0, 0.0, 0.3, 0.0, 0.0, 1.0, -0.2]


def lattice_site_value(variant, classes, site, points):
    """fp64 [p]: the site's unit of the wired network (GAIN) on lattice ``points`` [p, 3] (fp32, CPU), and the largest other split value
    as a share of the limit"""
    div = 10.0 if variant == "ssr" else 1.0
    sd = wire(variant, classes, rr.weights(variant, classes, "sharp"), site, GAIN)
    rays = torch.zeros(points.shape[0], 11)
    rays[:, 0:3] = points
    rays[:, 10] = 1.0
    slots = fs.reference_slots(fs.make_module(variant, classes, sd), rays, torch.zeros(points.shape[0], 1), div, False)
    slot, col = site_slot(site)
    value = slots[slot][:, col].clone()
    worst = 0.0
    for k in fs.ACTIVATION_SLOTS:
        v = slots[k].abs()
        if k == slot:
            v = v.clone()
            v[:, col] = 0.0
        worst = max(worst, float(v.max()) if v.numel() else 0.0)
    return value, worst / LIMIT
