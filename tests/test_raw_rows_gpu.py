"""The raw rows - [rgb, sigma, albedo, shading, residual | logits | endpoint] per sample point - of every fused forward form against fp64,
point for point, at the yardstick of the activation slots (tests/test_forward_slots_gpu.py): per channel group
max |got - fp64| <= 4 D + 2^-21 max |fp64|, D = the reference's own fp32 forward against fp64 on the same points (tests/_raw_rows.py).

The slot tests stop one layer short of the rows, and every other test of the rows uses 1e-5 + 1e-4 |want|, 100 to 1000 times the kernels' own
error: a dropped product in an output head, a partial sum of one wave left out of the exchange, a half from the wrong plane pass all of them
(tests/test_raw_rows_cpu.py shows by how much, and that this bound sees each).  Here each form's tail is pinned on its own - the 1-4-row heads,
the four-wave exchange, the sigmoids and albedo * shading + residual, the per-wave / channel-split / 128-point semantic heads, the endpoint
copy, the sixteen-byte-piece and four-byte row stores - so a fault that all forms of a network share shows too.  The bit-equalities between
forms (t128 = dual = pp, gated survivors = plain, training buffers) stay where they are.

Every launch goes through the C ABI into a caller-owned view pre-filled with a NaN word, 16 guard words either side, and checks: every word of
the rows written, the guards intact, status 0, every group inside its bound.  Weights: ``sharp`` (tests/_raw_rows.py) - sigma of both signs,
sigmoids from 0.002 to 0.999, logits of both signs.

Worst figures on an MI355X (profiles/raw_rows.txt has every line), err / D and err / bound per group over all 75 cases; no factor was raised:
  f16x3 forms   rgb 2.06 / 0.40, sigma 1.90 / 0.37, albedo 1.85 / 0.24, shading 1.99 / 0.27, residual 2.09 / 0.42, logits 1.56 / 0.28,
                endpoint 1.26 / 0.17; the one-point launches, whose D is ONE point's fp32 error: sigma 3.17 / 0.54, residual 3.27 / 0.43, rgb 2.62 / 0.28
  exact fp32    rgb 2.63 / 0.48, sigma 1.89 / 0.40, albedo 1.99 / 0.26, shading 1.99 / 0.29, residual 2.55 / 0.49, logits 2.09 / 0.36, endpoint 2.06 / 0.27
  slot module   (default-init weights, tests/test_forward_slots_gpu.py) err / bound at most 0.28 (sigma), err / D at most 1.54 but for sigma of its
                one-point case (8.4: that D is one point's; it passes through the bound's second term at 0.16)
  reduced encodings  (the 22 cases at (6, 2), (0, 0) and SSR C = 28 at (3, 0); profiles/backward_descs.txt) err / D at most 2.95 (residual, exact
                fp32 at (0, 0)), err / bound at most 0.67 (sigma, exact fp32, C = 28 at (3, 0), 65 points); the f16x3 forms at most 0.54 (residual, C = 28 at (3, 0), 703 points); no factor raised
A scratch build without one  w_lo x_hi  product of regop_gemm (csrc/mlp_f16_heads.h) fails every two-workgroup and 128-point case here on
albedo, shading, residual and rgb - 60, 81 and 160 times the bound, the CPU module's prediction - and passes test_encode_mlp_raw.
"""
import functools

import pytest
import torch

import _forward_slots as fs
import _raw_rows as rr
from intrinsicnerf_amd import _capi, packing

pytestmark = pytest.mark.gpu

ENV = ("INERF_PRECISION", "INERF_F16_KERNEL", "INERF_TRAIN_FWD", "INERF_GATE", "INERF_PROBE", "INERF_PROBE_WG", "INERF_GATE_BYTES", "INERF_ENC_CACHE")
# form -> environment (f32: the descriptor's precision instead - k_encode_mlp, csrc/mlp.hip)
FORMS = {"default": {}, "f32": {}, "dual": {"INERF_F16_KERNEL": "dual"}, "single": {"INERF_F16_KERNEL": "single"}, "pp": {"INERF_F16_KERNEL": "pp"},
         "wave": {"INERF_F16_KERNEL": "wave"}, "csplit": {"INERF_F16_KERNEL": "csplit"}, "t128": {"INERF_F16_KERNEL": "t128"},
         "train-t128": {"INERF_TRAIN_FWD": "t128"}, "probe-wg1": {"INERF_PROBE_WG": "1"}}
KIND = "sharp"


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _select_form(monkeypatch, form):
    for name, value in FORMS[form].items():
        monkeypatch.setenv(name, value)


def _points(points):
    """A tile-loop case's point count: the persistent loop's second trip with a ragged last tile, three tiles beyond the grid."""
    if isinstance(points, int):
        return points
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {"loop-2wg": 64 * (2 * cus + 3) - 5, "loop-1wg": 64 * (cus + 3) - 5, "loop-t128": 128 * (cus + 3) - 5}[points]


@functools.lru_cache(maxsize=None)
def _packed(variant, classes, endpoint, p, precision, enc=(10, 4)):
    """the case's packed weights on the host, once per format"""
    return packing.pack_state_dict(rr.desc_of(variant, classes, precision, *enc), rr.case_weights(variant, classes, endpoint, p, KIND, *enc))


def _setup(variant, classes, endpoint, p, form, enc=(10, 4)):
    dev = torch.device("cuda:0")
    precision = _capi.PREC_F32 if form == "f32" else _capi.PREC_F16X3
    desc = rr.desc_of(variant, classes, precision, *enc)
    rays, z, raw64, raw32 = rr.reference(variant, classes, endpoint, p, KIND, *enc)
    return dev, desc, _packed(variant, classes, endpoint, p, precision, enc).to(dev), rays.to(dev), z.to(dev), raw64, raw32


def _launch(dev, desc, packed, rays, z, flags, offset=0, probe_out=None):
    buf = rr.RawBuffer(z.numel(), _capi.lib().inerf_raw_channels(desc, flags, 1), dev, offset)
    status = rr.launch(desc, packed, rays, z, flags, buf.rows, probe_out)
    return buf, status


def _written(buf, problems, tag):
    left = buf.words() == fs.SENTINEL
    if bool(left.any()):
        ch = buf.rows.shape[1]
        rows = left.view(-1, ch).any(1).nonzero().flatten()
        problems.append(f"{tag}: {int(left.sum())} words of the rows never written, in {rows.numel()} points (first {rows[:4].tolist()})")
    if not buf.guards_intact():
        problems.append(f"{tag}: the guard words around the rows were written")


def _id(variant, classes, endpoint, form, points, enc=(10, 4)):
    return (f"{variant}{classes if variant == 'ssr' else ''}{'-endpoint' if endpoint else ''}-{form}-{points}"
            + ("" if enc == (10, 4) else f"-x{enc[0]}d{enc[1]}"))


def _params(rows):
    """rows of (variant, classes, endpoint, form, points[, (l_xyz, l_dir)]): the encodings default to (10, 4)"""
    return [pytest.param(*(tuple(r) + ((10, 4),))[:6], id=_id(*r)) for r in rows]


# ---------------------------------------------------------------------------------------------------------------------
# 1. inference forms
# ---------------------------------------------------------------------------------------------------------------------
INFERENCE = (
    # object-level: the 128-point tile, the two-workgroup kernel, the one-workgroup kernel, the pipelined trunk, exact fp32
    [("object", 0, False, form, 703) for form in ("default", "dual", "single", "pp", "f32")]
    + [("object", 0, False, form, p) for form in ("default", "dual") for p in (1, 63, 64, 65, 127, 128, 129)]
    # SSR, C = 28: the channel-split head, the per-wave head, the one-workgroup kernel, the 128-point tile's head, exact fp32
    + [("ssr", 28, False, form, 703) for form in ("default", "wave", "single", "t128", "f32")]
    + [("ssr", 28, False, "default", p) for p in (65, 129)]
    # more than 32 classes: the per-wave head by default, the channel-split head block by block through the scratch on request
    + [("ssr", c, False, form, 320) for c in (33, 240) for form in ("default", "csplit", "single", "f32")]
    # the edges of sem_head's 16-row blocks and of the 32-class blocks; C = 1 and C = 240 (above) are the ends
    + [("ssr", c, False, form, 65) for c in (1, 16, 17, 32) for form in ("default", "wave", "t128")]
    + [("ssr", 0, False, "default", 65)]
    # the endpoint feature takes the one-workgroup kernel
    + [("ssr", 5, True, form, 147) for form in ("default", "f32")]
    # the persistent loop's second trip, one case per kernel body
    + [("object", 0, False, "dual", "loop-2wg"), ("ssr", 28, False, "default", "loop-2wg"), ("object", 0, False, "single", "loop-1wg"),
       ("object", 0, False, "default", "loop-t128"), ("ssr", 28, False, "t128", "loop-t128")]
    # reduced encodings (the pad columns of the encoding slots start at 39 / 15, 3 / 3 and 21 / 3): every object-level body, the SSR heads
    + [("object", 0, False, form, p, enc) for enc in ((6, 2), (0, 0)) for form in ("default", "dual", "single", "f32") for p in (703, 65)]
    + [("ssr", 28, False, form, p, (3, 0)) for form in ("default", "t128", "f32") for p in (703, 65)])


@pytest.mark.parametrize("variant,classes,endpoint,form,points,enc", _params(INFERENCE))
def test_rows_against_fp64(variant, classes, endpoint, form, points, enc, monkeypatch):
    """inerf_encode_mlp_probed, one launch: rows written, guards intact, status 0, every group within 4 D + 2^-21 max |fp64| of fp64."""
    print()
    p = _points(points)
    tag = _id(variant, classes, endpoint, form, points, enc) + (f" ({p} points)" if p != points else "")
    _select_form(monkeypatch, form)
    dev, desc, packed, rays, z, raw64, raw32 = _setup(variant, classes, endpoint, p, form, enc)
    buf, status = _launch(dev, desc, packed, rays, z, rr.flags_of(endpoint))
    problems = []
    _written(buf, problems, tag)
    rr.judge(buf.rows, raw64, raw32, rr.groups(variant, classes, endpoint), tag, problems)
    assert status == 0
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the density gate
# ---------------------------------------------------------------------------------------------------------------------
GATE_POINTS = 703                # 37 rays x 19 samples
GATE_RAYS_PER_SUB = 13           # sub-ranges of 13, 13 and 11 rays; the second and third start 4 and 8 bytes off a sixteen-byte boundary


@pytest.mark.parametrize("probe,form", [pytest.param(False, "default", id="gate"), pytest.param(True, "default", id="gate-probe-wg2"),
                                        pytest.param(True, "probe-wg1", id="gate-probe-wg1")])
def test_gated_rows_against_fp64(probe, form, monkeypatch, request):
    """INERF_FLAG_GATE_COLOUR [| INERF_FLAG_GATE_PROBE] over three sub-ranges.  fp64 sigma above +bound: the whole row is judged.  Below
    -bound: sigma <= 0 (without the probe within the bound of fp64; with it the culled points carry the probe's s < 0) and the ten colour
    channels are +0, bit for bit.  Inside +- bound - the one exclusion - at most 1 % of the points (the reference has none:
    test_raw_rows_cpu.py)."""
    print()
    tag = request.node.callspec.id
    n, s = rr.split(GATE_POINTS)
    assert (n, s) == (37, 19)
    monkeypatch.setenv("INERF_GATE_BYTES", str(GATE_RAYS_PER_SUB * s * 1028))      # 1028 bytes per point: a record and its index
    _select_form(monkeypatch, form)
    dev, desc, packed, rays, z, raw64, raw32 = _setup("object", 0, False, GATE_POINTS, form)
    buf, status = _launch(dev, desc, packed, rays, z, rr.flags_of(gate_colour=True, gate_probe=probe))
    groups = rr.groups("object", 0, False)
    bound = rr.bound_of(raw64, raw32, "sigma", groups["sigma"])[0]
    live, dead = raw64[:, 3] > bound, raw64[:, 3] < -bound
    undecided = int((~live & ~dead).sum())
    print(f"{rr.TAG} {tag}: {int(live.sum())} points above +bound, {int(dead.sum())} below -bound, {undecided} inside (bound {bound:.3e})")
    first = [0, GATE_RAYS_PER_SUB * s, 2 * GATE_RAYS_PER_SUB * s, GATE_POINTS]
    for a, b in zip(first[:-1], first[1:]):                   # every sub-range has points on both sides
        assert 0 < int(live[a:b].sum()) < b - a
    problems = []
    _written(buf, problems, tag)
    rr.judge(buf.rows, raw64, raw32, groups, tag + " live", problems, rows=live)
    got = buf.rows.cpu()
    if not probe:
        rr.judge(buf.rows, raw64, raw32, groups, tag + " dead", problems, rows=dead, only=("sigma",))
    if not bool((got[dead][:, 3] <= 0).all()):
        problems.append(f"{tag}: {int((~(got[dead][:, 3] <= 0)).sum())} points below -bound whose sigma is not <= 0")
    colours = got[dead][:, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]].contiguous().view(torch.int32)
    if not bool((colours == 0).all()):
        problems.append(f"{tag}: {int((colours != 0).sum())} colour words of points below -bound are not +0")
    assert status == 0
    assert undecided <= GATE_POINTS // 100
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the training forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,classes,endpoint,form,points,enc", _params([
    ("object", 0, False, "default", 703), ("object", 0, False, "single", 703), ("object", 0, False, "train-t128", 703),
    ("ssr", 28, False, "default", 703), ("ssr", 28, False, "single", 703), ("ssr", 5, True, "default", 147)]))
def test_training_forward_rows_against_fp64(variant, classes, endpoint, form, points, enc, monkeypatch):
    """inerf_encode_mlp_train (the saving forms of the same tails): the same four checks on its raw rows."""
    print()
    tag = "train " + _id(variant, classes, endpoint, form, points)
    _select_form(monkeypatch, form)
    dev, desc, packed, rays, z, raw64, raw32 = _setup(variant, classes, endpoint, points, form)
    buf = rr.RawBuffer(points, raw64.shape[1], dev)
    _, _, _, status = fs.run_train_forward(desc, packed, rays, z, endpoint, raw=buf.rows)
    problems = []
    _written(buf, problems, tag)
    rr.judge(buf.rows, raw64, raw32, rr.groups(variant, classes, endpoint), tag, problems)
    assert status == 0
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# 4. rows that start four bytes off a sixteen-byte boundary
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("points", [703, 129])
@pytest.mark.parametrize("form", ["default", "dual", "single"])
@pytest.mark.parametrize("variant,classes", [("object", 0), ("ssr", 28)])
def test_rows_off_the_sixteen_byte_boundary_are_the_same_bits(variant, classes, form, points, monkeypatch):
    """The 11-channel rows of whole tiles leave as sixteen-byte pieces when ``raw`` is sixteen-byte aligned and as four-byte stores when it is
    not (csrc/mlp_f16.hip, csrc/mlp_f16_t128.hip: whole_rows): the same input into a view offset by one float gives the same rows, bit for bit,
    all of them written, and touches no word either side."""
    _select_form(monkeypatch, form)
    dev, desc, packed, rays, z, _, _ = _setup(variant, classes, False, points, form)
    aligned, status_a = _launch(dev, desc, packed, rays, z, 0)
    shifted, status_s = _launch(dev, desc, packed, rays, z, 0, offset=1)
    assert aligned.rows.data_ptr() % 16 == 0 and shifted.rows.data_ptr() % 16 == 4
    problems = []
    _written(aligned, problems, "aligned")
    _written(shifted, problems, "offset by one float")
    assert status_a == 0 and status_s == 0
    assert not problems, "; ".join(problems)
    assert torch.equal(aligned.words(), shifted.words())
