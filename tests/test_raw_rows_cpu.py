"""CPU: that the cases of tests/test_raw_rows_gpu.py are fair and that its bound can see ONE dropped product - before anything runs on a GPU.

The bound is tests/_raw_rows.py's, per channel group: 4 D + 2^-21 max |fp64|, D = the reference's own fp32 forward against fp64.

  inputs       the ``sharp`` weights populate what the kernels' tails branch on: either sign of sigma in a quarter of the points at least,
               sigmoid outputs below 0.05 and above 0.9 in the residual group, logits of both signs; no point of the gated case has its
               fp64 sigma inside +- bound (the gated test leaves such points out).  The gains alone do not get there - object-level at 703
               points tops out at 0.898, the 65-point cases stay inside [0.22, 0.78] - so the recipe centres the residual head per case and
               doubles its gain until it does (tests/_raw_rows.py _centre_sharp); the conditions here are on the reference alone
  sensitivity  an output layer's weights rounded to their f16 hi half at the packer's power-of-two scale (csrc/pack.cpp weight_scale,
               split_f16) - what a dropped  w_lo x_hi  MFMA does - or the layer's input rounded towards zero to its f16 hi half at the
               activation scale 8 (a dropped  w_hi x_lo), everything else in fp64: the worst error on the layer's own group is at least
               2 x bound with the ``plain`` weights and 8 x with the ``sharp`` ones.  Each line also shows the error against the plain
               tolerance 1e-5 + 1e-4 |want| of the tests that existed: below 1 means they could not have noticed.
  judge        one moved value gives one problem that names its point; an untouched copy none; a sentinel word is "never written".

Figures of this module (pytest -s prints every line), the smallest ratio to the bound over the cases: without a weight lo half 2.4 (plain:
shading, SSR C = 5 with the endpoint feature) and 27 (sharp: residual, C = 17 at 65 points); without an activation lo half 7.2 (plain) and 120
(sharp).  Against the plain tolerance the same errors of the plain weights are at most 0.73 (weight lo) and 1.96 (activation lo; only the logits
and sigma pass 1): the tests that existed could not have noticed a dropped weight product with the network they use.  With the sharp gains
sigma's error is 90 to 770 times that tolerance, the other heads' 0.3 to 76 times."""
import copy

import pytest
import torch

import _forward_slots as fs
import _raw_rows as rr
from intrinsicnerf_amd import kernels

# (variant, classes, endpoint, points): the GPU module's cases at 703 / 320 / 147 / 65 points
SHARP_CASES = [("object", 0, False, 703), ("object", 0, False, 65), ("ssr", 28, False, 703), ("ssr", 28, False, 65), ("ssr", 33, False, 320),
               ("ssr", 240, False, 320), ("ssr", 1, False, 65), ("ssr", 16, False, 65), ("ssr", 17, False, 65), ("ssr", 32, False, 65),
               ("ssr", 0, False, 65), ("ssr", 5, True, 147)]
# the forward-slots module's cases at those sizes (its raw rows are judged with the ``plain`` weights)
PLAIN_CASES = [("object", 0, False, 703), ("object", 0, False, 65), ("ssr", 28, False, 703), ("ssr", 0, False, 65), ("ssr", 5, True, 147)]
# reduced encodings (test_raw_rows_gpu.py's last rows): (..., kind, l_xyz, l_dir)
REDUCED_CASES = [("object", 0, False, p, "sharp", lx, ld) for lx, ld in ((6, 2), (0, 0)) for p in (703, 65)] + [("ssr", 28, False, p, "sharp", 3, 0) for p in (703, 65)]
CASES = [c + ("sharp",) for c in SHARP_CASES] + [c + ("plain",) for c in PLAIN_CASES] + REDUCED_CASES
MIN_RATIO = {"plain": 2.0, "sharp": 8.0}


def _id(case):
    variant, classes, endpoint, p, kind = case[:5]
    return f"{variant}{classes if variant == 'ssr' else ''}{'-endpoint' if endpoint else ''}-{p}-{kind}" + (f"-x{case[5]}d{case[6]}" if len(case) > 5 else "")


def _plain_tolerance_ratio(err, want):
    """worst |err| / (1e-5 + 1e-4 |want|), value by value: tests/_cases.py's tolerance, the one the other raw-row tests use"""
    return float((err / (1e-5 + 1e-4 * want.abs())).max())


def f16_hi_weights(w):
    """The f16 hi half of a GEMM's weights at the packer's scale: the power of two that brings max |w| = f 2^e, f in [0.5, 1), to
    2^14 f; hi = f16(w scale) to nearest."""
    scale = 2.0 ** (14 - int(torch.frexp(w.abs().max())[1]))
    return ((w.float() * scale).half().double() / scale).to(w.dtype)


def f16_hi_activations(v):
    """The f16 hi half of non-negative activations as the layer slots carry them: 8 v rounded TOWARDS ZERO to f16 (include/inerf.h)."""
    x = v.double() * kernels.ACT_SCALE
    assert bool((x >= 0).all())
    h = x.to(torch.float16)
    above = h.double() > x                                   # to-nearest went up: one f16 step back (positive, so the bit pattern - 1)
    h = torch.where(above, (h.view(torch.int16) - 1).view(torch.float16), h)
    assert bool((h.double() <= x).all()) and bool((x - h.double() <= x * 2.0 ** -10 + 2.0 ** -24).all())
    return h.double() / kernels.ACT_SCALE


@pytest.mark.parametrize("case", [c for c in CASES if c[4] == "sharp"], ids=_id)
def test_sharp_inputs_are_what_the_docstrings_say(case):
    variant, classes, endpoint, p, kind = case[:5]
    raw64 = rr.reference(*case)[2]
    g = rr.groups(variant, classes, endpoint)
    sigma = raw64[:, 3]
    res = raw64[:, g["residual"][0]:g["residual"][1]]
    sig = raw64[:, 4:11]
    print(f"\n{rr.TAG} inputs {_id(case)}: sigma [{float(sigma.min()):.3f}, {float(sigma.max()):.3f}], > 0 in {float((sigma > 0).double().mean()):.3f}, "
          f"< 0 in {float((sigma < 0).double().mean()):.3f}; sigmoid outputs [{float(sig.min()):.4f}, {float(sig.max()):.4f}], residual "
          f"[{float(res.min()):.4f}, {float(res.max()):.4f}]"
          + (f"; logits [{float(raw64[:, 11:11 + classes].min()):.3f}, {float(raw64[:, 11:11 + classes].max()):.3f}]" if classes else ""))
    assert float((sigma > 0).double().mean()) >= 0.25 and float((sigma < 0).double().mean()) >= 0.25
    assert float(res.min()) < 0.05 and float(res.max()) > 0.9
    if classes > 1:
        logits = raw64[:, 11:11 + classes]
        assert float(logits.min()) < 0 < float(logits.max())
    assert bool(torch.isfinite(raw64).all())


def test_no_point_of_the_gated_case_is_undecided():
    """The gated test leaves out the points whose fp64 sigma lies inside +- bound: the reference has none at its size."""
    _, _, raw64, raw32 = rr.reference("object", 0, False, 703, "sharp")
    bound, d = rr.bound_of(raw64, raw32, "sigma", (3, 4))
    closest = float(raw64[:, 3].abs().min())
    print(f"\n{rr.TAG} gated object-703: sigma bound {bound:.3e} (D {d:.3e}), smallest |sigma| {closest:.3e}")
    assert int((raw64[:, 3].abs() <= bound).sum()) == 0


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_bound_sees_one_dropped_product(case):
    variant, classes, endpoint, p, kind = case[:5]
    _, _, raw64, raw32 = rr.reference(*case)
    slots = rr.last_slots(*case)
    groups = rr.groups(variant, classes, endpoint)
    net = rr.module(*case).double()
    assert torch.equal(fs.heads_from_slots(net, slots, endpoint), raw64)          # the continuation is the reference itself
    inputs = {"sigma": kernels.SAVE_H0 + 7, "albedo": kernels.SAVE_AS1H, "shading": kernels.SAVE_AS1H, "residual": kernels.SAVE_VH,
              "logits": kernels.SAVE_SEMH}
    print()
    low = []
    for group, layer in rr.output_layers(variant, classes).items():
        a, b = groups[group]
        want = raw64[:, a:b]
        bound, d = rr.bound_of(raw64, raw32, group, (a, b))
        # the layer's weights without their lo half
        dropped = copy.deepcopy(net)
        lin = dropped.get_submodule(layer)
        with torch.no_grad():
            lin.weight.copy_(f16_hi_weights(lin.weight))
        err_w = (fs.heads_from_slots(dropped, slots, endpoint)[:, a:b] - want).abs()
        # the layer's input without its lo half (as1h: the albedo and shading heads' hidden layers side by side - this head's half)
        cut = dict(slots)
        hi = f16_hi_activations(slots[inputs[group]])
        if group == "albedo":
            hi = torch.cat([hi[:, :128], slots[kernels.SAVE_AS1H][:, 128:]], -1)
        elif group == "shading":
            hi = torch.cat([slots[kernels.SAVE_AS1H][:, :128], hi[:, 128:]], -1)
        cut[inputs[group]] = hi
        err_x = (fs.heads_from_slots(net, cut, endpoint)[:, a:b] - want).abs()
        for what, err in (("weight lo", err_w), ("activation lo", err_x)):
            ratio = float(err.max()) / bound
            print(f"{rr.TAG} sensitivity {_id(case)} {group} ({layer}) without its {what}: err {float(err.max()):.3e} = {ratio:.1f} x bound "
                  f"{bound:.3e} (D {d:.3e}), {_plain_tolerance_ratio(err, want):.3f} x the plain tolerance")
            if not ratio >= MIN_RATIO[kind]:
                low.append(f"{group} without its {what}: {ratio:.2f} x bound")
    assert not low, f"{_id(case)}: the bound would miss a dropped product - " + "; ".join(low)


WEIGHT_DIGESTS = {("object", 0): "297b0dfacef27512c26e71d74bc553015393058d790ab193302602986acae728",
                  ("ssr", 28): "f79cff4819300013d0b16f4fd5225c50375a84257ae7d2d34de241594debb19c"}


@pytest.mark.parametrize("variant,classes", list(WEIGHT_DIGESTS))
def test_default_description_weights_are_the_ones_before_the_encoding_arguments(variant, classes):
    """oracle.make_state_dict took l_xyz / l_dir for the reduced-encoding cases: at the default description (variant, classes, seed) gives
    the tensors it gave before - sha256 over names and fp32 bytes in order, recorded from the function without the arguments."""
    import hashlib
    import oracle
    for sd in (oracle.make_state_dict(variant, classes, seed=rr.WEIGHT_SEED),
               oracle.make_state_dict(variant, classes, seed=rr.WEIGHT_SEED, l_xyz=10, l_dir=4), rr.weights(variant, classes, "plain")):
        h = hashlib.sha256()
        for name, t in sd.items():
            h.update(name.encode())
            h.update(t.numpy().tobytes())
        assert h.hexdigest() == WEIGHT_DIGESTS[(variant, classes)]


def test_judge_names_the_point_and_the_unwritten_word(capsys):
    case = ("ssr", 5, True, 147, "sharp")
    _, _, raw64, raw32 = rr.reference(*case)
    groups = rr.groups("ssr", 5, True)
    clean = raw32.clone()                                    # the reference's own fp32 rows: at D, inside 4 D
    problems = []
    rr.judge(clean, raw64, raw32, groups, "self-check", problems)
    assert problems == []
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(rr.TAG)]
    assert len(lines) == len(groups) and all(" err / bound " in ln for ln in lines)
    for name, (a, b) in groups.items():
        bound = rr.bound_of(raw64, raw32, name, (a, b))[0]
        moved = clean.clone()
        point, channel = 100, b - 1
        moved[point, channel] = float(raw64[point, channel]) + 2.0 * bound
        problems = []
        rr.judge(moved, raw64, raw32, groups, "self-check", problems)
        assert len(problems) == 1, problems
        assert f" {name}: " in problems[0] and "1 values over, in 1 of 147 points (first [100])" in problems[0] and "tiles [1]" in problems[0]
    left = clean.clone()
    left.view(torch.int32)[146, 3] = fs.SENTINEL
    problems = []
    rr.judge(left, raw64, raw32, groups, "self-check", problems)
    assert len(problems) == 1 and "sigma: 1 words never written, in 1 of 147 points (first [146])" in problems[0] and "tiles [2]" in problems[0]
    # judging some points only: the moved value is seen where its point is selected and nowhere else
    moved = clean.clone()
    moved[100, 3] += 1.0
    rows = torch.zeros(147, dtype=torch.bool)
    rows[:100] = True
    problems = []
    rr.judge(moved, raw64, raw32, groups, "self-check", problems, rows=rows)
    assert problems == []
    rr.judge(moved, raw64, raw32, groups, "self-check", problems, rows=~rows, only=("sigma",))
    assert len(problems) == 1
