"""INERF_STATUS_F16_RANGE layer by layer in every fused forward form: networks that leave the f16 range at ONE site (tests/_range_guard.py;
tests/test_range_guard_cpu.py shows that the cases are fair) must set exactly the status words of the rays that own a point beyond the
limit there - a site that is not watched, a maximum lost or kept across a trip of a persistent tile loop, a sub-range's first ray left out
of the word index all show as a word that differs - and the rows of every CLEAR word must still be within the raw-rows yardstick
(tests/_raw_rows.py judge: 4 D + 2^-21 max |fp64|) of fp64: a clear word is the caller's licence to believe them.

Every launch goes through the C ABI with one status word per ``status_rays`` rays, zeroed here, eight sentinel words behind them, the
rows in the guarded rr.RawBuffer.  n_samples * status_rays = 128 and every launch starts at ray 0, so no 64- or 128-point tile straddles
two words and the expectation is exact.  One line per launch is printed (profiles/range_guard.txt holds those of a run on an MI355X).

Figures of that run (781 lines); every set of words equal to the expected one, no factor raised:
  clear rows, worst err / bound   f16x3 forms 0.71 (the endpoint group of SSR C = 5 with views_linears.0 at 0.99 of the limit: the group carries
                                  the site's own 7.4e3), 0.48 elsewhere; exact fp32 0.48
  training forward at 0.99        act_max / largest decoded value - 1 between 4.6e-7 and 8.4e-4 (allowed: 0 .. 2^-9 = 1.95e-3)
A scratch build in which the t128 body's epilogue of pts_linears.4 (store256, csrc/mlp_f16_t128.hip) feeds a dead copy of the maximum fails
the pts_linears.4 cases of test_every_site_in_every_form (object, ssr5), test_gate_forms, test_training_forward (object) and test_grid_kernel
(both networks) and nothing else here; the range tests that existed before this file all pass on it.
"""
import ctypes as C
import functools

import pytest
import torch

import _forward_slots as fs
import _range_guard as rg
import _raw_rows as rr
from intrinsicnerf_amd import _capi, kernels, packing
from test_raw_rows_gpu import ENV, FORMS, _points

pytestmark = pytest.mark.gpu

TAG = "range_guard |"
SHAPE = (24, 32, 4)              # rays, samples, rays per status word: 768 points, 6 words of 128 points
STATUS_SENTINEL = 0x5A5A5A5A
STATUS_GUARD = 8
ENV = ENV + ("INERF_GATE_FUSED",)
VARIANTS = {"object": ("object", 0, False, ("default", "dual", "single", "pp", "f32")),
            "ssr5": ("ssr", 5, False, ("default", "wave", "single", "t128", "f32")),
            "ssr33": ("ssr", 33, False, ("csplit",)),
            "ssr5-endpoint": ("ssr", 5, True, ("default", "f32"))}
TRAIN_FORMS = {"default": {}, "single": {"INERF_F16_KERNEL": "single"}, "t128": {"INERF_TRAIN_FWD": "t128"}}      # test_forward_slots_gpu.py


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for name in ENV + ("INERF_TRAIN_FWD",):
        monkeypatch.delenv(name, raising=False)


def _set_env(monkeypatch, env):
    for name in ENV + ("INERF_TRAIN_FWD",):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


@functools.lru_cache(maxsize=None)
def _packed_case(variant, classes, endpoint, site, kind, precision):
    c = rg.case(variant, classes, endpoint, *SHAPE, site, kind)
    return packing.pack_state_dict(rr.desc_of(variant, classes, precision), c.sd)


def _sync(dev=None):
    """a HIP error ends the session: nothing more is started on a device that has faulted"""
    try:
        torch.cuda.synchronize(dev)
    except RuntimeError as e:
        pytest.exit(f"HIP error at a synchronisation: {e}", returncode=3)


def _run(desc, packed, rays, z, flags, status_rays):
    """one inerf_encode_mlp_probed launch: (RawBuffer, bool [words] of the non-zero status words, the status sentinels intact)"""
    lib = _capi.lib()
    dev = rays.device
    n, s = z.shape
    words = -(-n // status_rays) if status_rays > 0 else 1
    buf = rr.RawBuffer(n * s, lib.inerf_raw_channels(desc, flags, 1), dev)
    status = torch.full((words + STATUS_GUARD,), STATUS_SENTINEL, dtype=torch.int32, device=dev)
    status[:words] = 0
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        ws_bytes = int(lib.inerf_encode_mlp_workspace_bytes(desc, n, s, flags))
        if ws_bytes < 0:
            _capi.check(ws_bytes, "inerf_encode_mlp_workspace_bytes")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes > 0 else None
        rc = lib.inerf_encode_mlp_probed(desc, ptr(packed), ptr(rays), ptr(z), n, s, flags, ptr(buf.rows), ptr(status), status_rays, ptr(ws), ws_bytes,
                                         None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == _capi.E_HIP:
        pytest.exit(f"inerf_encode_mlp_probed: HIP error {lib.inerf_last_hip_error()}", returncode=3)
    _capi.check(rc, "inerf_encode_mlp_probed")
    _sync(dev)
    got = status.cpu()
    assert bool(((got[:words] & ~_capi.STATUS_F16_RANGE) == 0).all()), got[:words].tolist()
    return buf, got[:words] != 0, bool((got[words:] == STATUS_SENTINEL).all()) and buf.guards_intact()


def _bits(words):
    return "".join("1" if w else "0" for w in words.tolist())


def _judge_clear(c, buf, got_words, tag, problems):
    """the rows of the clear words against fp64 at the yardstick; the worst err / bound over the groups"""
    rows = c.clear_rows(got_words)
    if not bool(rows.any()):
        return 0.0
    out = rr.judge(buf.rows, c.raw64, c.raw32, rr.groups(c.variant, c.classes, c.endpoint), tag, problems, rows=rows)
    return max(err / bound for err, _, bound in out.values())


def _launch_case(c, kind, form, flags, problems, monkeypatch, env=None, expect=None, judge=True):
    """one form on one case: the words against ``expect`` (None: c.e_all(); f32: none), the clear rows, the sentinels; one printed line"""
    _set_env(monkeypatch, FORMS[form] if env is None else env)
    dev = torch.device("cuda:0")
    precision = _capi.PREC_F32 if form == "f32" else _capi.PREC_F16X3
    desc = rr.desc_of(c.variant, c.classes, precision)
    packed = _packed_case(c.variant, c.classes, c.endpoint, c.site, kind, precision).to(dev)
    buf, got, intact = _run(desc, packed, c.rays.to(dev), c.z.to(dev), flags, c.status_rays)
    expect = (torch.zeros(c.words, dtype=torch.bool) if form == "f32" else c.e_all()) if expect is None else expect
    tag = f"{c.variant}{c.classes or ''}{'-endpoint' if c.endpoint else ''} {c.site} {kind} {form}"
    worst = _judge_clear(c, buf, got, tag, problems) if judge else float("nan")
    print(f"{TAG} {tag}: {int(c.beyond().sum())} points beyond the limit, words expected {_bits(expect)} got {_bits(got)}, clear rows " + (f"err / bound {worst:.2f}" if judge else "bit for bit the ungated ones"))
    if got.tolist() != expect.tolist():
        problems.append(f"{tag}: words {_bits(got)}, expected {_bits(expect)}")
    if not intact:
        problems.append(f"{tag}: the sentinels behind the status words or around the rows were written")
    return buf, got


def _kinds(site):
    return ("over", "under") if site == rg.ENCODING else ("over", "flipped", "under")


# ---------------------------------------------------------------------------------------------------------------------
# a. every site in every form
# ---------------------------------------------------------------------------------------------------------------------
SITE_CASES = [pytest.param(name, site, id=f"{name}-{site}") for name, (v, c, e, _) in VARIANTS.items() for site in rg.sites(v, c)]


@pytest.mark.parametrize("name,site", SITE_CASES)
def test_every_site_in_every_form(name, site, monkeypatch):
    """Per form: at gain LIMIT / T the non-zero words are E_all (exact fp32: none) and the rows of every clear word are within the yardstick;
    with the ramp's sign flipped a ReLU site clips the value to 0 (pts_linears.0, which has no ReLU in front: to the ramp's clipped part,
    a quarter of the limit) and nothing is set, while feature_linear, which has none, counts |t| and sets E_all; with the largest activation
    at 0.99 of the limit nothing is set.  Where nothing is set every row is judged."""
    print()
    variant, classes, endpoint, forms = VARIANTS[name]
    flags = rr.flags_of(endpoint)
    problems = []
    for kind in _kinds(site):
        c = rg.case(variant, classes, endpoint, *SHAPE, site, kind)
        assert kind == "under" or not bool(c.in_band().any())           # (under: the largest activation sits AT the band's edge, 0.99)
        for form in forms:
            _launch_case(c, kind, form, flags, problems, monkeypatch)
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# b. the gate, object-level network
# ---------------------------------------------------------------------------------------------------------------------
GATE_FORMS = {"gate": (False, {}), "probe": (True, {}), "probe-unfused": (True, {"INERF_GATE_FUSED": "0"}), "probe-wg1": (True, {"INERF_PROBE_WG": "1"})}
COLOURS = [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]


def _gate_rows(c, plain, buf, got, sigma, tag, problems):
    """live rows of clear words: the ungated default form's, bit for bit; dead rows: colours +0 and channel 3 <= 0"""
    rows, want = buf.rows.cpu(), plain.rows.cpu()
    live = (~(sigma <= 0)) & c.clear_rows(got)
    dead = sigma <= 0
    if not torch.equal(rows[live].view(torch.int32), want[live].view(torch.int32)):
        problems.append(f"{tag}: {int((rows[live].view(torch.int32) != want[live].view(torch.int32)).any(1).sum())} live rows of clear words differ from the ungated rows")
    if not bool((rows[dead][:, COLOURS].contiguous().view(torch.int32) == 0).all()) or not bool((rows[dead][:, 3] <= 0).all()):
        problems.append(f"{tag}: dead rows with a colour word that is not +0 or with channel 3 > 0")


def _gate_case(c, site, problems, monkeypatch, env_extra=None, forms=GATE_FORMS):
    plain, _ = _launch_case(c, "over", "default", 0, problems, monkeypatch, judge=False)
    sigma = plain.rows[:, 3].cpu()
    head = site in rg.HEAD_SITES
    if head:
        assert bool(torch.isfinite(sigma).all())                      # (the wire leaves sigma alone)
    expect = c.e_live(sigma) if head else c.e_all()
    for form, (probe, env) in forms.items():
        env = dict(env, **(env_extra or {}))
        buf, got = _launch_case(c, "over", form, rr.flags_of(gate_colour=True, gate_probe=probe), problems, monkeypatch, env=env, expect=expect, judge=False)
        _gate_rows(c, plain, buf, got, sigma, f"{site} {form}", problems)
    return expect


@pytest.mark.parametrize("site", rg.sites("object", 0))
def test_gate_forms(site, monkeypatch):
    """INERF_FLAG_GATE_COLOUR alone, with INERF_FLAG_GATE_PROBE, with INERF_GATE_FUSED=0 and with INERF_PROBE_WG=1.  The encoding and the
    trunk sites: E_all - the trunk (gate alone) or the probe (include/inerf.h: 'on this path the trunk's share of INERF_STATUS_F16_RANGE is
    decided on the probe's hi-only activations, for every point') sees every point.  The head sites: E_live, the words of points beyond the
    limit whose density is positive - 'a gated point's heads are not evaluated, so they can neither raise INERF_STATUS_F16_RANGE ...' and 'a
    candidate with sigma <= 0 has its heads evaluated and discarded: ... it raises no flag behind the trunk' (include/inerf.h,
    INERF_FLAG_GATE_COLOUR / INERF_FLAG_GATE_PROBE); the sign is that of the ungated default kernel's own sigma."""
    print()
    c = rg.case("object", 0, False, *SHAPE, site, "over")
    problems = []
    expect = _gate_case(c, site, problems, monkeypatch)
    if site in rg.HEAD_SITES:
        assert bool(expect.any()) and bool((c.e_all() & ~expect).any())
    assert not problems, "; ".join(problems)


@pytest.mark.parametrize("site", ["pts_linears.3", "albedo_linear1"])
def test_gate_sub_ranges(site, monkeypatch):
    """Three sub-ranges of 8 rays (INERF_GATE_BYTES) with every offending ray in the second: a sub-range's first ray belongs in the word
    index."""
    print()
    n, s, status_rays = SHAPE
    offenders = torch.zeros(n, dtype=torch.bool)
    offenders[[9, 10, 12, 13, 14, 15]] = True
    c = rg.Case("object", 0, False, n, s, status_rays, site, offenders=offenders, seed=1)
    assert c.e_all().tolist() == [False, False, True, True, False, False] and not bool(c.in_band().any())
    dev = torch.device("cuda:0")
    problems = []
    desc = rr.desc_of("object", 0, _capi.PREC_F16X3)
    packed = packing.pack_state_dict(desc, c.sd).to(dev)
    rays, z = c.rays.to(dev), c.z.to(dev)
    plain, got = _run(desc, packed, rays, z, 0, status_rays)[:2]
    sigma = plain.rows[:, 3].cpu()
    expect = c.e_live(sigma) if site in rg.HEAD_SITES else c.e_all()
    assert bool(expect.any()) and got.tolist() == c.e_all().tolist()
    for form, (probe, env) in GATE_FORMS.items():
        _set_env(monkeypatch, dict(env, INERF_GATE_BYTES=str(8 * s * 1028)))
        buf, got, intact = _run(desc, packed, rays, z, rr.flags_of(gate_colour=True, gate_probe=probe), status_rays)
        print(f"{TAG} object {site} sub-ranges {form}: {int(c.beyond().sum())} points beyond the limit, words expected {_bits(expect)} got {_bits(got)}")
        if got.tolist() != expect.tolist() or not intact:
            problems.append(f"{form}: words {_bits(got)}, expected {_bits(expect)}, sentinels intact: {intact}")
        _gate_rows(c, plain, buf, got, sigma, f"{site} sub-ranges {form}", problems)
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# c. the training forward
# ---------------------------------------------------------------------------------------------------------------------
def _largest_decoded(desc, save, p):
    lib = _capi.lib()
    largest = 0.0
    for slot in fs.ACTIVATION_SLOTS:
        words, width = fs.slot_words(desc, save, p, slot)
        if width == 0:
            continue
        if lib.inerf_mlp_save_slot_is_fragment(slot, 0) == 1:
            got = fs.planes_value(fs.frag_planes(words, width).cpu())
        else:
            got = words[:p * width].cpu().view(torch.float32).double()
        largest = max(largest, float(got.abs().max()))
    return largest


@pytest.mark.parametrize("name,site", [pytest.param(name, site, id=f"{name}-{site}") for name in ("object", "ssr5") for site in rg.sites(*VARIANTS[name][:2])])
def test_training_forward(name, site, monkeypatch):
    """inerf_encode_mlp_train, forms default / single / t128: the one status word is set at 1.01 of the limit (E_all non-empty) and clear
    at 0.99, where act_max is not below the largest value any slot decodes to and at most (1 + 2^-9) times it (split_upper_bound,
    csrc/mlp_f16_dev.h, documents 2^-10 + 2^-24 / |hi|: twice that)."""
    print()
    variant, classes, endpoint, _ = VARIANTS[name]
    dev = torch.device("cuda:0")
    desc = rr.desc_of(variant, classes, _capi.PREC_F16X3)
    problems = []
    for kind in ("over", "under"):
        c = rg.case(variant, classes, endpoint, *SHAPE, site, kind)
        packed = _packed_case(variant, classes, endpoint, site, kind, _capi.PREC_F16X3).to(dev)
        for form, env in TRAIN_FORMS.items():
            _set_env(monkeypatch, env)
            buf = rr.RawBuffer(c.n * c.s, c.raw64.shape[1], dev)
            _, save, act_max, status = fs.run_train_forward(desc, packed, c.rays.to(dev), c.z.to(dev), endpoint, raw=buf.rows)
            want = int(bool(c.e_all().any()))
            line = f"{TAG} train {name} {site} {kind} {form}: {int(c.beyond().sum())} points beyond the limit, status expected {want} got {status}"
            if status != want * _capi.STATUS_F16_RANGE or not buf.guards_intact():
                problems.append(f"{kind} {form}: status {status}, expected {want}")
            if kind == "under":
                largest = _largest_decoded(desc, save, c.n * c.s)
                line += f", act_max {act_max!r} / largest decoded {largest!r} = 1 + {act_max / largest - 1.0:.3e}"
                if not largest <= act_max <= (1.0 + 2.0 ** -9) * largest:
                    problems.append(f"{kind} {form}: act_max {act_max!r} against the largest decoded value {largest!r}")
                rr.judge(buf.rows, c.raw64, c.raw32, rr.groups(variant, classes, endpoint), f"train {name} {site} {form}", problems)
            print(line)
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# d. the persistent loops
# ---------------------------------------------------------------------------------------------------------------------
LOOPS = [("object", 0, "dual", "loop-2wg", 64), ("ssr", 5, "default", "loop-2wg", 64), ("object", 0, "single", "loop-1wg", 64),
         ("object", 0, "default", "loop-t128", 128), ("ssr", 5, "t128", "loop-t128", 128)]


@pytest.mark.parametrize("site", ["pts_linears.3", "albedo_linear1"])
@pytest.mark.parametrize("variant,classes,form,points,tile", [pytest.param(*row, id=f"{row[0]}-{row[2]}-{row[3]}") for row in LOOPS])
def test_persistent_loops(variant, classes, form, points, tile, site, monkeypatch):
    """More tiles than persistent workgroups (the loop's second trip, a ragged last tile): offenders among the rays of the first three tiles
    only - the words of every later tile stay clear (a maximum kept across a trip would set them) - and in the last three tiles only -
    exactly their words are set (a maximum lost across a trip would clear them).  The expectation is E_all of the ramp: nothing of the
    tile-to-workgroup order goes into it."""
    print()
    dev = torch.device("cuda:0")
    p = _points(points)
    n, s = rr.split(p)
    status_rays = 128
    div = 10.0 if variant == "ssr" else 1.0
    desc = rr.desc_of(variant, classes, _capi.PREC_F16X3)
    packed = packing.pack_state_dict(desc, rg.wire(variant, classes, rr.weights(variant, classes, "sharp"), site, rg.GAIN)).to(dev)
    first_point = torch.arange(n) * s
    problems = []
    for where, offenders in (("first", first_point + s <= 3 * tile), ("last", first_point >= p - 3 * tile)):
        offenders = offenders & (torch.arange(n) % 2 == 0) if int(offenders.sum()) > 2 else offenders
        assert bool(offenders.any())
        rays, z, expect = rg.wire_words(n, s, div, status_rays, offenders, seed=3)
        assert bool(expect.any()) and not bool(expect.all())
        _set_env(monkeypatch, FORMS[form])
        buf, got, intact = _run(desc, packed, rays.to(dev), z.to(dev), 0, status_rays)
        print(f"{TAG} {variant}{classes or ''} {site} {form} {points} ({p} points = {n} x {s}) offenders in the {where} tiles: words expected {_bits(expect)} got {_bits(got)}")
        if got.tolist() != expect.tolist() or not intact:
            problems.append(f"{where}: words {_bits(got)}, expected {_bits(expect)}, sentinels intact: {intact}")
    assert not problems, "; ".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# e. the grid kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site", ["pts_linears.0", "pts_linears.4", "pts_linears.5", "pts_linears.7"])
@pytest.mark.parametrize("variant,classes", [("object", 0), ("ssr", 5)])
def test_grid_kernel(variant, classes, site):
    """kernels.occupancy_grid (kGridTrunk) on a 16^3 lattice whose ramp coordinate grows along the lattice order: the words per
    status_points = 128 are those of the lattice points whose fp64 slot is beyond the limit at the site."""
    print()
    dev = torch.device("cuda:0")
    div = 10.0 if variant == "ssr" else 1.0
    t, scale, m = rg.lattice(div)
    pts = kernels.grid_points(t, scale, m)
    value, others = rg.lattice_site_value(variant, classes, site, pts)
    assert others <= rg.OTHERS and not bool(((value.abs() / rg.LIMIT - 1.0).abs() <= rg.BAND).any())
    words = pts.shape[0] // 128
    expect = (value.abs() > rg.LIMIT).reshape(words, 128).any(1)
    assert bool(expect.any()) and not bool(expect.all())
    desc = rr.desc_of(variant, classes, _capi.PREC_F16X3)
    packed = packing.pack_state_dict(desc, rg.wire(variant, classes, rr.weights(variant, classes, "sharp"), site, rg.GAIN)).to(dev)
    status = torch.full((words + STATUS_GUARD,), STATUS_SENTINEL, dtype=torch.int32, device=dev)
    status[:words] = 0
    kernels.occupancy_grid(desc, packed, t.to(dev), scale, m, 0.01, status=status, status_points=128)
    _sync()
    got = status.cpu()
    print(f"{TAG} grid {variant}{classes or ''} {site}: {int((value.abs() > rg.LIMIT).sum())} points beyond the limit, words expected {_bits(expect)} got {_bits(got[:words] != 0)}")
    assert bool((got[words:] == STATUS_SENTINEL).all())
    assert (got[:words] != 0).tolist() == expect.tolist()
