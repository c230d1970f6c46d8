"""GPU: the probe path without records: probe kernel -> listed WHOLE kernel, k_mlp_gate_whole_listed_f16x3.

A candidate takes the exact trunk and the heads in one tile body; nothing but the candidate list and the probe's (s, S) is kept per
point.  Every launch is held four ways - ungated, the gate alone, the fused probe path, and INERF_GATE_FUSED=0 (probe -> listed trunk ->
heads of the survivors' records, the path this one replaced): raw rows, rendered maps, range words, margin state and logged counts of
the two probe paths are equal bit for bit, a surviving row is the ungated kernel's, and a candidate with sigma <= 0 - whose heads are
now evaluated and thrown away - carries the exact sigma, zero colours and no range flag.  Equality is ``torch.equal`` on the bits."""
import re

import pytest
import torch

import _gate_probe as gp
import test_gate_probe_gpu as tp

pytestmark = pytest.mark.gpu

COLOURS = tp.COLOURS
S_C, S_I = tp.S_C, tp.S_I


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("INERF_PRECISION", "INERF_F16_KERNEL", "INERF_GATE", "INERF_PROBE", "INERF_PROBE_WG", "INERF_GATE_LOG", "INERF_ENC_CACHE",
              "INERF_GATE_BYTES", "INERF_GATE_FUSED", "INERF_PROBE_ADAPT", "INERF_PROBE_MIN_OBS"):
        monkeypatch.delenv(k, raising=False)


def _four_ways(monkeypatch, c, packed, rays, z, **kw):
    """(ungated, gate alone, fused probe path, INERF_GATE_FUSED=0, probe_out [n, 2])"""
    from intrinsicnerf_amd import kernels
    plain, gated, fused, po = tp._three_ways(c, packed, rays, z, **kw)
    monkeypatch.setenv("INERF_GATE_FUSED", "0")
    kw = {k: (torch.zeros_like(v) if k == "status" else v) for k, v in kw.items()}
    parent = kernels.encode_mlp(c["desc"], packed, rays, z, gate_colour=True, gate_probe=True, **kw).reshape(-1, 11)
    torch.cuda.synchronize()
    monkeypatch.delenv("INERF_GATE_FUSED")
    return plain, gated, fused, parent, po


def _assert_four(plain, gated, fused, parent, po):
    """Fused rows are the parent path's; the statements of tests/test_gate_probe_gpu.py about them; what a candidate that does not
    survive carries.  Returns (candidate mask, candidates that do not survive)."""
    assert torch.equal(tp._bits(fused), tp._bits(parent))
    cand = tp._assert_rows(plain, gated, fused, po)
    dead = cand & (plain[:, 3] <= 0)
    assert torch.equal(tp._bits(fused[dead][:, 3]), tp._bits(plain[dead][:, 3]))
    assert int((tp._bits(fused[dead][:, COLOURS]) != 0).sum()) == 0
    return cand, dead


@pytest.mark.parametrize("n_rays,n_samples,rays_per_sub", [(171, 193, 40), (37, 64, 12)])
def test_raw_rows(monkeypatch, n_rays, n_samples, rays_per_sub):
    """171 x 193: 258 tiles with a ragged last one, in five sub-ranges (the last of 11 rays); 37 x 64 in four."""
    c = tp._setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(rays_per_sub * n_samples * 1028))
    rays = tp._frame_rays(c, n_rays)
    z = gp.sample_depths(rays.cpu(), n_samples, seed=23).to(c["dev"])
    cand, dead = _assert_four(*_four_ways(monkeypatch, c, tp._pack(c, c["sd_f"]), rays, z))
    print(f"{n_rays} x {n_samples}: {int(cand.sum())} candidates, {int(dead.sum())} of them do not survive")
    assert int(dead.sum()) > 0 and int(dead.sum()) < int(cand.sum())


@pytest.mark.parametrize("target", [255, 256, 257])
def test_candidate_count_at_the_tile_boundary(monkeypatch, target):
    """The construction of tests/test_gate_probe_gpu.py: the prefix of 3 072 one-sample rays that holds exactly ``target`` candidates."""
    c = tp._setup()
    packed = tp._pack(c, tp._with_alpha_bias(c["sd_f"], 1.0))
    rays, z = tp._point_rays(c, 3072)
    if "prefix" not in tp._cache:
        _, _, _, po = tp._three_ways(c, packed, rays, z)
        tp._cache["prefix"] = (~(po[:, 0] < -gp.KAPPA * po[:, 1])).long().cumsum(0)
    count = tp._cache["prefix"]
    assert int(count[-1]) >= 257, int(count[-1])
    n = int(torch.nonzero(count == target)[0]) + 1
    cand, _ = _assert_four(*_four_ways(monkeypatch, c, packed, rays[:n].contiguous(), z[:n].contiguous()))
    assert int(cand.sum()) == target and bool(cand[-1])


@pytest.mark.parametrize("case", ["none", "all"])
def test_no_candidate_and_all_candidates(monkeypatch, case):
    c = tp._setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(12 * 64 * 1028))
    rays = tp._frame_rays(c, 37)
    z = gp.sample_depths(rays.cpu(), 64, seed=5).to(c["dev"])
    packed = tp._pack(c, tp._with_alpha_bias(c["sd_f"], -1.0e4 if case == "none" else 1.0e4))
    cand, _ = _assert_four(*_four_ways(monkeypatch, c, packed, rays, z))
    assert int(cand.sum()) == (0 if case == "none" else cand.numel())


@pytest.mark.parametrize("n_rays,n_samples", [(1, 1), (37, 64)])
def test_one_point_and_a_nan_density(monkeypatch, n_rays, n_samples):
    """A NaN weight in alpha_linear: every point is a candidate and a survivor, and its colours are not NaN.  A launch of ONE point,
    and 37 x 64 in four sub-ranges."""
    c = tp._setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(12 * 64 * 1028))
    sd = {k: v.clone() for k, v in c["sd_f"].items()}
    sd["alpha_linear.weight"][0, 5] = float("nan")
    rays = tp._frame_rays(c, 37)[:n_rays].contiguous()
    z = gp.sample_depths(rays.cpu(), n_samples, seed=9).to(c["dev"])
    plain, gated, fused, parent, po = _four_ways(monkeypatch, c, tp._pack(c, sd), rays, z)
    assert bool(torch.isnan(plain[:, 3]).all()) and not bool(torch.isnan(plain[:, COLOURS]).any())
    cand, dead = _assert_four(plain, gated, fused, parent, po)
    assert bool(cand.all()) and int(dead.sum()) == 0
    assert bool(torch.isnan(fused[:, 3]).all()) and not bool(torch.isnan(fused[:, COLOURS]).any())


def test_one_point_of_the_unchanged_network(monkeypatch):
    c = tp._setup()
    rays = tp._frame_rays(c, 37)[:1].contiguous()
    z = gp.sample_depths(rays.cpu(), 1, seed=9).to(c["dev"])
    _assert_four(*_four_ways(monkeypatch, c, tp._pack(c, c["sd_f"]), rays, z))


@pytest.mark.parametrize("white", [True, False])
def test_rendered_maps(monkeypatch, white):
    c = tp._setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(12 * 64 * 1028))      # 4 coarse sub-ranges, 10 fine ones
    fused = tp._render(c, white=white)
    monkeypatch.delenv("INERF_GATE_BYTES")
    one_sub = tp._render(c, white=white)
    monkeypatch.setenv("INERF_GATE_BYTES", str(12 * 64 * 1028))
    monkeypatch.setenv("INERF_GATE_FUSED", "0")
    parent = tp._render(c, white=white)
    monkeypatch.delenv("INERF_GATE_FUSED")
    monkeypatch.setenv("INERF_PROBE", "0")
    gate = tp._render(c, white=white)
    monkeypatch.setenv("INERF_GATE", "0")
    plain = tp._render(c, white=white)
    for other in (parent, gate, plain, one_sub):
        tp._assert_maps_equal(fused, other)
    assert int(fused["status"].max()) == 0 and int(one_sub["status"].max()) == 0


def test_range_flag(monkeypatch):
    """Unit 3 of albedo_linear1 becomes the constant 1e4: scaled by 8 it passes the guard's 6e4 on every point whose heads are
    evaluated.  37 rays of 8 samples each, one status word per 8 rays: the rays of words 0, 2 and 4 take the eight of their 64 depths with the
    non-positive densities nearest to zero (no survivor, but candidates of the probe), those of words 1 and 3 the eight
    with the largest.  The fused path evaluates the heads of every candidate and must flag the survivors' rays alone."""
    from intrinsicnerf_amd import kernels
    c = tp._setup()
    rays = tp._frame_rays(c, 37)
    z64 = gp.sample_depths(rays.cpu(), 64, seed=11).to(c["dev"])
    sigma = kernels.encode_mlp(c["desc"], tp._pack(c, c["sd_f"]), rays, z64)[..., 3]
    largest = sigma.topk(8, -1).indices
    nearest_below = torch.where(sigma <= 0, sigma, torch.full_like(sigma, float("-inf"))).topk(8, -1).indices
    live_ray = ((torch.arange(37, device=c["dev"]) // 8) % 2 == 1)[:, None]
    z = torch.where(live_ray, z64.gather(1, largest), z64.gather(1, nearest_below)).contiguous()
    words = -(-37 // 8)
    hot = {k: v.clone() for k, v in c["sd_f"].items()}
    hot["albedo_linear1.weight"][3].zero_()
    hot["albedo_linear1.bias"][3] = 1.0e4
    for net, flagged in ((hot, True), (c["sd_f"], False)):
        packed = tp._pack(c, net)
        st = {}
        for path in ("fused", "parent"):
            if path == "parent":
                monkeypatch.setenv("INERF_GATE_FUSED", "0")
            st[path] = torch.zeros(words, dtype=torch.int32, device=c["dev"])
            po = torch.full((z.numel(), 2), float("nan"), device=c["dev"])
            raw = kernels.encode_mlp(c["desc"], packed, rays, z, gate_colour=True, gate_probe=True, status=st[path], status_rays=8, probe_out=po)
            torch.cuda.synchronize()
            monkeypatch.delenv("INERF_GATE_FUSED", raising=False)
        survivors = (~(raw[..., 3] <= 0)).reshape(37, 8).any(-1)
        listed = (~(po[:, 0] < -gp.KAPPA * po[:, 1])).reshape(37, 8).any(-1)
        print("status words:", st["fused"].tolist(), "parent path:", st["parent"].tolist(), "rays with a survivor:", int(survivors.sum()),
              "with a candidate:", int(listed.sum()))
        assert torch.equal(st["fused"], st["parent"])
        if flagged:
            assert bool(survivors[8:16].all()) and not bool(survivors[:8].any()) and bool(listed[:8].any())      # the construction holds
            assert bool((st["parent"] != 0).any()) and bool((st["parent"] == 0).any())
            assert (st["fused"] != 0).tolist() == [False, True, False, True, False]
        else:
            assert int(st["fused"].max()) == 0


def _gate_counts(capfd):
    lines = tp._gate_lines(capfd)
    assert len(lines) == 1, lines
    m = re.search(r"in (\d+) sub-launches, (\d+) of (\d+) points survive .*?, (\d+) are the probe's candidates", lines[0])
    assert m, lines[0]
    return dict(zip(("sub", "kept", "points", "cand"), map(int, m.groups())))


def test_margin_state_and_logged_counts(monkeypatch, capfd):
    """One pass on a fresh state per path: the same r_max (bits), observed and counts; a second pass then culls with the same margin."""
    from intrinsicnerf_amd import kernels
    c = tp._setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(40 * 193 * 1028))
    monkeypatch.setenv("INERF_GATE_LOG", "1")
    monkeypatch.setenv("INERF_PROBE_MIN_OBS", "1")
    rays = tp._frame_rays(c, 171)
    z = gp.sample_depths(rays.cpu(), 193, seed=23).to(c["dev"])
    packed = tp._pack(c, c["sd_f"])
    got = {}
    for path in ("fused", "parent"):
        if path == "parent":
            monkeypatch.setenv("INERF_GATE_FUSED", "0")
        state = torch.zeros(8, dtype=torch.int32, device=c["dev"])
        capfd.readouterr()
        first = kernels.encode_mlp(c["desc"], packed, rays, z, gate_colour=True, gate_probe=True, gate_state=state)
        torch.cuda.synchronize()
        counts = _gate_counts(capfd)
        words = state.clone()
        second = kernels.encode_mlp(c["desc"], packed, rays, z, gate_colour=True, gate_probe=True, gate_state=state)
        torch.cuda.synchronize()
        got[path] = (counts, words, kernels.gate_margin(words), first, second, _gate_counts(capfd), state.clone())
    (cf, wf, mf, f1, f2, cf2, sf), (cp, wp, mp, p1, p2, cp2, sp) = got["fused"], got["parent"]
    print("fused:", cf, mf, "second pass:", cf2)
    assert cf == cp and cf2 == cp2 and cf["sub"] == 5
    assert 0 < mf["observed"] <= cf["cand"] and 0 < cf["kept"] < cf["cand"] < cf["points"]
    assert torch.equal(wf, wp) and torch.equal(sf, sp)                     # r_max bits, kappa_in_use, observed, launches
    assert torch.equal(tp._bits(f1), tp._bits(p1)) and torch.equal(tp._bits(f2), tp._bits(p2))
    assert cf2["cand"] <= cf["cand"]                                       # the measured margin (<= 2^-6 on this network) is in use in the second pass


def test_default_sub_range(monkeypatch, capfd):
    """INERF_GATE_BYTES unset: 11 000 x 192 = 2.11 M points are more than one sub-range of the record paths and ONE of this one."""
    c = tp._setup()
    monkeypatch.setenv("INERF_GATE_LOG", "1")
    rays = c["rays"].repeat(3, 1)[:11000].contiguous()
    z = gp.sample_depths(rays.cpu(), 192, seed=31).to(c["dev"])
    capfd.readouterr()
    plain, gated, fused, po = tp._three_ways(c, tp._pack(c, c["sd_f"]), rays, z)
    lines = tp._gate_lines(capfd)
    assert len(lines) == 2, lines
    assert "in 2 sub-launches" in lines[0] and "candidates" not in lines[0], lines[0]      # the gate alone
    assert "in 1 sub-launches" in lines[1] and "candidates" in lines[1], lines[1]
    cand = tp._assert_rows(plain, gated, fused, po)
    dead = cand & (plain[:, 3] <= 0)
    assert int(dead.sum()) > 0
    assert torch.equal(tp._bits(fused[dead][:, 3]), tp._bits(plain[dead][:, 3])) and int((tp._bits(fused[dead][:, COLOURS]) != 0).sum()) == 0


def test_workspace(monkeypatch):
    """Without records the probe path's workspace is below the gate's by at least 1 024 B per point of a sub-range, on the default
    sub-ranges and on forced ones; ``kernels.encode_mlp`` allocates exactly the figure, and such a launch runs."""
    from intrinsicnerf_amd import _capi
    c = tp._setup()
    lib = _capi.lib()
    gate, probe = _capi.FLAG_GATE_COLOUR, _capi.FLAG_GATE_COLOUR | _capi.FLAG_GATE_PROBE
    for n_rays, n_samples, rays_per_sub in ((171, 193, None), (171, 193, 40), (640000, 192, None)):
        if rays_per_sub is not None:
            monkeypatch.setenv("INERF_GATE_BYTES", str(rays_per_sub * n_samples * 1028))
        sub_points = (rays_per_sub or min(n_rays, (2 * 2 ** 30 // 1028) // n_samples)) * n_samples
        ws_gate = int(lib.inerf_encode_mlp_workspace_bytes(c["desc"], n_rays, n_samples, gate))
        ws_probe = int(lib.inerf_encode_mlp_workspace_bytes(c["desc"], n_rays, n_samples, probe))
        monkeypatch.setenv("INERF_GATE_FUSED", "0")
        ws_parent = int(lib.inerf_encode_mlp_workspace_bytes(c["desc"], n_rays, n_samples, probe))
        monkeypatch.delenv("INERF_GATE_FUSED")
        monkeypatch.delenv("INERF_GATE_BYTES", raising=False)
        print(f"{n_rays} x {n_samples}, {rays_per_sub} rays per sub-range: gate {ws_gate}, probe {ws_probe}, INERF_GATE_FUSED=0 {ws_parent} B")
        assert ws_parent == ws_gate                                        # the record paths share one plan
        if n_rays == 640000:       # the bench frame's fine pass, ONE sub-range here and 59 of the gate's: 12 B per point and the scratch
            assert 0 < ws_probe < min(ws_gate, 12 * n_rays * n_samples + 2 ** 24)
        else:                      # the same sub-ranges on both paths
            assert 0 < ws_probe <= ws_gate - 1024 * sub_points
    monkeypatch.setenv("INERF_GATE_BYTES", str(40 * 193 * 1028))
    rays = tp._frame_rays(c, 171)
    z = gp.sample_depths(rays.cpu(), 193, seed=23).to(c["dev"])
    tp._assert_rows(*tp._three_ways(c, tp._pack(c, c["sd_f"]), rays, z))
