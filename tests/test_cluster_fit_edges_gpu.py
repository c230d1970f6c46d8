"""Mean-shift fit of the albedo clusters on the GPU (csrc/cluster_fit.hip) at the sizes and inputs where it changes
behaviour: every case of tests/golden/cluster_fit_edges.npz (the reference on the real sklearn,
make_golden_cluster_fit_edges.py) through the shared checker, once against the fixture and once against the fp64 oracle
(oracle/cluster_fit.py); the subsample bound against the oracle alone; the class partition against single-class fits; labels
outside [0, K) against their removal.  Every fit runs twice and must be bit-equal."""
import numpy as np
import pytest
import torch

from _cluster_fit_check import (GOLD_EDGES, _attach, _check_class, class_sets, edge_cases, edge_inputs, load, oracle_gold)
from oracle import cluster_fit as ocf

pytestmark = pytest.mark.gpu

EDGES = load(GOLD_EDGES)
SWEEP = [1, 2, 3, 4, 11, 12, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4999, 5000, 5001]
MULTI = ["multi_k6", "multi_k28", "multi_k255"]
OTHERS = [c for c in edge_cases(EDGES) if not c.startswith("sweep_n") and c not in MULTI]

_oracle = {}


def oracle_of(case, px, lab, K, factor, band_factor, n_samples=5000):
    if case not in _oracle:
        _oracle[case] = ocf.fit(px, lab, K, [factor] * K, band_factor=band_factor, n_samples=n_samples)
    return _oracle[case]


def _per_class(res):
    return res.centers + res.mapped_centers + res.center_counts + res.anchors + res.links


def assert_bit_equal(a, b, what):
    for x, y in zip(_per_class(a), _per_class(b)):
        assert (x is None and y is None) or torch.equal(x, y), what
    assert torch.equal(a.pixel_label, b.pixel_label), what
    assert a.bandwidth == b.bandwidth and np.array_equal(a.stats, b.stats), what


def fit_twice(px, lab, K, factor, band_factor, n_samples=5000):
    import intrinsicnerf_amd.cluster as ic
    a = ic.fit(px, lab, K, [factor] * K, band_factor=band_factor, n_samples=n_samples)
    b = ic.fit(px, lab, K, [factor] * K, band_factor=band_factor, n_samples=n_samples)
    assert_bit_equal(a, b, "two runs of one fit differ")
    return a


def run_case(case, fixture=True, inputs=None, n_samples=5000):
    """one case: fitted twice (bit-equal), every class against the fixture (when there is one) and the oracle."""
    px, lab, K, factor, band_factor = inputs or edge_inputs(EDGES, case)
    res = fit_twice(px, lab, K, factor, band_factor, n_samples)
    sets = class_sets(px, lab, K)
    res._labels = lab
    _attach(res, sets, [factor] * K)
    fits = oracle_of(case, px, lab, K, factor, band_factor, n_samples)
    og = oracle_gold(fits, case)
    for c, s in enumerate(sets):
        key = f"{case}_c{c}"
        if len(s) == 0:
            assert res.centers[c] is None and res.anchors[c] is None and res.stats[c].tolist() == [0, 0, 0, 0]
            assert f"{key}_bw" not in EDGES or not fixture
            continue
        assert int(res.stats[c, 0]) == len(s)
        if fixture:
            g = EDGES
            if f"{key}_bw_fp64" in EDGES:       # 4 to 11 pixels: the kernel is held to the fp64 bandwidth, not sklearn's fp32 one
                g = {**{k: v for k, v in EDGES.items() if k.startswith(key)}, f"{key}_bw": EDGES[f"{key}_bw_fp64"]}
            _check_class(g, key, s, factor, res, c)
        m = _check_class(og, key, s, factor, res, c)
        f = fits[c]
        assert int(res.stats[c, 2]) == int((f["seed_counts"] > 0).sum()), (key, "seeds that found a point")
        assert int(res.stats[c, 3]) == f["centers"].shape[0]
    return res, fits


@pytest.mark.parametrize("n", SWEEP)
def test_class_size_sweep(n):
    res, fits = run_case(f"sweep_n{n}")
    if n <= 4:                                      # bandwidth 0: one seed per bin of the floor, 0.01 exactly
        assert res.bandwidth[0] == 0.01 and fits[0]["floor_bound"]


@pytest.mark.parametrize("n", [8192, 8193])
def test_subsample_bound(n):
    g = torch.Generator().manual_seed(n)
    modes = torch.rand(5, 3, generator=g) * 0.7 + 0.15
    px = (modes[torch.randint(0, 5, (n,), generator=g)] * (torch.rand(n, 1, generator=g) * 0.6 + 0.6)
          + 0.02 * torch.randn(n, 3, generator=g)).clamp(0.01, 1.0).numpy()
    res, _ = run_case(f"sub8192_n{n}", fixture=False, inputs=(px, None, 1, 0.5, 0.5), n_samples=8192)
    assert res.sample_begin.tolist() == [0, 8192]


def test_subsample_above_bound_raises():
    import intrinsicnerf_amd.cluster as ic
    px = np.full((8193, 3), 0.5, np.float32)
    with pytest.raises(ValueError):
        ic.fit(px, None, 1, [0.5], n_samples=8193)


@pytest.mark.parametrize("case", MULTI)
def test_multi_class_layout(case):
    res, _ = run_case(case)
    if case == "multi_k6":
        assert res.centers[0] is None and res.centers[5] is None
    if case == "multi_k255":
        assert sum(x is not None for x in res.centers) == 6 and res.centers[254] is not None


def test_labels_outside_the_classes_are_ignored():
    import intrinsicnerf_amd.cluster as ic
    px, lab, K, factor, band_factor = edge_inputs(EDGES, "multi_k6")
    g = np.random.default_rng(5)
    n, extra = len(px), 300
    stray_px = g.uniform(0.05, 0.95, size=(extra, 3)).astype(np.float32)
    stray_lab = np.array([-1, K, 1 << 40], np.int64)[g.integers(0, 3, extra)]
    assert len(set(stray_lab.tolist())) == 3
    pos = np.sort(g.choice(n + extra, extra, replace=False))        # where the strays sit in the mixed input
    is_stray = np.zeros(n + extra, bool)
    is_stray[pos] = True
    mixed_px, mixed_lab = np.empty((n + extra, 3), np.float32), np.empty(n + extra, np.int64)
    mixed_px[is_stray], mixed_lab[is_stray] = stray_px, stray_lab
    mixed_px[~is_stray], mixed_lab[~is_stray] = px, lab
    clean = fit_twice(px, lab, K, factor, band_factor)
    mixed = fit_twice(mixed_px, mixed_lab, K, factor, band_factor)
    for x, y in zip(_per_class(clean), _per_class(mixed)):
        assert (x is None and y is None) or torch.equal(x, y)
    assert clean.bandwidth == mixed.bandwidth and np.array_equal(clean.stats, mixed.stats)
    pl = mixed.pixel_label.cpu().numpy()
    assert np.all(pl[is_stray] == -1) and np.array_equal(pl[~is_stray], clean.pixel_label.cpu().numpy())


@pytest.mark.parametrize("case", MULTI)
def test_partition_matches_single_class_fits(case):
    import intrinsicnerf_amd.cluster as ic
    px, lab, K, factor, band_factor = edge_inputs(EDGES, case)
    multi = ic.fit(px, lab, K, [factor] * K, band_factor=band_factor)
    pl = multi.pixel_label.cpu().numpy()
    for c in range(K):
        s = px[lab == c]                            # the class's pixels in their original order
        if len(s) == 0:
            assert multi.centers[c] is None
            continue
        one = ic.fit(s, None, 1, [factor], band_factor=band_factor)
        for name in ("centers", "mapped_centers", "center_counts", "anchors", "links"):
            assert torch.equal(getattr(multi, name)[c], getattr(one, name)[0]), (case, c, name)
        assert multi.bandwidth[c] == one.bandwidth[0] and np.array_equal(multi.stats[c], one.stats[0]), (case, c)
        assert np.array_equal(pl[lab == c], one.pixel_label.cpu().numpy()), (case, c, "labels")


@pytest.mark.parametrize("case", OTHERS)
def test_edge_case(case):
    res, fits = run_case(case)
    f, n = fits[0], int(res.stats[0, 0])
    one = lambda name: EDGES[f"{case}_c0_{name}"]
    if case in ("floor_identical", "floor_below"):
        assert res.bandwidth[0] == 0.01 and f["floor_bound"]
    if case == "floor_above":
        assert 0.01 < res.bandwidth[0] <= 0.0101 and not f["floor_bound"]
    if case == "seeds_all":
        assert int(res.stats[0, 1]) == n == 13 and f["seeds_are_points"]
    if case == "seeds_allbut1":
        assert int(res.stats[0, 1]) == n - 1 == 13 and not f["seeds_are_points"]
    if case in ("tie2", "tie3", "seeds_all"):       # equal counts: the centre tuples decide the order, centre for centre
        ours = res.mapped_centers[0].cpu().numpy()
        assert np.abs(ours - one("centers_mapped")).max() <= 5e-3 * res.bandwidth[0]
        assert res.center_counts[0].cpu().tolist() == one("counts").tolist() == f["center_counts"].tolist()
        assert [tuple(r) for r in ours.tolist()] == sorted((tuple(r) for r in ours.tolist()), reverse=True)
    if case.startswith("cand_"):
        assert int(res.stats[0, 2]) == int(case[5:]) == int(one("n_seeds"))
    if case == "floor_identical":
        assert res.stats[0].tolist() == [64, 1, 1, 1]
    if case == "anchor_dup":                        # ties between equal pixels: the lowest rank, as the oracle picks
        assert torch.equal(res.anchors[0].cpu(), torch.from_numpy(f["anchors"]))
        assert torch.equal(res.links[0].cpu(), torch.from_numpy(f["links"]))
    if case == "anchor_clamp":
        a = res.anchors[0].cpu().numpy()
        assert a.shape == one("anchors").shape and np.any(a[:, 1] == 1.0) and np.any(a[:, 2] == 1.0)
