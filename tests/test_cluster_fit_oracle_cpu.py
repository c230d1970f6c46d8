"""The fp64 oracle of the mean-shift fit (oracle/cluster_fit.py) against the reference + sklearn fixtures: every class of
tests/golden/cluster_fit.npz and cluster_fit_edges.npz through the checker the GPU tests use, at the same tolerances
(bandwidth 1e-9 relative, seed and centre counts exact, centres within 5e-3 * bw one-to-one, rgb centres 1e-5, labels up
to near-ties, anchors bit-equal up to voxel-distance ties), and - where sklearn is installed - against sklearn live."""
import numpy as np
import pytest

from _cluster_fit_check import (GOLD, GOLD_EDGES, _check_class, class_sets, edge_cases, edge_inputs, load, oracle_result)
from oracle import cluster_fit as ocf


@pytest.fixture(scope="module")
def gold():
    return load(GOLD)


@pytest.fixture(scope="module")
def edges():
    return load(GOLD_EDGES)


def tiny_bound(edges):
    """classes of 4 to 11 pixels: the oracle's fp64 bandwidth against sklearn's, twice the worst relative difference the
    generator recorded over the fixture (tests/golden/README.md), and never below the 1e-9 every other class gets."""
    return max(1e-9, 2.0 * float(edges["tiny_bw_rel"]))


def _check_case(gold, case, px, lab, K, factor, band_factor, tiny_rel):
    fits = ocf.fit(px, lab, K, [factor] * K, band_factor=band_factor)
    res = oracle_result(fits)
    for c, s in enumerate(class_sets(px, lab, K)):
        key = f"{case}_c{c}"
        if len(s) == 0:
            assert fits[c] is None and f"{key}_bw" not in gold
            continue
        _check_class(gold, key, s, factor, res, c, bw_rel=tiny_rel if 4 <= len(s) <= 11 else 1e-9)
    return fits


@pytest.mark.parametrize("case", ["ssr_multi", "ssr_single", "cluster_f08"])
def test_oracle_reproduces_reference_fixture(gold, edges, case):
    px = gold[f"{case}_pixels"]
    if case == "cluster_f08":
        lab, K, factor = None, 1, float(gold["cluster_f08_factor"])
    else:
        K, factor = int(gold[f"{case}_class_num"]), 0.5
        lab = gold[f"{case}_labels"].reshape(-1) if K > 1 else None
    fits = _check_case(gold, case, px, lab, K, factor, float(gold[f"{case}_band_factor"]), tiny_bound(edges))
    if case == "ssr_multi":
        assert fits[1] is None and "ssr_multi_c1_none" in gold
        assert fits[3]["seeds_are_points"] and fits[4]["floor_bound"] and not fits[0]["floor_bound"]


def _edge_case_names():
    return edge_cases(load(GOLD_EDGES))


@pytest.mark.parametrize("case", _edge_case_names())
def test_oracle_reproduces_edge_fixture(edges, case):
    px, lab, K, factor, band_factor = edge_inputs(edges, case)
    fits = _check_case(edges, case, px, lab, K, factor, band_factor, tiny_bound(edges))
    for c, f in enumerate(fits):
        if f is None:
            continue
        # seed for seed (sklearn's dict order): the same seeds find a point, out of sklearn's fp32 brute-force path
        if f["mapped"].shape[0] > 11:
            ref = edges[f"{case}_c{c}_seed_counts"]
            assert ref.shape == f["seed_counts"].shape and np.array_equal(ref > 0, f["seed_counts"] > 0), (case, c)
        if f"{case}_c{c}_bw_fp64" in edges:         # the kernel's yardstick for these classes: fp64, at 1e-9
            exact = float(edges[f"{case}_c{c}_bw_fp64"])
            assert abs(f["bandwidth"] - exact) <= 1e-9 * exact


def test_edge_fixture_hits_its_edges(edges):
    """what the generator asserted before it wrote, read back from the file."""
    one = lambda case, name: edges[f"{case}_c0_{name}"]
    assert float(one("floor_identical", "bw")) == 0.01 and int(one("floor_identical", "n_seeds")) == 1
    raw = float(edges["floor_below_bw_raw"]) * float(edges["floor_below_band_factor"])
    assert 0.0099 <= raw < 0.01 and float(one("floor_below", "bw")) == 0.01
    raw = float(edges["floor_above_bw_raw"]) * float(edges["floor_above_band_factor"])
    assert 0.01 < raw <= 0.0101 and float(one("floor_above", "bw")) == raw
    assert int(one("seeds_all", "n_seeds")) == 13 == len(edges["seeds_all_pixels"])
    assert int(one("seeds_allbut1", "n_seeds")) == 13 == len(edges["seeds_allbut1_pixels"]) - 1
    for case, m in (("tie2", 2), ("tie3", 3)):
        assert one(case, "counts").tolist() == [20] * m and int(one(case, "n_seeds")) == m
    for case, m in (("cand_129", 129), ("cand_257", 257)):
        assert int(one(case, "n_seeds")) == m and int((one(case, "seed_counts") > 0).sum()) == m
    a = one("anchor_clamp", "anchors")
    assert np.any(a[:, 1] == 1.0) and np.any(a[:, 2] == 1.0)
    K = int(edges["multi_k255_class_num"])
    n = len(edges["multi_k255_pixels"])
    assert K == 255 and (K + 1) * ((n + 1023) // 1024) > 1024
    assert 0.0 <= float(edges["tiny_bw_rel"]) < 1e-3


def test_oracle_orders_equal_counts_by_centre_tuple(edges):
    for case in ("tie2", "tie3", "seeds_all"):
        px, lab, K, factor, band_factor = edge_inputs(edges, case)
        f = ocf.fit(px, lab, K, [factor], band_factor=band_factor)[0]
        assert len(set(f["center_counts"].tolist())) == 1
        tuples = [tuple(c) for c in f["centers"].tolist()]
        assert tuples == sorted(tuples, reverse=True)
        ref = edges[f"{case}_c0_centers_mapped"]
        assert np.abs(ref - f["centers"]).max() <= 5e-3 * f["bandwidth"]        # the same order, centre for centre


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_matches_sklearn_live(seed):
    skc = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(100 + seed)
    n = [300, 900, 1500][seed]
    base = rng.uniform(0.1, 0.9, size=(3 + seed, 3))
    px = np.clip(base[rng.integers(0, len(base), n)] * rng.uniform(0.6, 1.2, size=(n, 1)) + rng.normal(0, 0.02, size=(n, 3)),
                 0.01, 1.0).astype(np.float32)
    f = ocf.fit_class(px, 0.5, quantile=0.3, n_samples=5000, band_factor=0.5)
    X = f["mapped"]
    raw = skc.estimate_bandwidth(X, quantile=0.3, n_samples=5000)
    assert abs(f["bandwidth_raw"] - raw) <= 1e-9 * raw
    bw = max(raw * 0.5, 0.01)
    from sklearn.cluster._mean_shift import get_bin_seeds
    seeds = get_bin_seeds(X, bw, 1)
    # the same bins in the same order; the positions are bin * bw, and the two bandwidths agree to 1e-9
    assert seeds.shape == f["seeds"].shape and np.allclose(np.asarray(seeds, np.float64), f["seeds"], rtol=2e-9, atol=0.0)
    ms = skc.MeanShift(bandwidth=bw, bin_seeding=True).fit(X)
    assert ms.cluster_centers_.shape == f["centers"].shape
    d = np.sqrt(ocf.sq_dists(ms.cluster_centers_.astype(np.float64), f["centers"].astype(np.float64)))
    assert d.argmin(1).tolist() == list(range(len(d))) and float(d.diagonal().max()) <= 5e-3 * bw
