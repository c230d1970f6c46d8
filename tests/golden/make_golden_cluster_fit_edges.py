#!/usr/bin/env python3
"""Golden vectors for the mean-shift fit at the sizes and inputs where csrc/cluster_fit.hip changes behaviour, from the
reference's own classes and the real sklearn (build container only; the tests read the .npz alone).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cluster_fit_edges.py

Same recipe and per-class keys as make_golden_cluster_fit.py (its ``Recorder`` is reused); cluster_fit.npz is not touched.
Cases (``cases`` in the file lists them; tests/golden/README.md):

  sweep_n<N>       one class of N pixels, N in SWEEP: slices of one stored pool (``sweep_pool``, ``_pool_off``, ``_n``)
  multi_k6         6 classes, the first and the last empty
  multi_k28        28 classes with sizes from the sweep, four of them empty
  multi_k255       255 classes over 5 121 pixels, six of them non-empty: (K+1) * chunks > 1 024, the second scan level
  floor_identical  64 equal pixels: bandwidth 0 -> the 0.01 floor, one bin, one candidate
  floor_below      a cloud scaled until estimate_bandwidth * band_factor lies within 1 % below 0.01 (floor binds);
                   band_factor 3.0 here and in floor_above
  floor_above      the same cloud scaled to within 1 % above 0.01 (floor does not bind)
  seeds_all        13 far-apart pixels, every bin holds one: n_seeds == n_c, the points themselves are the seeds;
                   13 centres of count 1 (the centre-tuple tie-break orders all of them)
  seeds_allbut1    the same 13 and a 14th in the bin of one of them: n_seeds == n_c - 1, bin centres are the seeds
  tie2, tie3       two / three far-apart clumps of 20 pixels, each one bin: 2 / 3 candidates with equal counts
  cand_129/257     129 / 257 isolated pixels, band_factor set for a window of 0.012: as many candidates as pixels, all of
                   count 1 (the bitonic sort of the candidates on a non-power-of-two length, ordered by the centre tuples
                   alone; 1, 2 and 3 candidates: floor_identical, tie2, tie3)
  anchor_dup       every pixel twice: every voxel's minimum distance ties
  anchor_clamp     pixels (0, g, 0) and (0, 0, b): a mapped coordinate of exactly 1.0, voxel id 100 clamps to 99

NOT a case: "a seed whose bin centre has no point within the bandwidth".  get_bin_seeds bins with bin_size = bandwidth, so
a point of a bin lies within bandwidth / 2 of the seed along each of the three axes, at most sqrt(3)/2 = 0.87 bandwidths
away (rounding moves that by parts in 1e7): in three dimensions every seed finds its own bin's points and no valid input
reaches a recorded count of 0.

Before anything is written, every recorded class must satisfy (a draw that does not is replaced by the next one, the
conditions stay):
  * no two pre-merge candidate centres at a distance within 1e-2 * bw of bw (an ulp in a trajectory cannot flip a merge);
  * at most 1e-3 * n_c pixels whose two nearest surviving centres are within 5e-3 * bw of each other in distance;
  * the edge the case is named after is hit, judged from the recorded values (asserted below, case by case).
For classes of 4 to 11 pixels both sklearn's bandwidth and the fp64 brute-force one (oracle/cluster_fit.py) are recorded;
``tiny_bw_rel`` is the worst relative difference between the two over the file.
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
from make_golden_cluster import albedo_samples  # noqa: E402
from make_golden_cluster_fit import Recorder  # noqa: E402
from oracle import cluster_fit as ocf  # noqa: E402

SWEEP = [1, 2, 3, 4, 11, 12, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4999, 5000, 5001]
K28_SIZES = [1, 2, 3, 4, 11, 12, 0, 63, 64, 65, 255, 256, 257, 0, 511, 512, 513, 1023, 1024, 1025, 0, 5, 100, 300, 7, 33, 0, 129]
FLOOR_BF = 3.0          # band_factor of the two scaled floor cases: the window covers the whole cloud, one robust centre
K255_SIZES = {0: 1500, 3: 1, 77: 2000, 128: 12, 200: 600, 254: 1008}


class Reject(Exception):
    pass


def sq(a, b):
    return np.sqrt(ocf.sq_dists(np.asarray(a, np.float64), np.asarray(b, np.float64)))


def conditions(f, X):
    """the two robustness conditions on one recorded fit (X = the mapped pixels of the class)."""
    bw, n_c = f["bw"], X.shape[0]
    cand = np.array(sorted({s[0] for s in f["seeds"] if s[1]}), np.float64).reshape(-1, 3)
    if len(cand) > 1:
        d = sq(cand, cand)[np.triu_indices(len(cand), 1)]
        if np.any(np.abs(d - bw) < 1e-2 * bw):
            raise Reject("two candidate centres at the merge radius")
    if n_c > 11 and len(f["centers"]) > 1:
        d = np.sort(sq(X, f["centers"]), axis=1)
        if int(np.sum(d[:, 1] - d[:, 0] < 5e-3 * bw)) > 1e-3 * n_c:
            raise Reject("too many pixels between two centres")


def interleave(rng, sets):
    px = np.concatenate([s for s in sets if len(s)])
    lab = np.concatenate([np.full(len(s), c, np.int64) for c, s in enumerate(sets) if len(s)])
    order = rng.permutation(len(px))
    return px[order], lab[order][:, None]


def main():
    mg.import_reference()
    from SSR.training import cluster as ref
    import sklearn.cluster
    torch.set_num_threads(1)            # choose_anchors' index_put must write in order (make_golden_cluster_fit.py)
    cpu = torch.device("cpu")
    ref.Cluster.__init__.__defaults__ = (cpu, 0.5, None)
    rec = Recorder(ref)
    out, cases = {}, []
    only = sys.argv[1:]                 # case names: a dry run of those cases alone, nothing is written

    def run(case, px, lab, K, band_factor, store_pixels=True):
        """the reference on one input; records every class under `case`, raises Reject when a condition fails."""
        rec.fits = []
        with contextlib.redirect_stdout(io.StringIO()):
            if K == 1:
                cl = ref.Cluster(device=cpu, intensity_factor=0.5)
                cl.update_center(px, band_factor=band_factor)
                clusters = [cl]
            else:
                mgr = ref.Cluster_Manager(class_num=K)
                mgr.update_center(lab, px, band_factor=band_factor)
                clusters = mgr.clusters
        sets = [px] if K == 1 else [px[lab.reshape(-1) == c] for c in range(K)]
        it, o, fits = iter(rec.fits), {}, []
        for c, cl in enumerate(clusters):
            if cl is None:
                assert len(sets[c]) == 0
                fits.append(None)
                continue
            f = next(it)
            X = ocf.mapping_color_np(sets[c], 0.5)
            conditions(f, X)
            k = f"{case}_c{c}"
            o[f"{k}_bw"] = np.float64(f["bw"])
            o[f"{k}_n_seeds"] = np.int64(f["n_seeds"])
            o[f"{k}_centers_mapped"] = f["centers"]
            o[f"{k}_labels"] = f["labels"]
            o[f"{k}_counts"] = f["counts"]
            o[f"{k}_seed_counts"] = np.array([s[1] for s in f["seeds"]], np.int32)
            o[f"{k}_anchors"] = cl.anchors.numpy().astype(np.float32)
            o[f"{k}_links"] = cl.links.numpy().astype(np.int64)
            o[f"{k}_rgb_centers"] = cl.rgb_centers.float().numpy()
            assert np.array_equal(o[f"{k}_anchors"], cl.anchors.numpy()) and cl.anchors.dtype == torch.float32
            if 4 <= len(sets[c]) <= 11:
                idx = np.random.RandomState(0).permutation(len(sets[c]))[:5000]
                exact = max(ocf.estimate_bandwidth(X, idx, 0.3) * band_factor, 0.01)
                o[f"{k}_bw_fp64"] = np.float64(exact)
            f["X"] = X
            fits.append(f)
        o[f"{case}_class_num"] = np.int64(K)
        o[f"{case}_band_factor"] = np.float64(band_factor)
        o[f"{case}_factor"] = np.float64(0.5)
        if store_pixels:
            o[f"{case}_pixels"] = px
        if K > 1:
            o[f"{case}_labels"] = lab.astype(np.int16 if K < 128 else np.int32)
        return o, fits

    def attempt(case, make, check=None, tries=200):
        """make(rng) -> (px, lab, K, band_factor[, extra]); the first draw that passes the conditions and `check` is kept."""
        if only and case not in only:
            return None, None
        for t in range(tries):
            rng = np.random.default_rng([20221016, len(cases), t])
            got = make(rng)
            try:
                o, fits = run(case, *got[:4], store_pixels=len(got) < 5 or got[4].get("store", True))
                if check is not None:
                    check(o, fits, got)
            except Reject as e:
                print(f"  {case}: draw {t} rejected ({e})", flush=True)
                continue
            if len(got) > 4:
                o.update({f"{case}_{k}": v for k, v in got[4].items() if k != "store"})
            out.update(o)
            cases.append(case)
            print(f"{case}: draw {t} kept", flush=True)
            return o, fits
        raise SystemExit(f"{case}: no draw in {tries} passed")

    def need(cond, why):
        if not cond:
            raise Reject(why)

    # ---- class-size sweep: slices of one pool
    pool = albedo_samples(np.random.default_rng(20221017), 5600, 4)
    out["sweep_pool"] = pool
    for n in SWEEP:
        def make(rng, n=n):
            off = int(rng.integers(0, len(pool) - n + 1)) if n < 5001 else int(rng.integers(0, 600))
            return pool[off:off + n], None, 1, 0.5, {"store": False, "pool_off": np.int64(off), "n": np.int64(n)}
        attempt(f"sweep_n{n}", make)

    # ---- multi-class layouts
    def class_draw(seed, c, s):
        """pixels of one class that pass the conditions on their own (the reference fits a manager class by class)."""
        if s == 0:
            return np.zeros((0, 3), np.float32)
        for t in range(400):
            px = albedo_samples(np.random.default_rng([seed, c, t]), s, 1 + (c % 4))
            try:
                run("_draw", px, None, 1, 0.5)
                return px
            except Reject:
                continue
        raise SystemExit(f"class {c} of {s} pixels: no draw passed")

    def multi(sizes):
        def make(rng):
            seed = int(rng.integers(1 << 30))
            sets = [class_draw(seed, c, s) for c, s in enumerate(sizes)]
            px, lab = interleave(rng, sets)
            return px, lab, len(sizes), 0.5
        return make
    attempt("multi_k6", multi([0, 257, 12, 1025, 63, 0]))
    attempt("multi_k28", multi(K28_SIZES))
    attempt("multi_k255", multi([K255_SIZES.get(c, 0) for c in range(255)]))
    assert sum(K255_SIZES.values()) == 5121 and 256 * ((5121 + 1023) // 1024) > 1024

    # ---- bandwidth floor
    def identical(rng):
        return np.tile(np.array([[0.4, 0.5, 0.3]], np.float32), (64, 1)), None, 1, 0.5

    def check_identical(o, fits, got):
        need(o["floor_identical_c0_bw"] == 0.01 and o["floor_identical_c0_n_seeds"] == 1, "floor / one seed")
        need(sklearn.cluster.estimate_bandwidth(fits[0]["X"], quantile=0.3, n_samples=5000) == 0.0, "bandwidth 0")
    attempt("floor_identical", identical, check_identical)

    def scaled(target):
        def make(rng):
            z = rng.normal(0, 1, size=(600, 3))
            cloud = lambda s: np.clip(np.array([0.4, 0.5, 0.3]) + s * z, 0.01, 1).astype(np.float32)
            est = lambda s: sklearn.cluster.estimate_bandwidth(ocf.mapping_color_np(cloud(s), 0.5), quantile=0.3, n_samples=5000) * FLOOR_BF
            lo, hi = 1e-4, 0.2
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if est(mid) < target else (lo, mid)
            return cloud(hi), None, 1, FLOOR_BF, {"bw_raw": np.float64(sklearn.cluster.estimate_bandwidth(
                ocf.mapping_color_np(cloud(hi), 0.5), quantile=0.3, n_samples=5000))}
        return make

    def check_below(o, fits, got):
        half = float(got[4]["bw_raw"]) * FLOOR_BF
        need(0.0099 <= half < 0.01 and o["floor_below_c0_bw"] == 0.01, f"not within 1 % below the floor: {half}")

    def check_above(o, fits, got):
        half = float(got[4]["bw_raw"]) * FLOOR_BF
        need(0.01 < half <= 0.0101 and o["floor_above_c0_bw"] == half, f"not within 1 % above the floor: {half}")
    attempt("floor_below", scaled(0.00995), check_below)
    attempt("floor_above", scaled(0.01005), check_above)

    # ---- seeds
    def lattice(rng, extra):
        pts = [(d0, d1, d2) for d0 in (0.1, 0.2) for d1 in (0.2, 0.3, 0.4) for d2 in (0.2, 0.3, 0.4)]
        d = np.array(pts)[rng.permutation(len(pts))[:13]] + rng.uniform(-0.004, 0.004, size=(13, 3))
        if extra:
            d = np.concatenate([d, d[5:6] + 0.002])
        I = d[:, 0] * 6.0                                           # the inverse mapping at intensity_factor 0.5
        g, b = d[:, 1] * I, d[:, 2] * I
        return np.stack([I - g - b, g, b], 1).astype(np.float32), None, 1, 0.5

    def check_all(o, fits, got):
        need(o["seeds_all_c0_n_seeds"] == 13, "n_seeds != n_c")
        need(len(o["seeds_all_c0_counts"]) == 13 and np.all(o["seeds_all_c0_counts"] == 1), "not 13 centres of count 1")

    def check_allbut1(o, fits, got):
        need(o["seeds_allbut1_c0_n_seeds"] == 13 and got[0].shape[0] == 14, "n_seeds != n_c - 1")
    attempt("seeds_all", lambda rng: lattice(rng, False), check_all)
    attempt("seeds_allbut1", lambda rng: lattice(rng, True), check_allbut1)

    # ---- merge order
    def clumps(m):
        def make(rng):
            ctr = np.array([[0.6, 0.2, 0.2], [0.2, 0.6, 0.2], [0.2, 0.2, 0.6]])[:m] + rng.uniform(-0.05, 0.05, size=(m, 3))
            px = np.concatenate([c + rng.normal(0, 4e-4, size=(20, 3)) for c in ctr]).astype(np.float32)
            return px[rng.permutation(len(px))], None, 1, 0.5
        return make

    def check_tie(m, case):
        def check(o, fits, got):
            need(o[f"{case}_c0_n_seeds"] == m and len(o[f"{case}_c0_counts"]) == m, "not one seed and one centre per clump")
            need(np.all(o[f"{case}_c0_counts"] == 20) and np.all(o[f"{case}_c0_seed_counts"] == 20), "counts not all equal")
        return check
    attempt("tie2", clumps(2), check_tie(2, "tie2"))
    attempt("tie3", clumps(3), check_tie(3, "tie3"))

    def cand(target):
        def make(rng):
            # `target` isolated pixels on a jittered lattice of the mapped space (spacing >= 0.03), band_factor chosen so that
            # the window is 0.012: every pixel is its own bin, its own candidate of count 1 and its own centre
            pts = [(d0, d1, d2) for d0 in (0.03, 0.06, 0.09, 0.12, 0.15) for d1 in np.arange(1, 9) * 0.05 for d2 in np.arange(1, 9) * 0.05]
            d = np.array(pts)[rng.permutation(len(pts))[:target]] + rng.uniform(-0.002, 0.002, size=(target, 3))
            I = d[:, 0] * 6.0
            g, b = d[:, 1] * I, d[:, 2] * I
            px = np.stack([I - g - b, g, b], 1).astype(np.float32)
            X = ocf.mapping_color_np(px, 0.5)
            raw = ocf.estimate_bandwidth(X, np.random.RandomState(0).permutation(target), 0.3)
            return px, None, 1, float(0.012 / raw)
        return make

    def check_cand(target, case):
        def check(o, fits, got):
            need(o[f"{case}_c0_n_seeds"] == target and np.all(o[f"{case}_c0_seed_counts"] > 0), f"not {target} candidates")
        return check
    attempt("cand_129", cand(129), check_cand(129, "cand_129"))
    attempt("cand_257", cand(257), check_cand(257, "cand_257"))

    # ---- anchors
    def dup(rng):
        px = albedo_samples(rng, 300, 3)
        return np.concatenate([px, px])[rng.permutation(600)], None, 1, 0.5

    def check_dup(o, fits, got):
        X = fits[0]["X"]
        need(len(np.unique(X, axis=0)) * 2 == len(X), "not every pixel twice")

    def clamp(rng):
        px = albedo_samples(rng, 400, 3)
        edge = np.zeros((16, 3), np.float32)
        edge[:8, 1] = rng.uniform(0.2, 0.9, 8)
        edge[8:, 2] = rng.uniform(0.2, 0.9, 8)
        return np.concatenate([px, edge])[rng.permutation(416)], None, 1, 0.5

    def check_clamp(o, fits, got):
        X, a = fits[0]["X"], o["anchor_clamp_c0_anchors"]
        need(int(np.sum(X[:, 1] == 1.0)) == 8 and int(np.sum(X[:, 2] == 1.0)) == 8, "no mapped coordinate of exactly 1.0")
        need(int(np.sum(a[:, 1] == 1.0)) >= 1 and int(np.sum(a[:, 2] == 1.0)) >= 1, "no anchor in a clamped voxel")
    attempt("anchor_dup", dup, check_dup)
    attempt("anchor_clamp", clamp, check_clamp)

    if only:
        return
    out["cases"] = np.array(cases)
    rel = [abs(float(out[k]) - float(out[k[:-5]])) / float(out[k]) for k in out if k.endswith("_bw_fp64")]
    assert len(rel) >= 4, "no class of 4 to 11 pixels recorded"
    out["tiny_bw_rel"] = np.float64(max(rel))
    path = os.path.join(HERE, "cluster_fit_edges.npz")
    np.savez_compressed(path, **out)
    for k in sorted(out):
        if k.endswith("_bw") or k.endswith("_n_seeds"):
            print(k, out[k], end="; ")
    print()
    print("tiny_bw_rel", out["tiny_bw_rel"])
    print("wrote cluster_fit_edges.npz", os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
