"""Host side of the mean-shift fit (no GPU): the bandwidth subsample the library receives, and argument checks of the C
ABI that return before anything is launched."""
import ctypes as C

import numpy as np
import pytest


def test_sample_indices_follow_sklearn_permutation():
    from intrinsicnerf_amd.cluster import sample_indices
    counts = [0, 1, 7, 5000, 12345]
    idx, begin = sample_indices(counts, n_samples=5000)
    assert begin.tolist() == [0, 0, 1, 8, 5008, 10008] and idx.dtype == np.int32
    for c, n_c in enumerate(counts):
        want = np.random.RandomState(0).permutation(n_c)[:5000] if n_c else np.zeros(0)
        assert np.array_equal(idx[begin[c]:begin[c + 1]], want)
    # the class's stable order: indices select from the class's pixels in their original order (labels == c)
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 3, 20000)
    pixels = rng.random((20000, 3)).astype(np.float32)
    idx, begin = sample_indices(np.bincount(labels, minlength=3), n_samples=5000)
    for c in range(3):
        X = pixels[labels == c]
        want = X[np.random.RandomState(0).permutation(X.shape[0])[:5000]]
        assert np.array_equal(X[idx[begin[c]:begin[c + 1]]], want)


def test_abi_rejects_bad_arguments():
    from intrinsicnerf_amd import _capi
    lib = _capi.lib()
    assert lib.inerf_cluster_fit_workspace_bytes(0, 1, 0) == _capi.E_INVALID
    assert lib.inerf_cluster_fit_workspace_bytes(100, 0, 10) == _capi.E_INVALID
    assert lib.inerf_cluster_fit_workspace_bytes(100, 256, 10) == _capi.E_INVALID
    assert lib.inerf_cluster_fit_workspace_bytes(100, 3, 100) > 0
    assert lib.inerf_cluster_fit(None, None) == _capi.E_INVALID
    fake = 1 << 20                                                  # never dereferenced: every call below fails its checks first
    good = dict(pixels=fake, labels=None, n_pixels=100, n_classes=1, max_class_samples=100, sample_idx=fake, sample_begin=fake,
                n_sample_idx=100, factor=fake, quantile=0.3, band_factor=0.5, workspace=fake, workspace_bytes=0,
                out_bandwidth=fake, out_centers=fake, out_center_begin=fake, out_anchors=fake, out_links=fake,
                out_anchor_begin=fake, status=fake)
    bad = [dict(pixels=None), dict(n_pixels=0), dict(n_classes=0), dict(quantile=0.0), dict(quantile=1.5),
           dict(band_factor=0.0), dict(band_factor=float("nan")), dict(status=None), dict(out_anchors=None), dict(sample_idx=None)]
    for b in bad:
        a = _capi.ClusterFitArgs(**{**good, **b})
        assert lib.inerf_cluster_fit(C.byref(a), None) == _capi.E_INVALID, b
    for b in [dict(n_classes=300), dict(max_class_samples=9000), dict(n_pixels=1 << 25)]:
        a = _capi.ClusterFitArgs(**{**good, **b})
        assert lib.inerf_cluster_fit(C.byref(a), None) == _capi.E_UNSUPPORTED, b
    a = _capi.ClusterFitArgs(**good)                                # workspace_bytes 0: too small
    assert lib.inerf_cluster_fit(C.byref(a), None) == _capi.E_WORKSPACE


def test_cpu_device_raises_before_any_launch():
    import intrinsicnerf_amd.cluster as ic
    with pytest.raises(RuntimeError):
        ic.fit(np.full((4, 3), 0.5, np.float32), None, 1, [0.5], device="cpu")
