"""CPU checks of the status centres (include/lsr_centers.h, language_centers.py): the numpy
restatement that the GPU tests compare against does what the header says (planted clusters, margins,
sklearn where installed), the time generator restated in integers has the stated properties, and the
'fine-base' initialisation, plain torch, has the reference's shape and noise."""
import numpy as np
import pytest
import torch

import centers_cases as cc


@pytest.mark.parametrize("shape", cc.SEPARATED, ids=str)
def test_restatement_recovers_planted_clusters(shape):
    P, S, D, K = shape
    x, sizes = cc.separated_case(P, S, D, K)
    assert np.abs(np.linalg.norm(x, axis=2) - 1).max() < 1e-6
    centers, counts, inertia, iters, assign = cc.separated_ref(P, S, D, K)
    assert np.array_equal(np.sort(counts, axis=1), np.tile(np.sort(sizes), (P, 1)))
    assert (iters >= 1).all() and (iters <= 3).all()
    # what makes these cases safe to compare on the GPU: no sample sits near a boundary
    gap, a64 = cc.margins(x, centers)
    assert gap.min() > 1e-3
    assert np.array_equal(a64, assign)
    assert inertia.max() < S * 0.02 ** 2


@pytest.mark.parametrize("shape", cc.SEPARATED, ids=str)
def test_restatement_matches_sklearn_on_separated_data(shape):
    cluster = pytest.importorskip("sklearn.cluster")
    P, S, D, K = shape
    x, _ = cc.separated_case(P, S, D, K)
    centers = cc.separated_ref(P, S, D, K)[0]
    for p in range(min(P, 8)):
        km = cluster.KMeans(n_clusters=K, n_init=10, random_state=0).fit(x[p].astype(np.float64))
        want = km.cluster_centers_[np.lexsort(km.cluster_centers_.T[::-1])]
        got = centers[p][np.lexsort(centers[p].T[::-1])]
        assert np.abs(got - want).max() < 1e-5


@pytest.mark.parametrize("shape", cc.UNSEPARATED, ids=str)
def test_restatement_stays_within_the_low_margin_cap(shape):
    """The GPU test ignores samples whose two nearest centres differ by less than LOW_MARGIN in d^2 and
    allows LOW_MARGIN_SHARE of them: on these seeds the restatement itself stays within that cap."""
    P, S, D, K = shape
    x = cc.unseparated_case(P, S, D)
    centers, counts, inertia, iters, assign = cc.kmeans_ref(x, K)
    gap, a64 = cc.margins(x, centers)
    low = gap < cc.LOW_MARGIN
    assert low.mean() <= cc.LOW_MARGIN_SHARE
    assert np.array_equal(a64[~low], assign[~low])
    assert (counts.sum(axis=1) == S).all() and (iters <= 100).all() and (iters >= 1).all()


def test_restatement_degenerate_rows():
    x0 = np.array([0.6, -0.8, 0.1], np.float32)
    c, n, inertia, it, _ = cc.kmeans_ref(np.tile(x0, (2, 7, 1)), 3)
    assert np.array_equal(c, np.tile(x0, (2, 3, 1))) and np.array_equal(n, [[7, 0, 0]] * 2)
    assert (inertia == 0).all() and (it == 1).all()
    x = np.eye(4, dtype=np.float32)[None]
    c, n, inertia, it, _ = cc.kmeans_ref(x, 4)
    assert sorted(map(tuple, c[0])) == sorted(map(tuple, x[0])) and (n == 1).all() and inertia[0] == 0 and it[0] == 1
    _, _, _, it, _ = cc.kmeans_ref(cc.unseparated_case(64, 100, 6), 8, max_iter=1)
    assert (it == 1).all()


def test_time_generator_restatement():
    t = cc.times_ref(0, 1000, 100)
    assert t.dtype == np.float32 and t.min() >= 0 and t.max() < 1
    scaled = t.astype(np.float64) * 2 ** 24
    assert np.array_equal(scaled, np.round(scaled))                       # multiples of 2^-24
    assert abs(float(t.astype(np.float64).mean()) - 0.5) < 0.01           # 10^5 draws
    assert len({tuple(r) for r in t}) == 1000                             # another row for every g
    other = cc.times_ref(1, 1000, 100)
    assert not (t == other).all(axis=1).any()                             # and for another seed
    assert np.array_equal(cc.times_ref(0, 1000, 100)[37:39, 5:9], t[37:39, 5:9])
    assert np.array_equal(cc.times_ref(2 ** 32 + 5, 3, 4), cc.times_ref(5, 3, 4))


def test_init_centers_fine_base():
    from language_centers import init_centers
    P, D, k = 20000, 6, 3
    g = torch.Generator().manual_seed(3)
    lang = torch.randn(P, D, generator=g) * 2.5
    unit = lang / (lang.norm(dim=-1, keepdim=True) + 1e-9)
    a = init_centers(lang, k, "fine-base", generator=torch.Generator().manual_seed(11))
    b = init_centers(lang, k, "fine-base", generator=torch.Generator().manual_seed(11))
    assert a.shape == (P, k * D) and torch.equal(a, b)
    off = a.reshape(P, k, D) - unit[:, None]
    # P * D draws of N(0, 0.05) per centre: the mean within 5 standard errors, the std within 2 %
    for j in range(k):
        assert abs(float(off[:, j].mean())) < 5 * 0.05 / (P * D) ** 0.5
        assert abs(float(off[:, j].std()) - 0.05) < 0.02 * 0.05
    assert not torch.equal(off[:, 0], off[:, 1])
    wide = init_centers(lang, k, "fine-base", noise_std=0.2, generator=torch.Generator().manual_seed(11))
    assert abs(float((wide.reshape(P, k, D) - unit[:, None]).std()) - 0.2) < 0.02 * 0.2
    perm = init_centers(lang, k, "fine-base", generator=torch.Generator().manual_seed(11), reference_permute=True)
    assert torch.equal(perm, a.reshape(P, k, D).permute(0, 2, 1).reshape(P, -1))
    with pytest.raises(ValueError, match="fine-base"):
        init_centers(lang, k, "coarse")
    with pytest.raises(ValueError, match="field is required"):
        init_centers(lang, k, "fine-lang")


def test_abi_refuses_out_of_range_arguments():
    """include/lsr_centers.h: every range is checked before the device is touched."""
    import ctypes
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                                    # never dereferenced: every call fails early
    km = lambda P, S, D, K, it=10: lib.lsr_centers_kmeans(p, P, S, D, K, it, p, p, p, p, None)   # noqa: E731
    err = lambda: lib.lsr_last_error().decode()   # noqa: E731
    for args, text in (((4, 10, 3, 0), "1 <= K <= 8"), ((4, 10, 3, 9), "1 <= K <= 8"), ((4, 2, 3, 3), "K <= S <= 256"),
                       ((4, 257, 3, 3), "K <= S <= 256"), ((4, 10, 33, 3), "1 <= D <= 32"), ((4, 10, 0, 3), "1 <= D <= 32"),
                       ((4, 10, 3, 3, 0), "max_iter >= 1"), ((-1, 10, 3, 3), "P >= 0")):
        assert km(*args) == 1 and text in err(), (args, err())
    assert km(0, 10, 3, 3) == 0                                # no rows: nothing is launched
    assert lib.lsr_centers_kmeans(None, 4, 10, 3, 3, 10, p, p, p, p, None) == 1 and "are required" in err()
    assert _lib.CENTERS_MAX_K == 8 and _lib.CENTERS_MAX_SAMPLES == 256 and _lib.CENTERS_MAX_DIM == 32
