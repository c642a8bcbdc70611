"""Shared by tests/test_centers.py and tests/test_centers_gpu.py: the k-means of include/lsr_centers.h
restated in numpy (float32, the same order of every sum), the time generator restated in integer
numpy, and the case builders.  No reference output exists for this feature (the reference's
'fine-lang' branch cannot run as released), so the restatement is the yardstick."""
import functools

import numpy as np

F = np.float32

# (P, S, D, K) of the separated cases; the unseparated ones
SEPARATED = [(1, 3, 3, 3), (5, 100, 3, 3), (67, 100, 6, 3), (130, 64, 32, 8), (9, 65, 3, 1), (3, 256, 16, 8)]
UNSEPARATED = [(200, 100, 3, 3), (64, 100, 6, 8)]
LOW_MARGIN = 1e-5          # samples whose two nearest centres are this close in d^2 may go either way
LOW_MARGIN_SHARE = 0.01    # at most this share of all samples


def kmeans_ref(x, K, max_iter=100):
    """include/lsr_centers.h for every row of x [P, S, D]: (centers [P, K, D] float32, counts [P, K],
    inertia [P] float64 sum of the float32 distances, iters [P], assignment [P, S])."""
    x = np.asarray(x, F)
    P, S, D = x.shape
    rows = np.arange(P)

    def d2(c):                                   # c [P, D] -> [P, S], the sum over d in ascending order
        acc = np.zeros((P, S), F)
        for d in range(D):
            t = x[:, :, d] - c[:, None, d]
            acc = acc + t * t
        return acc

    def assign(c):
        dist = np.stack([d2(c[:, j]) for j in range(K)], axis=2)
        return dist.argmin(axis=2), dist          # argmin / argmax: the first of equals

    m = np.zeros((P, D), F)
    for s in range(S):
        m = m + x[:, s]
    m = m / F(S)
    c = np.zeros((P, K, D), F)
    c[:, 0] = x[rows, d2(m).argmax(axis=1)]
    mind = d2(c[:, 0])
    for j in range(1, K):
        c[:, j] = x[rows, mind.argmax(axis=1)]
        mind = np.minimum(mind, d2(c[:, j]))
    a, dist = assign(c)
    iters = np.zeros(P, np.int64)
    active = np.ones(P, bool)
    while active.any():
        new = c.copy()
        for j in range(K):
            on = a == j
            n = on.sum(axis=1)
            tot = np.zeros((P, D), F)
            for s in range(S):
                tot = tot + np.where(on[:, s, None], x[:, s] - c[:, j], F(0))
            upd = c[:, j] + tot / np.maximum(n, 1).astype(F)[:, None]
            new[:, j] = np.where((n > 0)[:, None], upd, c[:, j])
        c = np.where(active[:, None, None], new, c).astype(F)
        iters += active
        a_new, dist_new = assign(c)
        changed = (a_new != a).any(axis=1)
        a = np.where(active[:, None], a_new, a)
        dist = np.where(active[:, None, None], dist_new, dist)
        active = active & changed & (iters < max_iter)
    counts = np.stack([(a == j).sum(axis=1) for j in range(K)], axis=1)
    inertia = np.take_along_axis(dist, a[:, :, None], axis=2)[:, :, 0].astype(np.float64).sum(axis=1)
    return c, counts, inertia, iters, a


def margins(x, centers):
    """Second-best minus best squared distance of every sample to `centers`, in float64, and the
    float64 assignment: ([P, S], [P, S]); the margin is inf with one centre."""
    x, c = np.asarray(x, np.float64), np.asarray(centers, np.float64)
    dist = ((x[:, :, None, :] - c[:, None, :, :]) ** 2).sum(axis=3)
    part = np.sort(dist, axis=2)
    gap = part[:, :, 1] - part[:, :, 0] if c.shape[1] > 1 else np.full(dist.shape[:2], np.inf)
    return gap, dist.argmin(axis=2)


def times_ref(seed, P, S):
    """The generator of include/lsr_centers.h: [P, S] float32 in [0, 1), multiples of 2^-24."""
    u = np.uint32
    g = np.arange(P, dtype=np.uint32)[:, None]
    s = np.arange(S, dtype=np.uint32)[None, :]
    h = u(seed & 0xFFFFFFFF) ^ (g * u(0x9E3779B1)) ^ (s * u(0x85EBCA77))
    h = h ^ (h >> u(16))
    h = h * u(0x7FEB352D)
    h = h ^ (h >> u(15))
    h = h * u(0x846CA68B)
    h = h ^ (h >> u(16))
    return (h >> u(8)).astype(F) * F(2.0 ** -24)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def planted_sizes(S, K):
    """Unequal cluster sizes with one cluster of a single sample (K >= 2)."""
    if K == 1:
        return [S]
    w = np.arange(1, K)
    parts = [max(1, int((S - 1) * wi // w.sum())) for wi in w[:-1]]
    parts.append(S - 1 - sum(parts))
    assert parts[-1] >= 1
    return [1] + parts


@functools.lru_cache(maxsize=None)
def separated_case(P, S, D, K, seed=0):
    """x [P, S, D] float32 on the unit sphere: K planted directions at least 0.5 apart per row, every
    sample within 0.01 of its direction (a within-cluster spread of at most 0.02), shuffled; and the
    planted sizes."""
    rng = np.random.default_rng(1000 * seed + 7 * S + 31 * D + K)
    sizes = planted_sizes(S, K)
    x = np.zeros((P, S, D))
    for p in range(P):
        while True:
            dirs = _unit(rng.standard_normal((K, D)))
            gap = np.linalg.norm(dirs[:, None] - dirs[None], axis=2) + 10 * np.eye(K)
            if gap.min() >= 0.55:
                break
        pts = []
        for j, n in enumerate(sizes):
            off = rng.standard_normal((n, D))
            off = off / np.linalg.norm(off, axis=1, keepdims=True) * rng.uniform(0, 0.008, (n, 1))
            pts.append(_unit(dirs[j] + off))
        x[p] = np.concatenate(pts)[rng.permutation(S)]
    x = x.astype(F)
    x.setflags(write=False)
    return x, sizes


@functools.lru_cache(maxsize=None)
def unseparated_case(P, S, D, seed=0):
    """Uniform on the unit sphere: nothing to recover, only invariants hold."""
    rng = np.random.default_rng(77 + 1000 * seed + D)
    x = _unit(rng.standard_normal((P, S, D))).astype(F)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def separated_ref(P, S, D, K):
    """The restatement's answer on a separated case, computed once."""
    return kmeans_ref(separated_case(P, S, D, K)[0], K)
