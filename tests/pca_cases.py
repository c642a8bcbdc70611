"""The yardstick of the PCA colouring tests: a float64 numpy restatement of the five formulas of
include/lsr_pca.h (gaussian_scene.pca_compress, i.e. sklearn's PCA(3).fit_transform and one min-max),
and the planted-spectrum images the tests run on.

An image is a random orthogonal basis with per-axis standard deviations spread * (1, 0.6, 0.36, then
0.16 decaying by 0.8 per axis) around a per-channel mean near 0.5, rounded to float32; the reference
upcasts those same float32 values.  The builder asserts, per case, the conditions under which the
answer is well defined: each of the top three eigenvalues is at least twice the next (else the
components are ill-conditioned), and in each component the entry of largest magnitude leads the
second by 0.01 (else the sign rule is).  These are conditions on inputs, not tolerances: the seeds
below were chosen so that every case meets them.
"""
import functools

import numpy as np

# The kernel constants the large cases are sized from, as include/lsr_pca.h defines them (tests/test_pca.py
# compares them with the header and with _lib): pixels of one block partial (LSR_PCA_BLOCK_PIXELS) and of
# one staged tile (LSR_PCA_TILE_PIXELS), and the fan-in of the two cross-block reductions: k_pca_finish's
# wave w adds the partials of blocks w, w + FINISH_WAVES, ... before the waves' sums are added
# (LSR_PCA_FINISH_WAVES), and k_pca_range's thread t folds the min / max pairs of blocks t,
# t + RANGE_THREADS, ... (LSR_PCA_RANGE_THREADS).
BLOCK_PIXELS = 2048
TILE_PIXELS = 256
FINISH_WAVES = 16
RANGE_THREADS = 256

EIGEN_GAP = 2.0
SIGN_MARGIN = 0.01


def pca_reference(x):
    """x [N, C] -> dict(mean [C], components [3, C], explained_variance [3], y [N, 3], out [N, 3],
    lo, hi, eigenvalues [C] descending), all float64."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mean = x.sum(axis=0) / n
    xc = x - mean
    cov = xc.T @ xc / (n - 1)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(w)[::-1]
    w, v = w[order], v[:, order]
    comps = v[:, :3].T.copy()
    for k in range(3):
        if comps[k, np.argmax(np.abs(comps[k]))] < 0:
            comps[k] = -comps[k]
    y = xc @ comps.T
    lo, hi = y.min(), y.max()
    out = (y - lo) / (hi - lo) if hi > lo else np.zeros_like(y)
    return dict(mean=mean, components=comps, explained_variance=w[:3].copy(), y=y, out=out, lo=lo, hi=hi,
                eigenvalues=w)


def well_defined(ref):
    """(smallest ratio of a top-three eigenvalue to the next, smallest lead of a component's largest entry)."""
    w = ref["eigenvalues"]
    gap = min(w[k] / max(w[k + 1], 1e-300) for k in range(3))
    lead = min(np.diff(np.sort(np.abs(c))[-2:])[0] for c in ref["components"])
    return gap, lead


def planted_image(H, W, C, seed, spread=0.15):
    """[H, W, C] float32 with the planted spectrum."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(C, C)))
    std = spread * np.array([1.0, 0.6, 0.36] + [0.16 * 0.8 ** i for i in range(C - 3)])
    mean = 0.5 + 0.05 * rng.uniform(-1, 1, size=C)
    z = rng.normal(size=(H * W, C))
    return (mean + (z * std) @ q.T).astype(np.float32).reshape(H, W, C)


# name: (H, W, C, seed, spread)
CASES = {
    "5x7x4": (5, 7, 4, 3, 0.15),             # fewer pixels than a wave, the smallest C
    "16x24x6": (16, 24, 6, 1, 0.15),         # the video width
    "17x23x32": (17, 23, 32, 5, 0.15),       # ragged slabs of 4 and a ragged last wave
    "33x65x16": (33, 65, 16, 11, 0.15),      # C padded to the tile (seed 1 leaves a sign margin of 0.002)
    "40x48x32": (40, 48, 32, 5, 0.15),
    # 61 * 83 = 5063 = 2 * BLOCK_PIXELS + 3 * TILE_PIXELS + 199: two full blocks and a ragged third whose last
    # tile is ragged, so the cross-block sums in float64 add three partials; C = 20 half-fills the second tile
    "blocks": (61, 83, 20, 7, 0.15),
    "low-contrast": (40, 48, 32, 8, 0.02),   # spread 0.02 around 0.5: what an uncentred float32 Gram loses
    # 260 * 262 = 68120 = 33 * BLOCK_PIXELS + 2 * TILE_PIXELS + 24: 34 > 2 * FINISH_WAVES blocks with a ragged
    # last one, so every wave of k_pca_finish adds at least two partials (waves 0 and 1 three) before the
    # 16-way fold.  H * W is a multiple of 4 and so is C: whole tiles take the 16-byte loads in both layouts.
    "fan-in": (260, 262, 20, 2, 0.15),
    # 724 * 726 = 525624 = 256 * BLOCK_PIXELS + 5 * TILE_PIXELS + 56: 257 > RANGE_THREADS blocks, so thread 0 of
    # k_pca_range folds two pairs, and a wave of k_pca_finish adds 16 or 17 partials: its loop, unrolled by 8,
    # runs the unrolled body twice and the remainder.  The smallest C keeps it at 8 MB.
    "many-blocks": (724, 726, 4, 3, 0.15),
}
assert 61 * 83 == 2 * BLOCK_PIXELS + 3 * TILE_PIXELS + 199
assert 260 * 262 == 33 * BLOCK_PIXELS + 2 * TILE_PIXELS + 24 and 33 > 2 * FINISH_WAVES and 260 * 262 % 4 == 0
assert 724 * 726 == RANGE_THREADS * BLOCK_PIXELS + 5 * TILE_PIXELS + 56 and 724 * 726 % 4 == 0
assert RANGE_THREADS >= 2 * 8 * FINISH_WAVES             # 257 blocks: two turns of the loop unrolled by 8


@functools.lru_cache(maxsize=None)
def case(name):
    """(image [H, W, C] float32, reference dict over its pixels), built once and shared: do not modify."""
    H, W, C, seed, spread = CASES[name]
    img = planted_image(H, W, C, seed, spread)
    ref = pca_reference(img.reshape(-1, C))
    gap, lead = well_defined(ref)
    assert gap >= EIGEN_GAP, f"case {name}: eigenvalue ratio {gap:.3f} < {EIGEN_GAP}: pick another seed"
    assert lead >= SIGN_MARGIN, f"case {name}: sign margin {lead:.4f} < {SIGN_MARGIN}: pick another seed"
    img.setflags(write=False)
    return img, ref


SEQUENCE_SEED = 5


@functools.lru_cache(maxsize=None)
def sequence_case():
    """Three 17x23x32 frames cut from one planted spectrum, and the reference over their concatenated
    pixels."""
    big = planted_image(3 * 17, 23, 32, SEQUENCE_SEED, 0.15)
    frames = [np.ascontiguousarray(big[17 * i:17 * (i + 1)]) for i in range(3)]
    ref = pca_reference(np.concatenate([f.reshape(-1, 32) for f in frames]))
    gap, lead = well_defined(ref)
    assert gap >= EIGEN_GAP and lead >= SIGN_MARGIN, (gap, lead)
    for f in frames:
        f.setflags(write=False)
    return frames, ref
