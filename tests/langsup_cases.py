"""Seeded inputs of the language-supervision tests (tests/test_language_supervision.py,
tests/test_language_supervision_gpu.py), shared with the fixture generator
tests/golden/make_langsup_golden.py so that the fixture holds the files' contents, a checksum of
the regenerated images and the reference's results.

A segment map is blocky (neighbouring pixels share a segment, as real maps do) with seeded -1
pixels; where the image is tall enough row 1 is wholly unlabelled (H >= 2) and row 2 is one segment
(H >= 3), and
pixel (0, 0) carries the index S - 1.  Images and tables are N(0, 1) float32 (the values the kernel
reads); float64 references upcast these same values.
"""
import hashlib

import numpy as np

LAM, BETA = 0.2, 0.01        # train.py's --lam and --beta defaults
FIXTURE_SEED = 5231
# (V, C, H, W, S, the feature level the losses use)
FIXTURE_CASES = [(2, 32, 19, 37, 11, 1), (1, 3, 5, 300, 4, 3)]
# the reference's naming, per view of each case: (colmap_id, data_type, split, cam_name)
FIXTURE_VIEWS = [[(17, "nerfies", "train", None), (612, "dynerf", "train", "cam03")],
                 [(4, "nerfies", "test", None)]]
# every naming the stems test covers (the dynerf video split has no supervision)
STEM_QUERIES = [(17, "nerfies", "train", None), (17, "nerfies", "test", None), (17, "nerfies", "video", None),
                (0, "nerfies", "train", None), (612, "dynerf", "train", "cam03"), (299, "dynerf", "test", "cam00"),
                (612, "dynerf", "video", "cam03")]
OUT_OF_RANGE = (-7, -2 ** 31, 2 ** 31 - 1)      # with S and S + 5: the values an "oob" map adds


def seg_map(H, W, S, seed, unlabelled=0.08, oob=False, all_unlabelled=False):
    """[H, W] int32."""
    rng = np.random.default_rng(seed)
    if all_unlabelled:
        return np.full((H, W), -1, np.int32)
    bh, bw = int(rng.integers(2, 5)), int(rng.integers(5, 12))
    perm = rng.integers(0, S, 4096)
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    seg = perm[((hh // bh) * 61 + ww // bw) % 4096].astype(np.int64)
    seg[rng.random((H, W)) < unlabelled] = -1
    if oob:
        bad = rng.random((H, W)) < 0.08
        seg[bad] = rng.choice(np.array([S, S + 5, *OUT_OF_RANGE], np.int64), int(bad.sum()))
    if H >= 2:
        seg[1] = -1
    if H >= 3:
        seg[2] = int(rng.integers(0, S))
    seg[0, 0] = S - 1
    if W > 1 and H < 3:
        seg[0, W - 1] = -1
    return seg.astype(np.int32)


def table(S, C, seed):
    return np.random.default_rng(seed).normal(0.0, 1.0, (S, C)).astype(np.float32)


def image(C, H, W, seed, seg, tab):
    """N(0, 1) float32 [C, H, W]; labelled elements within 1e-3 of their target move by 1e-2 (and row 2,
    where there is one, copies its target in channel 0 shifted by 0.5, a constant row against a
    constant target), so that no sign(x - t) depends on the precision it is taken in."""
    x = np.random.default_rng(seed).normal(0.0, 1.0, (C, H, W)).astype(np.float32)
    S = tab.shape[0]
    m = (seg >= 0) & (seg < S)
    t = tab[np.where(m, seg, 0)].transpose(2, 0, 1)
    if H >= 3:
        x[0, 2] = t[0, 2] + np.float32(0.5)
    close = m[None] & (np.abs(x - t) < 1e-3)
    x[close] += np.float32(1e-2)
    return x


def checksum(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def fixture_inputs(k):
    """Case k of the fixture: dict(segs [V, 4, H, W] int32, tables [V, S, C], images [V, C, H, W], level)."""
    V, C, H, W, S, level = FIXTURE_CASES[k]
    base = FIXTURE_SEED + 1000 * k
    segs = np.stack([np.stack([seg_map(H, W, S, base + 10 * v + lv) for lv in range(4)]) for v in range(V)])
    tables = np.stack([table(S, C, base + 100 + v) for v in range(V)])
    images = np.stack([image(C, H, W, base + 200 + v, segs[v, level], tables[v]) for v in range(V)])
    return dict(segs=segs, tables=tables, images=images, level=level)


# the GPU sweep: (V, C, H, W, S), the smallest shapes that reach each code path
SWEEP = [(1, 3, 1, 1, 1), (1, 6, 5, 63, 2), (8, 3, 2, 65, 7), (1, 7, 3, 37, 5), (2, 32, 3, 300, 40),
         (1, 32, 2, 1352, 700)]


def sweep_case(V, C, H, W, S, seed=77, oob=True, all_unlabelled=False):
    """(segs [V, H, W], tables [V, S, C], images [V, C, H, W]) with unlabelled pixels, where H >= 2 an
    all-unlabelled row, and (oob) indices outside [-1, S)."""
    base = seed + 7919 * (V + 3 * C + 5 * H + 11 * W + 13 * S)
    segs = np.stack([seg_map(H, W, S, base + v, oob=oob, all_unlabelled=all_unlabelled) for v in range(V)])
    tables = np.stack([table(S, C, base + 100 + v) for v in range(V)])
    images = np.stack([image(C, H, W, base + 200 + v, segs[v], tables[v]) for v in range(V)])
    return segs, tables, images
