"""Seeded inputs of the segmentation tests (tests/test_segment.py, tests/test_segment_gpu.py), shared with
the fixture generator tests/golden/make_segment_golden.py so that the fixture holds only a checksum and
the reference's results.

The maps are blobby, as relevancy maps are: a sigmoid of bilinearly up-sampled low-resolution noise
(one field per phrase, shared by its levels and its annotation, plus one per map) and pixel noise.
Roughly a third of each map ends above the threshold and the annotations are blob-shaped, so the IoUs
spread over (0, 1); uniform noise gives IoU near 0.005 and tests nothing.  Every map is float32 (the
values the kernel reads); float64 references upcast these same values.
"""
import hashlib

import numpy as np

FIXTURE_SEED = 2917
FIXTURE_LKHW = (2, 3, 61, 83)
CELL = 12                      # pixels per cell of the low-resolution noise
QUANTUM = 4096.0               # quantised maps are multiples of 1 / 4096: 29 * 29 * 4096 < 2^24, every window sum is exact


def smooth_field(H, W, rng):
    """[H, W] float64, about unit variance: N(0, 1) on a grid of CELL-pixel cells, bilinearly up-sampled."""
    gh, gw = H // CELL + 2, W // CELL + 2
    g = rng.normal(0.0, 1.0, (gh, gw))
    y, x = np.arange(H) / CELL, np.arange(W) / CELL
    y0, x0 = y.astype(int), x.astype(int)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    top = g[y0][:, x0] * (1 - fx) + g[y0][:, x0 + 1] * fx
    bot = g[y0 + 1][:, x0] * (1 - fx) + g[y0 + 1][:, x0 + 1] * fx
    return (top * (1 - fy) + bot * fy) * 1.4


def maps(L, n_pos, H, W, seed, quantised=False):
    """(rel [L, n_pos, H, W] float32 in (0, 1), gt [n_pos, H, W] uint8 of 0 / 1)."""
    rng = np.random.default_rng(seed)
    rel = np.empty((L, n_pos, H, W), np.float64)
    gt = np.empty((n_pos, H, W), np.uint8)
    for k in range(n_pos):
        base = smooth_field(H, W, rng)
        gt[k] = base > 0.5
        for l in range(L):
            z = 0.8 * base + 0.5 * smooth_field(H, W, rng) + 0.25 * rng.normal(0.0, 1.0, (H, W))
            rel[l, k] = 1.0 / (1.0 + np.exp(-3.0 * (z + 0.1)))
    if quantised:
        rel = np.round(rel * QUANTUM) / QUANTUM
    return rel.astype(np.float32), gt


def checksum(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def fixture_inputs():
    """The fixture's inputs: (rel [2, 3, 61, 83] float32, gt [3, 61, 83] uint8)."""
    return maps(*FIXTURE_LKHW, FIXTURE_SEED)
