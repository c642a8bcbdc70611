"""Seeded inputs of the image-loss tests (tests/test_image_loss.py, tests/test_image_loss_gpu.py), shared
with the fixture generator tests/golden/make_image_loss_golden.py: the fixture holds the seeds, a checksum
of the regenerated inputs and the reference's results.

The shapes are the smallest at which the stencil of csrc/image_loss.hip can go wrong (its tile is
TILE_H x TILE_W pixels, the window 11 taps, the padding 5):
  a   1 view, 3 planes, 7 x 5: both sides shorter than the window, every window clipped on all four sides
  b   2 views, 37 x 19: ragged against the tile; the ground truth is the [:, :3] view of a [V, 4, H, W]
      tensor (views 4 H W floats apart)
  c   8 views, 83 x 61: several tiles both ways, the full view count
  d0, d1   one plane of 1 x 40 and of 40 x 1: one row, one column
  e0, e1, e2   3 views of exactly one tile, one tile + 1 both ways, (2 TILE_H - 1) x (2 TILE_W + 1): the seams

Content: gt uniform in [0, 1), x = clamp(gt + 0.15 noise, 0, 1).  In a patch in the middle x is constant
(windows inside it have variance 0: the denominators sit at C2); in a patch at the bottom right x == gt
(ssim_map 1, and L1's sign(0) = 0).  Outside that patch no element has |x - gt| < 1e-3 (elements that
would are moved 1e-2 away), so no sign depends on the precision it is taken in.
"""
import hashlib

import numpy as np

TILE_H, TILE_W = 16, 64          # IL_TH, IL_TW of csrc/image_loss.hip
FIXTURE_SEED = 9127
# name: (V, C, H, W, channels of the ground-truth tensor)
CASES = {
    "a": (1, 3, 7, 5, 3),
    "b": (2, 3, 37, 19, 4),
    "c": (8, 3, 83, 61, 3),
    "d0": (1, 1, 1, 40, 1),
    "d1": (1, 1, 40, 1, 1),
    "e0": (3, 3, TILE_H, TILE_W, 3),
    "e1": (3, 3, TILE_H + 1, TILE_W + 1, 3),
    "e2": (3, 3, 2 * TILE_H - 1, 2 * TILE_W + 1, 3),
}
# the one array too large for the 1 MiB file limit beside the others lives in a file of its own
GRAD_FILE_OF = {"c": "image_loss_golden_c.npz"}


def patches(H, W):
    """((rows, cols) of the constant patch, (rows, cols) of the x == gt patch): disjoint slices."""
    th, tw = -(-H // 3), -(-W // 3)
    qh, qw = -(-H // 4), -(-W // 4)
    return (slice(H // 3, H // 3 + th), slice(W // 3, W // 3 + tw)), (slice(H - qh, H), slice(W - qw, W))


def equal_mask(H, W):
    m = np.zeros((H, W), bool)
    _, (r, c) = patches(H, W)
    m[r, c] = True
    return m


def inputs(name):
    """(x [V, C, H, W] float32, gt_full [V, Cg, H, W] float32); the ground truth of the loss is gt_full[:, :C]."""
    V, C, H, W, Cg = CASES[name]
    rng = np.random.default_rng(FIXTURE_SEED + 101 * sorted(CASES).index(name))
    gt_full = rng.random((V, Cg, H, W), dtype=np.float32)
    noise = rng.standard_normal((V, C, H, W), dtype=np.float32)
    gt = gt_full[:, :C]                                              # a view: edits below land in gt_full
    x = np.clip(gt + np.float32(0.15) * noise, 0.0, 1.0).astype(np.float32)
    (cr, cc), (er, ec) = patches(H, W)
    x[:, :, cr, cc] = np.float32(0.5)
    const = np.zeros((H, W), bool)
    const[cr, cc] = True
    close = np.abs(x - gt) < 2e-3
    # in the constant patch the ground truth moves, elsewhere x does
    move_gt = close & const
    gt[move_gt] = np.where(gt[move_gt] < 0.5, gt[move_gt] - np.float32(1e-2), gt[move_gt] + np.float32(1e-2))
    move_x = close & ~const
    x[move_x] = np.where(gt[move_x] < 0.5, gt[move_x] + np.float32(1e-2), gt[move_x] - np.float32(1e-2))
    x[:, :, er, ec] = gt[:, :, er, ec]
    outside = ~np.broadcast_to(equal_mask(H, W), x.shape)
    assert not (np.abs(x.astype(np.float64) - gt.astype(np.float64))[outside] < 1e-3).any(), name
    assert x.min() >= 0.0 and x.max() <= 1.0 and gt_full.min() >= -1e-2 and gt_full.max() <= 1.0 + 1e-2
    return x, gt_full


def checksum(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
