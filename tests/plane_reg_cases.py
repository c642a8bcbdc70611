"""The HexPlane regularisers restated in float64 numpy (include/lsr_plane_reg.h; scene/regulation.py:22-28,
scene/gaussian_model.py:763-802), and the cases tests/test_plane_reg.py and tests/test_plane_reg_gpu.py share.

  d2[c, i, w] = t[c, i+2, w] - 2 t[c, i+1, w] + t[c, i, w]          i in [0, H - 2)
  smooth      = sum d2^2 / N_s,  N_s = C (H - 2) W
  d smooth / d t[c, j, w] = (2 / N_s) (d2[j-2] - 2 d2[j-1] + d2[j]),  d2 = 0 outside [0, H - 2)
  l1          = sum |1 - t| / N,  N = C H W;   d l1 / d t = -sign(1 - t) / N,  sign(0) = 0
"""
import numpy as np

SPATIAL, TIME = (0, 1, 3), (2, 4, 5)
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]   # xy, xz, xt, yz, yt, zt
GOLDEN_RES, GOLDEN_MULTIRES, GOLDEN_WEIGHTS = [4, 5, 6, 7], [1, 2], (1e-3, 1e-4, 2e-4)

# (C, H, W): the smallest shapes at which the stencil can go wrong.  H = 3: one second difference per column;
# H = 4: two, no element sees three; H = 5: the first H with an element whose three d2 all exist; W = 65 and 257:
# rows that are no multiple of a wave or of a block's 256 threads; (16, 6, 64) = 6 whole blocks of 1024 elements;
# (16, 5, 65) and (3, 9, 257): several blocks that start mid-row and mid-channel, the last one in part
SHAPES = [(1, 3, 1), (1, 4, 1), (2, 5, 7), (16, 5, 65), (16, 6, 64), (3, 9, 257)]
# name -> (w_smooth, w_l1)
MODES = {"smooth": (3e-3, 0.0), "l1": (0.0, 7e-4), "both": (1e-3, 1e-4)}
KINDS = ("spatial", "time")


def plane_shapes(resolution, multires, channels=16):
    """[scale][ci] -> (1, C, H, W) of a field's planes (scene/hexplane.py:48-70)."""
    out = []
    for m in multires:
        reso = [r * m for r in resolution[:3]] + [resolution[3]]
        out.append([(1, channels, reso[c1], reso[c0]) for c0, c1 in PAIRS])
    return out


def plane_values(shape, kind, rng):
    """float32 [1, C, H, W]: 'spatial' U(0.1, 0.5) (a fresh spatial plane); 'time' 1 with half the entries
    perturbed by N(0, 1e-2) (a time plane early in training: the rest sit exactly on the L1 term's kink)."""
    shape = (1,) + tuple(shape)[-3:]
    if kind == "spatial":
        return rng.uniform(0.1, 0.5, size=shape).astype(np.float32)
    t = np.ones(shape, np.float32)
    hit = rng.random(size=shape) < 0.5
    t[hit] += (rng.normal(size=shape) * 1e-2).astype(np.float32)[hit]
    return t


def smooth_np(t):
    """(smooth, d smooth / d t) in float64; (0, zeros) where H < 3."""
    t = np.asarray(t, np.float64)
    _, C, H, W = t.shape
    g = np.zeros_like(t)
    if H < 3:
        return 0.0, g
    n_s = C * (H - 2) * W
    d2 = t[:, :, 2:] - 2 * t[:, :, 1:-1] + t[:, :, :-2]
    g[:, :, 2:] += d2                       # d2[j - 2]
    g[:, :, 1:-1] -= 2 * d2                 # d2[j - 1]
    g[:, :, :-2] += d2                      # d2[j]
    return float((d2 * d2).sum() / n_s), g * (2.0 / n_s)


def l1_np(t):
    """(l1, d l1 / d t) in float64."""
    t = np.asarray(t, np.float64)
    return float(np.abs(1 - t).sum() / t.size), -np.sign(1 - t) / t.size


def plane_np(t, w_smooth, w_l1):
    """(smooth, l1, w_smooth d smooth + w_l1 d l1) of one plane."""
    s, gs = smooth_np(t)
    a, ga = l1_np(t)
    return s, a, w_smooth * gs + w_l1 * ga


def plane_weights(weights, ci):
    tsw, l1w, tvw = weights
    return (tvw, 0.0) if ci in SPATIAL else (tsw, l1w)


def field_np(planes, weights):
    """planes [scale][ci] -> (total, terms [n, 2], grads [scale][ci]) with weights = (time_smoothness_weight,
    l1_time_planes_weight, plane_tv_weight)."""
    tsw, l1w, tvw = weights
    terms, grads, sums = [], [], [0.0, 0.0, 0.0]
    for scale in planes:
        grads.append([])
        for ci, t in enumerate(scale):
            s, a, g = plane_np(t, *plane_weights(weights, ci))
            terms.append((s, a))
            grads[-1].append(g)
            if ci in SPATIAL:
                sums[0] += s
            else:
                sums[1] += s
                sums[2] += a
    return tvw * sums[0] + tsw * sums[1] + l1w * sums[2], np.array(terms, np.float64).reshape(-1, 2), grads
