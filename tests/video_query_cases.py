"""Seeded inputs of the time-sensitive query tests (tests/test_video_query.py, tests/test_video_query_gpu.py),
shared with the fixture generator tests/golden/make_video_query_golden.py so that the fixture holds only
seeds, checksums and the reference's results.

As in tests/query_cases.py: weights N(0, 2 / in), biases N(0, 0.1^2), latents uniform (-1, 1), queries a
decoded pixel plus noise so that the cosines spread over a useful range.  Every array is float32 (the
values the kernel reads); float64 references upcast these same values.
"""
import numpy as np

from query_cases import checksum, decode_np, decoder_arrays, latents, state_dict  # noqa: F401

FIXTURE_SEED = 6203
FULL_DIMS = [6, 32, 64, 128, 256, 512, 1024, 2048, 4096]    # the reference's video decoder (eval/eval.py:428-429)
FIXTURE_HW = (24, 20)
FIXTURE_MASKS = 3
COEFFS = ([0.1, 0.8, 0.1], [0.1, 0.2, 0.4, 0.2, 0.1])       # the reference's two default windows


def queries(ws, bs, pixels, n, seed, scale=1.7):
    """n query vectors [n, d_out] float32: the decoded feature of a seeded row of `pixels` [N, c_in] plus
    0.6 N(0, 1 / d_out) noise, times `scale` (they are not unit vectors: the code under test normalises)."""
    rng = np.random.default_rng(seed)
    f = decode_np(ws, bs, pixels[rng.integers(0, pixels.shape[0], n)])
    e = f + 0.6 * rng.normal(0.0, np.sqrt(1.0 / f.shape[1]), f.shape)
    return (scale * e).astype(np.float32)


def case(dims, n_rows, n_q, seed):
    """One sweep case: (ws, bs, rows [n_rows, c_in], queries [n_q, d_out])."""
    ws, bs = decoder_arrays(dims, seed)
    rows = latents((n_rows, dims[0]), seed + 1)
    return ws, bs, rows, queries(ws, bs, rows, n_q, seed + 2)


def fixture_masks(seed=FIXTURE_SEED + 3):
    """[3, H, W] uint8: mask 0 a 7 x 8 rectangle (56 pixels), mask 1 a seeded scatter of about 100, mask 2
    labels 0 / 1 / 2 mixed: a 12 x 10 rectangle of ones (120) whose seeded third is relabelled 2, with 2s
    outside it as well.  Only == 1 counts."""
    H, W = FIXTURE_HW
    rng = np.random.default_rng(seed)
    m = np.zeros((FIXTURE_MASKS, H, W), np.uint8)
    m[0, 3:10, 5:13] = 1
    m[1] = rng.random((H, W)) < 0.21
    m[2, 8:20, 6:16] = 1
    m[2][(rng.random((H, W)) < 0.33) & (m[2] == 1)] = 2
    m[2, 0:3, 0:5] = 2
    return m


def fixture_inputs():
    """dict(ws, bs, latent [H, W, 6], masks [3, H, W] uint8, queries [3, 4096])."""
    H, W = FIXTURE_HW
    ws, bs = decoder_arrays(FULL_DIMS, FIXTURE_SEED)
    lat = latents((H, W, FULL_DIMS[0]), FIXTURE_SEED + 1)
    q = queries(ws, bs, lat.reshape(-1, FULL_DIMS[0]), FIXTURE_MASKS, FIXTURE_SEED + 2)
    return dict(ws=ws, bs=bs, latent=lat, masks=fixture_masks(), queries=q)


# ---- the host-side part: frame lists for evaluate_video_feature and the smoothing ---------------------------
def eval_cases():
    """{name: dict(ids, sims, ious, intervals, thresh)}: inputs of evaluate_video_feature."""
    rng = np.random.default_rng(FIXTURE_SEED + 10)
    n = 14
    sims = rng.uniform(0.2, 0.8, n).round(6).tolist()
    ious = rng.uniform(0.3, 0.95, n).round(6).tolist()
    ids = list(range(3, 3 + n))
    return {
        "generic": dict(ids=ids, sims=sims, ious=ious, intervals=[[4, 8], [12, 13]], thresh=float(np.mean(sims))),
        "nothing_predicted_nothing_labelled": dict(ids=ids, sims=sims, ious=ious, intervals=[[40, 50]], thresh=0.9),
        "no_predictions": dict(ids=ids, sims=sims, ious=ious, intervals=[[5, 9]], thresh=0.9),
        "all_predicted_none_labelled": dict(ids=ids, sims=sims, ious=ious, intervals=[], thresh=0.1),
        # frames 5 and 9 lie exactly on the interval's ends, 4 and 10 just outside; every frame is predicted
        "interval_ends": dict(ids=[4, 5, 7, 9, 10], sims=[0.5, 0.5, 0.5, 0.5, 0.5], ious=[0.9, 0.8, 0.7, 0.6, 0.5],
                              intervals=[[5, 9]], thresh=0.5),
    }


def smooth_cases():
    """{name: dict(values, coeffs)}: inputs of the smoothing loop."""
    rng = np.random.default_rng(FIXTURE_SEED + 11)
    v = rng.uniform(0.0, 1.0, 9).round(6).tolist()
    return {
        "nine_by_three": dict(values=v, coeffs=COEFFS[0]),
        "nine_by_five": dict(values=v, coeffs=COEFFS[1]),
        "two_by_three": dict(values=v[:2], coeffs=COEFFS[0]),       # shorter than the window: all raw
        "four_by_five": dict(values=v[:4], coeffs=COEFFS[1]),       # shorter than the window: all raw
        "five_by_five": dict(values=v[:5], coeffs=COEFFS[1]),       # only the middle frame is smoothed
        "one_by_three": dict(values=v[:1], coeffs=COEFFS[0]),
    }


def sequence_case():
    """One phrase over 11 frames given out of order: dict(ids, sims, clip, ious, intervals).  A spike in the
    video similarities and a ramp in the CLIP scores make the unsmoothed / smoothed mean rule matter."""
    rng = np.random.default_rng(FIXTURE_SEED + 12)
    n = 11
    ids = rng.permutation(np.arange(20, 20 + n)).tolist()
    sims = rng.uniform(0.30, 0.40, n)
    sims[[2, 5]] = [0.95, 0.05]
    clip = rng.uniform(0.2, 0.6, n)
    clip[[0, 7]] = [0.99, 0.01]
    ious = rng.uniform(0.4, 0.9, n)
    return dict(ids=ids, sims=sims.round(6).tolist(), clip=clip.round(6).tolist(), ious=ious.round(6).tolist(),
                intervals=[[22, 25], [28, 28]])
