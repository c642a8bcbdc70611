"""Seeded inputs of the open-vocabulary query tests (tests/test_query.py, tests/test_query_gpu.py),
shared with the fixture generator tests/golden/make_query_golden.py so that the fixture holds only
seeds, a checksum and the reference's results.

Weights are N(0, 2 / in) and biases N(0, 0.1^2): with nn.Linear's default init every pixel decodes
to nearly the same vector and the relevancy stays within 0.43-0.52, which tests little.  Every array
is float32 (the values the kernel reads); float64 references upcast these same values.
"""
import hashlib

import numpy as np

FIXTURE_SEED = 4117
FIXTURE_DIMS = [3, 16, 32, 64, 128, 256, 512]       # c_in, then the decoder's widths
FIXTURE_LHW = (3, 37, 29)
FIXTURE_POS, FIXTURE_NEG = 5, 4
FIXTURE_SAMPLES = 64                                 # pixels whose decoded features the fixture holds
DEFAULT_DECODER = FIXTURE_DIMS[1:]


def decoder_arrays(dims, seed):
    """([W_i [out, in]], [b_i [out]]) float32 of a decoder with dims = [c_in, widths...]."""
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    for i in range(len(dims) - 1):
        ws.append(rng.normal(0.0, np.sqrt(2.0 / dims[i]), (dims[i + 1], dims[i])).astype(np.float32))
        bs.append(rng.normal(0.0, 0.1, dims[i + 1]).astype(np.float32))
    return ws, bs


def latents(shape, seed):
    """Uniform (-1, 1) float32."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


def decode_np(ws, bs, x):
    """The decoder in float64 numpy (used only to place the phrase embeddings near real features)."""
    x = np.asarray(x, np.float64)
    for i, (w, b) in enumerate(zip(ws, bs)):
        x = (np.maximum(x, 0.0) if i else x) @ w.astype(np.float64).T + b.astype(np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def phrase_embeddings(ws, bs, pixels, n, seed):
    """n unit vectors [n, d_out] float32: the decoded feature of a seeded pixel of `pixels` [N, c_in]
    plus 0.3 N(0, 1 / d_out) noise, renormalised."""
    rng = np.random.default_rng(seed)
    f = decode_np(ws, bs, pixels[rng.integers(0, pixels.shape[0], n)])
    e = f + 0.3 * rng.normal(0.0, np.sqrt(1.0 / f.shape[1]), f.shape)
    return (e / np.linalg.norm(e, axis=-1, keepdims=True)).astype(np.float32)


def state_dict(ws, bs, torch):
    """The decoder's part of the reference Autoencoder's state dict: Linear layers at 0, 2, 4, ..."""
    sd = {}
    for i, (w, b) in enumerate(zip(ws, bs)):
        sd[f"decoder.{2 * i}.weight"] = torch.from_numpy(w.copy())
        sd[f"decoder.{2 * i}.bias"] = torch.from_numpy(b.copy())
    return sd


def checksum(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def case(dims, n_pix, n_pos, n_neg, seed):
    """One sweep case: (ws, bs, latent [n_pix, c_in], pos [n_pos, d_out], neg [n_neg, d_out])."""
    ws, bs = decoder_arrays(dims, seed)
    lat = latents((n_pix, dims[0]), seed + 1)
    e = phrase_embeddings(ws, bs, lat, n_pos + n_neg, seed + 2)
    return ws, bs, lat, e[:n_pos], e[n_pos:]


def fixture_inputs():
    """The fixture's inputs: dict(ws, bs, latent [L, H, W, 3], pos, neg, samples [64] flat pixel indices)."""
    L, H, W = FIXTURE_LHW
    ws, bs = decoder_arrays(FIXTURE_DIMS, FIXTURE_SEED)
    lat = latents((L, H, W, FIXTURE_DIMS[0]), FIXTURE_SEED + 1)
    e = phrase_embeddings(ws, bs, lat.reshape(-1, FIXTURE_DIMS[0]), FIXTURE_POS + FIXTURE_NEG, FIXTURE_SEED + 2)
    samples = np.random.default_rng(FIXTURE_SEED + 3).choice(L * H * W, FIXTURE_SAMPLES, replace=False)
    return dict(ws=ws, bs=bs, latent=lat, pos=e[:FIXTURE_POS], neg=e[FIXTURE_POS:], samples=np.sort(samples))
