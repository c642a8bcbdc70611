"""Seeded inputs of the language autoencoder tests (tests/test_autoencoder.py, tests/test_autoencoder_gpu.py),
shared with the fixture generator tests/golden/make_autoencoder_golden.py so that the fixture holds only
seeds, checksums and the reference's results.

State dicts carry the reference Autoencoder's keys (autoencoder/model.py).  Linear weights and biases are
uniform in +-1 / sqrt(fan_in) (nn.Linear's default distribution); the BatchNorm weights are uniform in
(0.5, 1.5) and their biases in (-0.3, 0.3), so that neither drops out of a product.  Rows are random unit
vectors, as CLIP and E5 features are.  Every floating array is float32 (the values the kernels read); float64
references upcast these same values.

The biases of the Linear layers in front of a BatchNorm have a true gradient of zero (train-mode BatchNorm
subtracts them): in float32 their gradient is rounding noise, Adam divides noise by itself, and they walk by
up to about lr per step.  PRE_BN_RULE is how the tests treat them.
"""
import hashlib

import numpy as np

FIXTURE_SEED = 15061
FEATURE, ENC, DEC = 48, [32, 16, 3], [16, 32, 48]
BATCH, LR, COS_WEIGHT, STEPS = 37, 7e-4, 1e-3, 8
EVAL_ROWS = 200
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
TOL = 8.0                                   # tests/test_query_gpu.py:3-8
PRE_BN_RULE = "finite, and |change| <= lr max(1, (1 - beta1) / sqrt(1 - beta2)) per step"

CLIP = (512, [256, 128, 64, 32, 3], [16, 32, 64, 128, 256, 256, 512])
VIDEO = (4096, [2048, 1024, 512, 256, 128, 64, 32, 6], [32, 64, 128, 256, 512, 1024, 2048, 4096])
ODD = (80, [144, 16, 6], [32, 144, 80])


def checksum(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def enc_key(i):
    return f"encoder.{3 * i}"


def bn_key(i):
    return f"encoder.{3 * i - 2}"


def dec_key(j):
    return f"decoder.{2 * j}"


def state_dict_np(feature, enc, dec, seed, running=False):
    """{key: array} in the reference's key order.  running: non-trivial running statistics (mean
    N(0, 0.2^2), variance uniform (0.5, 1.5), 5 batches tracked) instead of 0 / 1 / 0."""
    rng = np.random.default_rng(seed)
    sd = {}

    def linear(key, fan_in, fan_out):
        b = 1.0 / np.sqrt(fan_in)
        sd[key + ".weight"] = rng.uniform(-b, b, (fan_out, fan_in)).astype(np.float32)
        sd[key + ".bias"] = rng.uniform(-b, b, fan_out).astype(np.float32)

    prev = feature
    for i, d in enumerate(enc):
        if i:
            k = bn_key(i)
            sd[k + ".weight"] = rng.uniform(0.5, 1.5, prev).astype(np.float32)
            sd[k + ".bias"] = rng.uniform(-0.3, 0.3, prev).astype(np.float32)
            sd[k + ".running_mean"] = (rng.normal(0, 0.2, prev) if running else np.zeros(prev)).astype(np.float32)
            sd[k + ".running_var"] = (rng.uniform(0.5, 1.5, prev) if running else np.ones(prev)).astype(np.float32)
            sd[k + ".num_batches_tracked"] = np.array(5 if running else 0, np.int64)
        linear(enc_key(i), prev, d)
        prev = d
    for j, d in enumerate(dec):
        linear(dec_key(j), prev, d)
        prev = d
    return sd


def torch_state_dict(sd, torch, dtype=None):
    """The arrays as tensors; floating ones cast to dtype if given."""
    out = {}
    for k, v in sd.items():
        t = torch.from_numpy(np.array(v))
        out[k] = t.to(dtype) if (dtype is not None and t.is_floating_point()) else t
    return out


def unit_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def param_keys(sd):
    return [k for k in sd if k.endswith((".weight", ".bias"))]


def pre_bn_bias_keys(n_enc):
    return [enc_key(i) + ".bias" for i in range(n_enc - 1)]


def fixture_inputs():
    """dict(train_sd, batches [STEPS, BATCH, FEATURE], eval_sd, eval_rows [EVAL_ROWS, FEATURE])."""
    return dict(train_sd=state_dict_np(FEATURE, ENC, DEC, FIXTURE_SEED),
                batches=unit_rows(STEPS * BATCH, FEATURE, FIXTURE_SEED + 1).reshape(STEPS, BATCH, FEATURE),
                eval_sd=state_dict_np(FEATURE, ENC, DEC, FIXTURE_SEED + 2, running=True),
                eval_rows=unit_rows(EVAL_ROWS, FEATURE, FIXTURE_SEED + 3))


def adam_step_bound(lr, betas=BETAS):
    """Adam's own bound on one update of one element."""
    return lr * max(1.0, (1 - betas[0]) / np.sqrt(1 - betas[1]))
