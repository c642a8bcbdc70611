"""Generate tests/golden/query_golden.npz: the REFERENCE's open-vocabulary query on seeded inputs,
run in the build container only (/root/reference does not exist on the GPU box).  The fixture is
data: seeds, a checksum of the regenerated weights, and the reference's results.

What runs is the reference's own code, unchanged, on the CPU:
  * autoencoder.model.Autoencoder.decode (autoencoder/model.py:42-46) with the seeded decoder
    weights loaded into its `decoder` ModuleList;
  * eval.openclip_encoder.OpenCLIPNetwork.get_max_across / get_relevancy
    (eval/openclip_encoder.py:41-56, 96-112).  The class's constructor downloads a CLIP model, so
    the object is made with OpenCLIPNetwork.__new__ and its `positives`, `negatives`, `pos_embeds`
    and `neg_embeds` are set by hand; the module's imports of open_clip and torchvision (absent
    here, never called by these two methods) are registered as empty modules.
Both run in float64 (the stored results) and again in float32: the float32 run's max abs error
against float64 is stored beside each result, and the tests bound the native error by a multiple
of it.

Inputs (tests/query_cases.py, shared with the tests): decoder 3 -> 16 -> 32 -> 64 -> 128 -> 256 ->
512, L = 3 levels of 37 x 29 latents uniform in (-1, 1), 5 positives and 4 negatives.

    python tests/golden/make_query_golden.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "query_golden.npz")

sys.path.insert(0, os.path.join(ROOT, "tests"))
import query_cases as qc  # noqa: E402


def reference_modules():
    for name in ("open_clip", "torchvision"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "eval"))
    from autoencoder.model import Autoencoder
    from openclip_encoder import OpenCLIPNetwork
    return Autoencoder, OpenCLIPNetwork


def run(Autoencoder, OpenCLIPNetwork, inp, dtype):
    """(features at the sampled pixels [64, 512], relevancy [L, n_pos, H, W]) in `dtype`."""
    with contextlib.redirect_stdout(io.StringIO()):           # the constructor prints its layers
        model = Autoencoder([256, 128, 64, 32, qc.FIXTURE_DIMS[0]], qc.DEFAULT_DECODER)
    missing, unexpected = model.load_state_dict(qc.state_dict(inp["ws"], inp["bs"], torch), strict=False)
    assert not unexpected and all(k.startswith("encoder.") for k in missing), (missing, unexpected)
    model = model.to(dtype).eval()
    net = OpenCLIPNetwork.__new__(OpenCLIPNetwork)
    net.positives = tuple(f"positive {i}" for i in range(qc.FIXTURE_POS))
    net.negatives = ("object", "things", "stuff", "texture")
    net.pos_embeds = torch.from_numpy(inp["pos"]).to(dtype)
    net.neg_embeds = torch.from_numpy(inp["neg"]).to(dtype)
    sem_feat = torch.from_numpy(inp["latent"]).to(dtype)
    with torch.no_grad():
        lvl, h, w, _ = sem_feat.shape
        restored = model.decode(sem_feat.flatten(0, 2))       # eval/eval.py:616
        relev = net.get_max_across(restored.view(lvl, h, w, -1))
    return restored[torch.from_numpy(inp["samples"])].numpy(), relev.numpy()


def main():
    Autoencoder, OpenCLIPNetwork = reference_modules()
    inp = qc.fixture_inputs()
    f64, r64 = run(Autoencoder, OpenCLIPNetwork, inp, torch.float64)
    f32, r32 = run(Autoencoder, OpenCLIPNetwork, inp, torch.float32)
    assert f64.dtype == np.float64 and r64.dtype == np.float64 and f32.dtype == np.float32
    L, H, W = qc.FIXTURE_LHW
    assert r64.shape == (L, qc.FIXTURE_POS, H, W) and f64.shape == (qc.FIXTURE_SAMPLES, qc.FIXTURE_DIMS[-1])
    feat_err = float(np.abs(f32.astype(np.float64) - f64).max())
    rel_err = float(np.abs(r32.astype(np.float64) - r64).max())
    np.savez_compressed(OUT, seed=np.int64(qc.FIXTURE_SEED), dims=np.array(qc.FIXTURE_DIMS, np.int64),
                        lhw=np.array(qc.FIXTURE_LHW, np.int64), n_pos=np.int64(qc.FIXTURE_POS),
                        n_neg=np.int64(qc.FIXTURE_NEG), samples=inp["samples"].astype(np.int64),
                        weights_sha256=np.array(qc.checksum(inp["ws"] + inp["bs"])),
                        inputs_sha256=np.array(qc.checksum([inp["latent"], inp["pos"], inp["neg"]])),
                        relevancy=r64, features=f64, relevancy_f32_err=np.float64(rel_err),
                        features_f32_err=np.float64(feat_err))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; relevancy in [{r64.min():.3f}, {r64.max():.3f}]; "
          f"float32 reference error: features {feat_err:.3g}, relevancy {rel_err:.3g}")


if __name__ == "__main__":
    main()
