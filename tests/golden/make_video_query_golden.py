#!/usr/bin/env python3
"""Writes tests/golden/video_query_golden.npz from the reference implementation's own code, on the CPU:

    python tests/golden/make_video_query_golden.py --reference /path/to/4DLangSplat

It needs the reference checkout, so it runs where the fixture is made, not in the test suite.

What is the reference's own code and what is restated:
  * the per-mask similarities come from eval/eval.py's cal_avg_video_feature, unchanged, with the
    reference's own Autoencoder(..., feature_dim=4096) (autoencoder/model.py) holding the seeded decoder
    weights, once in float64 and once in float32.  eval.py is imported with cv2, jaxtyping, torchvision,
    open_clip, mediapy, sentence_transformers and seaborn registered as stub modules, as
    make_segment_golden.py does; sklearn is installed, so cosine_similarity is the real one.
  * the frame metrics come from eval/eval.py's evaluate_video_feature, unchanged.
  * two pieces of eval.py live inside its `if __name__ == '__main__':` block and cannot be imported:
    assert_idx_in_list (:704-708) and the smoothing loop with the two threshold rules (:719-760).  They are
    restated here in this file's own words (in_intervals, smooth, sequence); evaluate_video_feature looks
    assert_idx_in_list up as a module global when it is called, so the restated one is set on the imported
    module under that name.

Stored: the float64 similarities and pixel counts, the float32 run's max error against them (the "float32
reference error" the GPU tests' tolerance is a multiple of), checksums of the inputs
(tests/video_query_cases.py), and as JSON text the recorded results of evaluate_video_feature, of the
smoothing and of one whole sequence.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import video_query_cases as vc  # noqa: E402
from make_segment_golden import import_reference  # noqa: E402  (the same stub modules)


def in_intervals(idx, intervals):
    """A frame is labelled if some interval holds it, both ends included."""
    return any(lo <= idx <= hi for lo, hi in intervals)


def smooth(values, coeffs):
    """A window of len(coeffs) centred on each frame; a frame whose window would leave the list keeps its
    raw value."""
    half = len(coeffs) // 2
    out = []
    for i, v in enumerate(values):
        if i - half < 0 or i + half >= len(values):
            out.append(v)
        else:
            acc = 0
            for j in range(-half, half + 1):
                acc += values[i + j] * coeffs[j + half]
            out.append(acc)
    return out


def similarities(ref_eval, Autoencoder, inp, dtype):
    with contextlib.redirect_stdout(io.StringIO()):            # the constructor prints its layers
        model = Autoencoder([2048, 1024, 512, 256, 128, 64, 32, vc.FULL_DIMS[0]], vc.FULL_DIMS[1:], feature_dim=4096)
    missing, unexpected = model.load_state_dict(vc.state_dict(inp["ws"], inp["bs"], torch), strict=False)
    assert not unexpected and all(k.startswith("encoder.") for k in missing), (missing, unexpected)
    model = model.to(dtype).eval()
    lat = torch.from_numpy(inp["latent"]).to(dtype)
    out = []
    with torch.no_grad():
        for k in range(inp["masks"].shape[0]):
            q = inp["queries"][k].astype(np.float64 if dtype == torch.float64 else np.float32)
            out.append(float(ref_eval.cal_avg_video_feature(model, torch.from_numpy(inp["masks"][k]), lat, q)))
    return np.array(out, np.float64)


def sequence(ref_eval, c, coeffs):
    """eval.py:719-769 for one phrase: sort, smooth, the two threshold rules, evaluate_video_feature."""
    video = sorted(zip(c["ids"], c["sims"], c["ious"]), key=lambda t: t[0])
    clip = sorted(zip(c["ids"], c["clip"], c["ious"]), key=lambda t: t[0])
    video_thresh = sum(c["sims"]) / len(c["sims"])             # the unsmoothed list
    if coeffs is not None:
        video = [(t[0], s, t[2]) for t, s in zip(video, smooth([t[1] for t in video], coeffs))]
        clip = [(t[0], s, t[2]) for t, s in zip(clip, smooth([t[1] for t in clip], coeffs))]
    clip_thresh = sum(t[1] for t in clip) / len(clip)          # the smoothed list
    return dict(video_thresh=video_thresh, clip_thresh=clip_thresh, smoothed=[t[1] for t in video],
                clip_smoothed=[t[1] for t in clip],
                video=ref_eval.evaluate_video_feature(video, c["intervals"], video_thresh),
                clip=ref_eval.evaluate_video_feature(clip, c["intervals"], clip_thresh))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds eval/eval.py)")
    ap.add_argument("--out", default=os.path.join(HERE, "video_query_golden.npz"))
    a = ap.parse_args()
    root = os.path.abspath(a.reference)
    ref_eval, _ = import_reference(root)
    from autoencoder.model import Autoencoder
    ref_eval.assert_idx_in_list = in_intervals

    inp = vc.fixture_inputs()
    s64 = similarities(ref_eval, Autoencoder, inp, torch.float64)
    s32 = similarities(ref_eval, Autoencoder, inp, torch.float32)
    counts = (inp["masks"] == 1).reshape(inp["masks"].shape[0], -1).sum(axis=1)

    evals = {}
    for name, c in vc.eval_cases().items():
        frames = list(zip(c["ids"], c["sims"], c["ious"]))
        evals[name] = ref_eval.evaluate_video_feature(frames, c["intervals"], c["thresh"])
    smooths = {name: smooth(c["values"], c["coeffs"]) for name, c in vc.smooth_cases().items()}
    seq = vc.sequence_case()
    seqs = {"none": sequence(ref_eval, seq, None), "three": sequence(ref_eval, seq, vc.COEFFS[0]),
            "five": sequence(ref_eval, seq, vc.COEFFS[1])}

    np.savez_compressed(
        a.out, seed=np.int64(vc.FIXTURE_SEED), dims=np.array(vc.FULL_DIMS, np.int64),
        weights_sha256=np.array(vc.checksum(inp["ws"] + inp["bs"])),
        inputs_sha256=np.array(vc.checksum([inp["latent"], inp["masks"], inp["queries"]])),
        host_sha256=np.array(vc.checksum([np.frombuffer(json.dumps(
            [vc.eval_cases(), vc.smooth_cases(), vc.sequence_case()], sort_keys=True).encode(), np.uint8)])),
        similarity=s64, counts=counts.astype(np.int64), similarity_f32_err=np.float64(np.abs(s32 - s64).max()),
        evaluate=np.array(json.dumps(evals)), smooth=np.array(json.dumps(smooths)), sequence=np.array(json.dumps(seqs)))
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes; similarities {s64.tolist()}, counts {counts.tolist()}, "
          f"float32 reference error {np.abs(s32 - s64).max():.3g}")
    for name, r in evals.items():
        print(name, {k: v for k, v in r.items() if not k.endswith("_list")})


if __name__ == "__main__":
    main()
