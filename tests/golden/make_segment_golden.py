#!/usr/bin/env python3
"""Writes tests/golden/segment_golden.npz from the reference implementation's own code, on the CPU:

    python tests/golden/make_segment_golden.py --reference /path/to/4DLangSplat

It needs the reference checkout, so it runs where the fixture is made, not in the test suite.

What is the reference's own code and what is restated:
  * blended, the level choice, the chosen IoU and the level scores come from eval/eval.py's
    activate_stream, unchanged, called once per strategy and dtype.  eval.py is imported with cv2,
    jaxtyping, torchvision, open_clip, mediapy, sentence_transformers and seaborn registered as stub
    modules (none of them is touched by activate_stream without visualisation).  The annotations
    go in through the module global img_ann; the stand-in clip_model's get_max_across returns a tensor
    the generator keeps: activate_stream overwrites it in place with the blended maps.
  * activate_stream returns masks and IoU of the chosen level only, and keeps its scores in a float32
    tensor whatever the input's dtype.  mask_raw, mask, inter, union of every level and the float64
    scores are therefore the same reference lines (eval.py:185-189, 241-251, 260) applied to that
    blended tensor here, with the reference's smooth_cuda for the 7 x 7 cleaning; the generator
    asserts that the chosen level's mask and IoU and the float32 scores agree with what
    activate_stream returned.
  * the "mean" strategy: activate_stream's byte-array indexing valid_map[i, k][uint8 array]
    (eval.py:271) runs with the installed torch (as a mask, with a deprecation warning), so the "mean"
    scores stored at float32 precision are the reference's own; their float64 values restate
    eval.py:266-271 as blended[mask_raw].mean() in float64, checked against them.

Stored: the float64 run's results, the float32 run's max error against it for blended and both scores
(the "float32 reference error" the GPU tests' tolerance is a multiple of), and a checksum of the inputs
(tests/segment_cases.py).
"""
import argparse
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import segment_cases as sc  # noqa: E402

THRESH, SCALE = 0.4, 29


class _Anything:
    """Subscriptable, callable, attribute-bearing: whatever an import-time use of a stub needs."""
    def __getitem__(self, k):
        return self

    def __call__(self, *a, **k):
        return self

    def __getattr__(self, k):
        return self


class _Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _Anything()


def import_reference(root):
    for name in ("cv2", "jaxtyping", "torchvision", "open_clip", "mediapy", "sentence_transformers", "seaborn"):
        sys.modules.setdefault(name, _Stub(name))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "eval"))
    import eval as ref_eval
    import eval_utils
    return ref_eval, eval_utils


class StandInClip:
    def __init__(self, maps, phrases):
        self.maps, self.positives = maps, phrases

    def get_max_across(self, sem_map):
        return self.maps


def run(ref_eval, eval_utils, rel, gt, dtype, strategy):
    L, K, H, W = rel.shape
    phrases = [f"phrase {k}" for k in range(K)]
    maps = torch.from_numpy(rel).to(dtype).clone()
    ref_eval.img_ann = {p: {"mask": gt[k]} for k, p in enumerate(phrases)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        iou_list, lvl_list, per_phrase, mask_dict, raw_dict = ref_eval.activate_stream(
            None, None, StandInClip(maps, phrases), None, thresh=THRESH, scale=SCALE, chose_mask_strategy=strategy)
    blended = maps                                     # overwritten in place (eval.py:175)
    raw = torch.zeros(L, K, H, W, dtype=torch.uint8)
    mask = torch.zeros(L, K, H, W, dtype=torch.uint8)
    inter = torch.zeros(L, K, dtype=torch.int64)
    union = torch.zeros(L, K, dtype=torch.int64)
    score = torch.zeros(L, K, dtype=dtype)
    for k in range(K):
        inside = torch.from_numpy(gt[k] != 0)
        for i in range(L):
            o = blended[i, k] - blended[i, k].min()
            o = o / (o.max() + 1e-9)
            o = torch.clip(o * 2.0 + (-1.0), 0, 1)
            raw[i, k] = (o > THRESH).to(torch.uint8)
            mask[i, k] = eval_utils.smooth_cuda(raw[i, k])
            inter[i, k] = (inside & mask[i, k].bool()).sum()
            union[i, k] = (inside | mask[i, k].bool()).sum()
            if strategy == "point":
                score[i, k] = blended[i, k].max()
            else:
                area = raw[i, k].bool()
                score[i, k] = blended[i, k][area].mean() if bool(area.any()) else 0.0
    level = torch.tensor([int(l) for l in lvl_list])
    chosen_iou = torch.stack([torch.as_tensor(x) for x in iou_list]).float()
    for k, p in enumerate(phrases):                    # the restated lines agree with what activate_stream returned
        iou, lvl, scores, _ = per_phrase[p]
        assert torch.equal(mask_dict[p].to(torch.uint8), mask[level[k], k])
        assert torch.equal(raw_dict[p][0].to(torch.uint8), raw[level[k], k])
        assert float(iou) == float((inter[level[k], k].float() / union[level[k], k].float()))
        assert np.array_equal(np.asarray(scores, np.float32), score[:, k].float().numpy()), (scores, score[:, k])
        assert int(torch.argmax(score[:, k])) == int(level[k])
    return dict(blended=blended, raw=raw, mask=mask, inter=inter, union=union, score=score, level=level,
                chosen_iou=chosen_iou)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds eval/eval.py)")
    ap.add_argument("--out", default=os.path.join(HERE, "segment_golden.npz"))
    a = ap.parse_args()
    ref_eval, eval_utils = import_reference(os.path.abspath(a.reference))
    rel, gt = sc.fixture_inputs()
    out = {"inputs_sha256": sc.checksum([rel, gt]), "thresh": THRESH, "scale": SCALE}
    for strategy in ("point", "mean"):
        r64 = run(ref_eval, eval_utils, rel, gt, torch.float64, strategy)
        r32 = run(ref_eval, eval_utils, rel, gt, torch.float32, strategy)
        for key in ("raw", "mask", "inter", "union", "level"):
            assert torch.equal(r64[key], r32[key]), f"{strategy}: float32 and float64 {key} differ"
        if strategy == "point":
            out.update(blended=r64["blended"].numpy(), mask_raw=r64["raw"].numpy(), mask=r64["mask"].numpy(),
                       inter=r64["inter"].numpy(), union=r64["union"].numpy(),
                       blended_f32_err=float((r32["blended"].double() - r64["blended"]).abs().max()))
        out[f"score_{strategy}"] = r64["score"].numpy()
        out[f"score_{strategy}_f32_err"] = float((r32["score"].double() - r64["score"]).abs().max())
        out[f"level_{strategy}"] = r64["level"].numpy()
        out[f"chosen_iou_{strategy}"] = r64["chosen_iou"].numpy()
        frac = float(r64["raw"].float().mean())
        iou = (r64["inter"].double() / r64["union"].double()).numpy()
        print(f"{strategy}: {frac:.3f} of the pixels above threshold, IoU {np.round(iou, 3).tolist()}, "
              f"levels {r64['level'].tolist()}, float32 errors blended "
              f"{float((r32['blended'].double() - r64['blended']).abs().max()):.3g} score {out[f'score_{strategy}_f32_err']:.3g}")
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
