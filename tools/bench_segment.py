#!/usr/bin/env python3
"""Open-vocabulary segmentation at the headline image size (csrc/segment.hip): 1352 x 1014 pixels,
3 levels, 8 phrases, with annotations, scale 29, threshold 0.4, the "point" strategy.

Three paths on the same card in one process, alternating, ROUNDS rounds each after a warm-up, timed
with device events around one frame (all 24 maps), inputs already on the device:
  fused          segment() on the native path
  fused_library  lsr_segment alone on preallocated outputs: the fused path without segment()'s allocations,
                 level choice and gather of the chosen masks
  torch_per_map  the reference's lines as torch ops one map at a time, as eval.py's activate_stream
                 loops (its .cpu() round trips left out)
  torch_batched  the same ops over all maps with one avg_pool2d call per window: the fair torch baseline
Prints one JSON line (and writes it to --out): ms per frame of each path (median, min, max of the
rounds), the fused path's GB/s over its 15 bytes per pixel and map (read the relevancy, write the
blend, read it back, read the annotation, write two byte masks), each path's peak memory above what
was allocated before it, the fused path's agreement with torch_per_map, and whether the fused
path's slowest round is below the batched baseline's fastest (the bar)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4dlangsplat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import segment_cases as sc  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402
from language_query import _segment_torch, segment  # noqa: E402

BYTES_PER_PIXEL_AND_MAP = 15
LANG_LOSS_TBPS = 2.2              # the streaming loss kernel on this card, for orientation only


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1352)
    ap.add_argument("--height", type=int, default=1014)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--phrases", type=int, default=8)
    ap.add_argument("--scale", type=int, default=29)
    ap.add_argument("--thresh", type=float, default=0.4)
    ap.add_argument("--strategy", default="point")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segment.py measures on the GPU; none found")
    L, K, H, W = a.levels, a.phrases, a.height, a.width
    rel_np, gt_np = sc.maps(L, K, H, W, 1)
    rel, gt = torch.from_numpy(rel_np).cuda(), torch.from_numpy(gt_np).cuda()
    gtb = gt != 0
    M = L * K

    def fused():
        return segment(rel, gt, thresh=a.thresh, scale=a.scale, strategy=a.strategy)

    lib = _lib.load()
    out = {"blended": torch.empty(M, H, W, device="cuda"), "mask_raw": torch.empty(M, H, W, dtype=torch.uint8, device="cuda"),
           "mask": torch.empty(M, H, W, dtype=torch.uint8, device="cuda"), "score": torch.empty(M, device="cuda"),
           "inter": torch.empty(M, dtype=torch.int64, device="cuda"), "union": torch.empty(M, dtype=torch.int64, device="cuda"),
           "ws": torch.empty(lib.lsr_segment_workspace_bytes(M, H, W), dtype=torch.uint8, device="cuda")}
    ptrs = [out[k].data_ptr() for k in ("blended", "mask_raw", "mask", "score", "inter", "union", "ws")]

    def fused_library():
        _lib.check(lib.lsr_segment(M, H, W, rel.data_ptr(), a.scale, a.thresh, _lib.SEGMENT_STRATEGIES[a.strategy],
                                   gt.data_ptr(), K, *ptrs, torch.cuda.current_stream().cuda_stream), "lsr_segment")

    def torch_per_map():
        out = []
        for k in range(K):
            for l in range(L):
                out.append(_segment_torch(rel[l, k][None], gtb[k][None], a.thresh, a.scale, a.strategy))
            torch.argmax(torch.stack([o[3][0] for o in out[-L:]]))
        return out

    def torch_batched():
        b, raw, mask, score, inter, union = _segment_torch(rel.reshape(M, H, W), gtb, a.thresh, a.scale, a.strategy)
        return b, raw, mask, score, inter, union, torch.argmax(score.reshape(L, K), dim=0)

    paths = {"fused": fused, "fused_library": fused_library, "torch_per_map": torch_per_map, "torch_batched": torch_batched}
    times = {k: [] for k in paths}
    peaks = {}
    for k, fn in paths.items():                              # warm-up, and each path's peak memory
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        r = fn()
        torch.cuda.synchronize()
        peaks[k] = torch.cuda.max_memory_allocated() - before
        del r
    for _ in range(a.rounds):
        for k, fn in paths.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = fn()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1))
            del r

    # the fused path against the reference's loop
    f, ref = fused(), torch_per_map()
    order = [(l, k) for k in range(K) for l in range(L)]
    agree = {"blended_max_abs_diff": 0.0, "score_max_abs_diff": 0.0, "mask_raw_pixels_differ": 0, "mask_pixels_differ": 0,
             "iou_max_abs_diff": 0.0}
    for (l, k), (b, raw, mask, score, inter, union) in zip(order, ref):
        agree["blended_max_abs_diff"] = max(agree["blended_max_abs_diff"], float((f.blended[l, k] - b[0]).abs().max()))
        agree["score_max_abs_diff"] = max(agree["score_max_abs_diff"], float((f.score[l, k] - score[0]).abs()))
        agree["mask_raw_pixels_differ"] += int((f.mask_raw[l, k] != raw[0]).sum())
        agree["mask_pixels_differ"] += int((f.mask[l, k] != mask[0]).sum())
        agree["iou_max_abs_diff"] = max(agree["iou_max_abs_diff"],
                                        abs(float(f.iou[l, k]) - float(inter[0].float() / union[0].float())))

    res = {"workload": {"width": W, "height": H, "levels": L, "phrases": K, "scale": a.scale, "thresh": a.thresh,
                        "strategy": a.strategy, "rounds": a.rounds, "maps": M,
                        "bytes_per_frame": BYTES_PER_PIXEL_AND_MAP * M * H * W},
           "device": torch.cuda.get_device_name(0)}
    for k in paths:
        res[k] = {"ms_per_frame_median": round(statistics.median(times[k]), 3), "ms_per_frame_min": round(min(times[k]), 3),
                  "ms_per_frame_max": round(max(times[k]), 3), "peak_memory_bytes": int(peaks[k])}
    med = statistics.median(times["fused"])
    res["fused"]["gb_per_s"] = round(BYTES_PER_PIXEL_AND_MAP * M * H * W / (med * 1e-3) / 1e9, 1)
    res["fused_library"]["gb_per_s"] = round(BYTES_PER_PIXEL_AND_MAP * M * H * W
                                             / (statistics.median(times["fused_library"]) * 1e-3) / 1e9, 1)
    res["fused"]["workspace_bytes"] = int(_lib.load().lsr_segment_workspace_bytes(M, H, W))
    res["lang_loss_tb_per_s_for_orientation"] = LANG_LOSS_TBPS
    res["speedup_vs_torch_batched"] = round(res["torch_batched"]["ms_per_frame_median"] / med, 2)
    res["speedup_vs_torch_per_map"] = round(res["torch_per_map"]["ms_per_frame_median"] / med, 2)
    res["bar_fused_max_below_batched_min"] = bool(max(times["fused"]) < min(times["torch_batched"]))
    res["fused_vs_torch_per_map"] = agree
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
