#!/usr/bin/env python3
"""The 'lang' stages' loss at the headline image size (csrc/lang_loss.hip): 1352 x 1014 pixels, with
(V = 2, C = 32) and (V = 1, C = 3), L1-only and with the cosine term, forward plus backward.

Paths on the same card in one process, alternating, ROUNDS rounds each after a warm-up, timed with
device events around forward + backward:
  native   segment_lang_loss on (language image, segment map, feature table)
  dense    the torch expression TrainStep.loss runs on gt_lang and lang_mask already on the device
  l1       lsr_l1_loss_views forward + backward over images of the same size: the yardstick for a
           streaming kernel of this shape
and, apart, the dense path's extra host-to-device copy of one view's gt_lang (pageable memory, as the
reference's `.cuda()` every iteration).
Prints one JSON line (and writes it to --out): ms of each path (median, min, max of the rounds), the
bytes each algorithm needs (native: forward V (4 C HW + 4 HW), backward the same plus 4 C HW written
per view; l1: 8 C HW forward, 12 C HW backward per view), the achieved GB/s, the native rate as a
fraction of the l1 kernels', and each path's peak memory above what was
allocated before it (the gradient images included)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4dlangsplat_amd"))

import torch  # noqa: E402

from language_supervision import SegmentSupervision, native_eligible, segment_lang_loss  # noqa: E402
from train_step import _L1Views  # noqa: E402

LAM, BETA = 0.2, 0.01


def blocky_map(H, W, S, gen, dev):
    """[H, W] int32: 16 x 24 pixel blocks of one random segment each, a tenth of the pixels unlabelled."""
    ids = torch.randint(0, S, ((H + 15) // 16, (W + 23) // 24), generator=gen, device=dev, dtype=torch.int32)
    seg = ids.repeat_interleave(16, 0).repeat_interleave(24, 1)[:H, :W].clone()
    seg[torch.rand(H, W, generator=gen, device=dev) < 0.1] = -1
    return seg.contiguous()


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1352)
    ap.add_argument("--height", type=int, default=1014)
    ap.add_argument("--segments", type=int, default=700)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lang_loss.py measures on the GPU; none found")
    dev = torch.device("cuda")
    H, W, S = a.height, a.width, a.segments
    gen = torch.Generator(device=dev).manual_seed(1)
    res = {"workload": {"width": W, "height": H, "segments": S, "rounds": a.rounds, "lam": LAM, "beta": BETA},
           "device": torch.cuda.get_device_name(0), "cases": []}
    for V, C in ((2, 32), (1, 3)):
        xs = [torch.randn(C, H, W, generator=gen, device=dev).requires_grad_(True) for _ in range(V)]
        sups = [SegmentSupervision(blocky_map(H, W, S, gen, dev), torch.randn(S, C, generator=gen, device=dev))
                for _ in range(V)]
        assert native_eligible(xs, sups)
        dense = [s.dense() for s in sups]
        gt, mask = torch.stack([g for g, _ in dense]), torch.stack([m for _, m in dense])
        del dense
        plane = C * H * W * 4
        for cos in (False, True):
            def native():
                return segment_lang_loss(xs, sups, LAM, BETA, addcosloss=cos)

            def dense_torch():
                lang = torch.stack(xs)
                p, q = lang * mask, gt * mask
                loss = LAM * (p - q).abs().mean()
                if cos:
                    loss = loss + BETA * (1 - torch.nn.functional.cosine_similarity(p, q, dim=-1).mean())
                return loss

            def l1():
                return _L1Views.apply(gt, *xs)

            def step(fn):
                for x in xs:
                    x.grad = None
                fn().backward()

            paths = {"native": native, "dense": dense_torch, "l1": l1}
            times, peaks, losses = {k: [] for k in paths}, {}, {}
            for k, fn in paths.items():                      # warm-up, and each path's peak memory
                step(fn)
                loss = None                                  # the previous path's graph, if anything of it is left
                for x in xs:
                    x.grad = None
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                loss = fn()
                loss.backward()
                torch.cuda.synchronize()
                peaks[k] = torch.cuda.max_memory_allocated() - before
                losses[k] = float(loss.detach())
            for _ in range(a.rounds):
                for k, fn in paths.items():
                    times[k].append(timed(lambda: step(fn)))
            need = {"native": V * (2 * (plane + 4 * H * W) + plane), "l1": V * 5 * plane}
            case = {"V": V, "C": C, "with_cos": cos, "image_bytes_per_view": plane,
                    "loss": {k: losses[k] for k in ("native", "dense")}}
            for k in paths:
                med = statistics.median(times[k])
                case[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4),
                           "ms_max": round(max(times[k]), 4), "peak_memory_bytes": int(peaks[k])}
                if k in need:
                    case[k]["algorithm_bytes"] = int(need[k])
                    case[k]["gb_per_s"] = round(need[k] / (med * 1e-3) / 1e9, 1)
            case["native_rate_over_l1_rate"] = round(case["native"]["gb_per_s"] / case["l1"]["gb_per_s"], 3)
            case["speedup_vs_dense"] = round(case["dense"]["ms_median"] / case["native"]["ms_median"], 2)
            res["cases"].append(case)
        # the copy the dense form pays per view and iteration on top (scene/cameras.py:118)
        host = gt[0].cpu()
        copies = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            host.to(dev)
            torch.cuda.synchronize()
            copies.append((time.perf_counter() - t) * 1e3)
        res["cases"][-1]["gt_lang_host_to_device_ms_per_view"] = round(statistics.median(copies), 3)
        res["cases"][-2]["gt_lang_host_to_device_ms_per_view"] = round(statistics.median(copies), 3)
        del xs, sups, gt, mask, host
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
