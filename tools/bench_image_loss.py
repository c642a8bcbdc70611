#!/usr/bin/env python3
"""The image loss with its D-SSIM term at the headline image size (csrc/image_loss.hip): 3 x 1014 x 1352
renders, V = 1, 2 and 8 views, forward plus backward of loss = l1 + 0.2 (1 - ssim).

Paths on the same card in one process, alternating, ROUNDS rounds each after a warm-up, timed with device
events around forward + backward:
  native   image_loss.image_loss_views (lsr_image_loss_views / _backward)
  torch    the same formulas as torch ops (the module's fallback: five grouped 11 x 11 conv2d and the
           elementwise chain, autograd's backward)
  l1       lsr_l1_loss_views forward + backward alone: what the loss costs without the term
Prints one JSON line (and writes it to --out): ms of each path (median, min, max of the rounds); the bytes
the kept design must move (forward: x and y read, three partial-derivative maps written, 20 bytes per
element; backward: the maps, x and y read, the gradient written, 24 bytes per element; l1: 8 + 12), the
achieved GB/s and that as a share of the 8.0 TB/s HBM peak (the floor: bytes over peak bandwidth over the
measured time); each path's peak memory above what was allocated before it (the gradients included).
With --loop N it also runs the configs[4] stand-in training loop (tools/bench_train_loop.py's scene) for
N iterations per segment, alternating lambda_dssim 0 and 0.2 on one trainer, iterations/s per segment."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4dlangsplat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import image_loss as il  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402
from train_step import _L1Views  # noqa: E402

LAMBDA = 0.2
HBM_PEAK = 8.0e12


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def loss_case(V, H, W, rounds, dev, gen):
    C = 3
    gts = torch.rand(V, 4, H, W, generator=gen, device=dev)
    xs = [(gts[v, :3] + 0.15 * torch.randn(C, H, W, generator=gen, device=dev)).clamp(0, 1).requires_grad_(True)
          for v in range(V)]
    gt3 = gts[:, :3]
    assert il.native_eligible(xs, gt3)

    def native():
        return il.image_loss_views(xs, gts, LAMBDA)[0]

    def torch_ops():
        l1, ss, _ = il._fallback(xs, gt3, il.NATIVE_WINDOW)
        return l1 + LAMBDA * (1.0 - ss)

    def l1():
        return _L1Views.apply(gt3, *xs)

    def step(fn):
        for x in xs:
            x.grad = None
        fn().backward()

    paths = {"native": native, "torch": torch_ops, "l1": l1}
    times, peaks, losses = {k: [] for k in paths}, {}, {}
    for k, fn in paths.items():                      # warm-up, and each path's peak memory
        step(fn)
        loss = None
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
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(timed(lambda: step(fn)))
    n = V * C * H * W
    need = {"native": 44 * n, "l1": 20 * n}
    case = {"V": V, "C": C, "elements": n, "loss": {k: losses[k] for k in ("native", "torch")},
            "workspace_bytes": int(_lib.load().lsr_image_loss_workspace_bytes(V, C, H, W))}
    for k in paths:
        med = statistics.median(times[k])
        case[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4),
                   "peak_memory_bytes": int(peaks[k])}
        if k in need:
            case[k]["algorithm_bytes"] = int(need[k])
            case[k]["gb_per_s"] = round(need[k] / (med * 1e-3) / 1e9, 1)
            case[k]["share_of_hbm_floor"] = round(need[k] / HBM_PEAK / (med * 1e-3), 4)
    case["speedup_vs_torch"] = round(case["torch"]["ms_median"] / case["native"]["ms_median"], 2)
    case["cost_over_l1_ms"] = round(case["native"]["ms_median"] - case["l1"]["ms_median"], 4)
    case["peak_memory_torch_minus_native"] = int(peaks["torch"] - peaks["native"])
    del xs, gts
    torch.cuda.empty_cache()
    return case


def training_loop(iters, segments, dev):
    import bench_train_loop as tl
    args = types.SimpleNamespace(gaussians=100_000, width=1352, height=1014, views=2, cameras=8, frames=4,
                                 point_noise=0.02, densify_until_iter=10_000)
    step, sched, pool, gts, _ = tl.build(args, dev)
    order = torch.Generator().manual_seed(5)
    it, out = 0, []
    for seg in range(-1, segments):                  # segment -1 warms both paths up
        for lam in (0.0, LAMBDA):
            step.lambda_dssim = lam
            n = 20 if seg < 0 else iters
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                it += 1
                idx = torch.randperm(len(pool), generator=order)[: args.views].tolist()
                step([pool[i] for i in idx], gts[idx], iteration=it)
            torch.cuda.synchronize()
            if seg >= 0:
                out.append({"lambda_dssim": lam, "iterations": n, "gaussians": step.trainer.P,
                            "iterations_per_s": round(n / (time.perf_counter() - t0), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1352)
    ap.add_argument("--height", type=int, default=1014)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--loop", type=int, default=0, help="iterations per segment of the training loop (0: skip it)")
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_loss.py measures on the GPU; none found")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1)
    res = {"workload": {"width": a.width, "height": a.height, "rounds": a.rounds, "lambda_dssim": LAMBDA},
           "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "cases": [loss_case(V, a.height, a.width, a.rounds, dev, gen) for V in a.views]}
    if a.loop > 0:
        res["training_loop"] = training_loop(a.loop, a.segments, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
