#!/usr/bin/env python3
"""The HexPlane regularisers (csrc/plane_reg.hip, plane_regularizer.py) at the sizes the configs train at:
  neu3d     resolution [64, 64, 64, 150], multires [1, 2]         (arguments/neu3d/default.py), 16 channels
  default   resolution [64, 64, 64, 25],  multires [1, 2, 4, 8]   (arguments/__init__.py), 16 channels
with the Neu3D weights (time_smoothness_weight 1e-3, l1_time_planes 1e-4, plane_tv_weight 2e-4), the gradient
accumulated onto the field's gradient buffers as TrainStep does.

All sides are timed on the same card in one process on the same tensors, ROUNDS rounds after a warm-up,
alternating, with device events around a window of back-to-back calls (200 fused, 20 of the others; the time per
call is the window's over the count, so a side whose launches the host cannot enqueue fast enough pays for that,
as it does in the training loop):
  fused      plane_regularizer.regularize_planes: every plane in one stencil launch and one finishing launch
  torch      plane_regularizer.regularize_planes_torch: the same formulas and the closed-form gradient as torch
             ops, plane by plane (the path CPU and float64 inputs take)
  autograd   the reference's expression (compute_plane_smoothness, abs(1 - t).mean(), the weighted sums) written
             as torch ops on planes that require a gradient, with backward(): what a caller had to write before
Prints one JSON line (and writes it to --out): ms per call (median, min, max of the rounds), the speed-ups, the
bytes the fused call needs (each plane read once, its gradient read and written once) and what share of the HBM
peak that is at the measured time.

With --loop N it also runs the configs[4] stand-in training loop (tools/bench_train_loop.py's scene) for
--segments rounds of N iterations with plane_reg off, fused and torch in turn, one process, one scene, and
reports iterations/s per segment."""
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

from plane_regularizer import SPATIAL_PLANES, TIME_PLANES, regularize_planes, regularize_planes_torch  # noqa: E402

HBM_PEAK = 8.0e12                       # MI355X HBM3E (spec), bytes/s
WEIGHTS = (1e-3, 1e-4, 2e-4)            # arguments/neu3d/default.py:11-13
FIELDS = {"neu3d": ([64, 64, 64, 150], [1, 2]), "default": ([64, 64, 64, 25], [1, 2, 4, 8])}
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def make_planes(resolution, multires, dev, gen, channels=16):
    """A field's planes a little into training: spatial U(0.1, 0.5), time planes 1 with half the entries moved."""
    planes = []
    for m in multires:
        reso = [r * m for r in resolution[:3]] + [resolution[3]]
        scale = []
        for c0, c1 in PAIRS:
            shape = (1, channels, reso[c1], reso[c0])
            if c1 == 3:
                t = torch.ones(shape, device=dev)
                hit = torch.rand(shape, device=dev, generator=gen) < 0.5
                t = torch.where(hit, t + 1e-2 * torch.randn(shape, device=dev, generator=gen), t)
            else:
                t = torch.rand(shape, device=dev, generator=gen) * 0.4 + 0.1
            scale.append(t.contiguous())
        planes.append(scale)
    return planes


def reference_expression(planes, weights):
    """GaussianModel.compute_regulation (scene/gaussian_model.py:763-802) as torch ops."""
    tsw, l1w, tvw = weights

    def smooth(t):
        first = t[..., 1:, :] - t[..., :-1, :]
        second = first[..., 1:, :] - first[..., :-1, :]
        return torch.square(second).mean()
    plane = sum(smooth(s[ci]) for s in planes for ci in SPATIAL_PLANES)
    tm = sum(smooth(s[ci]) for s in planes for ci in TIME_PLANES)
    l1 = sum(torch.abs(1 - s[ci]).mean() for s in planes for ci in TIME_PLANES)
    return tvw * plane + tsw * tm + l1w * l1


REPS = {"fused": 200, "torch": 20, "autograd": 20}   # calls per timed window


def field_case(name, rounds, dev, gen):
    resolution, multires = FIELDS[name]
    planes = make_planes(resolution, multires, dev, gen)
    grads = [[torch.zeros_like(t) for t in s] for s in planes]
    leaves = [[t.clone().requires_grad_(True) for t in s] for s in planes]
    n = sum(t.numel() for s in planes for t in s)

    def autograd_side():
        for s in leaves:
            for t in s:
                t.grad = None
        total = reference_expression(leaves, WEIGHTS)
        total.backward()
        for sg, sl in zip(grads, leaves):                       # onto the buffers, as the other sides do
            for g, t in zip(sg, sl):
                g += t.grad
        return total

    calls = {"fused": lambda: regularize_planes(planes, WEIGHTS, grads, accumulate=True).total,
             "torch": lambda: regularize_planes_torch(planes, WEIGHTS, grads, accumulate=True).total,
             "autograd": autograd_side}
    times = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(REPS[k]):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) / REPS[k])
    case = {"field": {"resolution": resolution, "multires": multires, "planes": 6 * len(multires), "elements": n},
            "calls_per_window": REPS}
    for k, v in times.items():
        case[k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    # the sides answer the same question
    for s in grads:
        for g in s:
            g.zero_()
    a = regularize_planes(planes, WEIGHTS, grads, accumulate=False)
    ga = [g.clone() for s in grads for g in s]
    b = regularize_planes_torch(planes, WEIGHTS, grads, accumulate=False)
    gb = [g for s in grads for g in s]
    case["total_fused"], case["total_torch"] = float(a.total), float(b.total)
    case["gradient_max_rel_diff_vs_torch"] = max(float((x - y).abs().max() / y.abs().max().clamp(min=1e-30))
                                                 for x, y in zip(ga, gb))
    need = 12 * n                                               # plane read, gradient read and written
    med = case["fused"]["ms_median"] * 1e-3
    case["fused"]["algorithm_bytes"] = need
    case["fused"]["gb_per_s"] = round(need / med / 1e9, 1)
    case["fused"]["share_of_hbm_peak"] = round(need / HBM_PEAK / med, 4)
    case["speedup_vs_torch"] = round(case["torch"]["ms_median"] / case["fused"]["ms_median"], 1)
    case["speedup_vs_autograd"] = round(case["autograd"]["ms_median"] / case["fused"]["ms_median"], 1)
    return case


def torch_regularize(field):
    """field.regularize on the torch formulation: the 'torch' row of the loop."""
    def regularize(weights, accumulate=True):
        S = range(len(field.multires))
        planes = [[field.p[f"grid.grids.{s}.{ci}"] for ci in range(6)] for s in S]
        grads = [[field.grads[f"grid.grids.{s}.{ci}"] for ci in range(6)] for s in S]
        return regularize_planes_torch(planes, weights, grads, accumulate)
    return regularize


def set_plane_reg(step, mode):
    """Switch a TrainStep between plane_reg off, the fused call and the torch formulation."""
    step.plane_reg = None if mode == "off" else WEIGHTS
    step.field.__dict__.pop("regularize", None)
    if mode == "torch":
        step.field.regularize = torch_regularize(step.field)


def training_loop(iters, segments, dev):
    import bench_train_loop as tl
    args = types.SimpleNamespace(gaussians=100_000, width=1352, height=1014, views=2, cameras=8, frames=4,
                                 point_noise=0.02, densify_until_iter=10_000)
    step, sched, pool, gts, _ = tl.build(args, dev)
    order = torch.Generator().manual_seed(5)
    it, out = 0, []
    for seg in range(-1, segments):                  # segment -1 warms every path up
        for mode in ("off", "fused", "torch"):
            set_plane_reg(step, mode)
            n = 20 if seg < 0 else iters
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                it += 1
                idx = torch.randperm(len(pool), generator=order)[: args.views].tolist()
                step([pool[i] for i in idx], gts[idx], iteration=it)
            torch.cuda.synchronize()
            if seg >= 0:
                out.append({"plane_reg": mode, "iterations": n, "gaussians": step.trainer.P,
                            "iterations_per_s": round(n / (time.perf_counter() - t0), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", nargs="+", default=list(FIELDS), choices=list(FIELDS))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--loop", type=int, default=0, help="iterations per segment of the training loop (0: skip it)")
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plane_reg.py measures on the GPU; none found")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1)
    res = {"workload": {"weights": WEIGHTS, "rounds": a.rounds, "accumulate": True},
           "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "cases": {f: field_case(f, a.rounds, dev, gen) for f in a.fields}}
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
