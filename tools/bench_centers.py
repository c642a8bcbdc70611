#!/usr/bin/env python3
"""The status centres at the headline size (csrc/deform_lang.hip k_centers_from_field): P = 2M Gaussians,
S = 100 sample times, K = 3 centres, lang_dim D = 3 and D = 6, a RESIDUAL field.

Both sides are timed on the same card in one process, ROUNDS rounds after a warm-up, alternating, with
device events around each call:
  fused     language_centers.sample_centers: times, lang_deform and the k-means in one kernel
  kmeans    language_centers.kmeans_rows on samples already in memory ([P, S, D])
  torch     the same formulas as torch ops: S calls of DeformationField.forward (the language output,
            one time per call, as the reference's loop does), stacked to [P, S, D], then the maximin
            seeding and Lloyd iterations batched over rows in chunks (--chunk rows at a time), run
            until no row's assignment changes or max_iter
Prints one JSON line (and writes it to --out): ms per call (median, min, max of the rounds), the ratio,
and the fused call's time against an arithmetic floor: the MLP's 128 x 128 layer is 2 * 128 * 128 * S
= 3.3 MFLOP per Gaussian at S = 100 (3.7 with the input and output layers), three MFMA products for the
hi / lo split, on the 2.5 PFLOP/s dense bf16 peak."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4dlangsplat_amd"))

import torch  # noqa: E402

from deformation import LANG_RESIDUAL, DeformationField  # noqa: E402
from language_centers import kmeans_rows, sample_centers  # noqa: E402

BF16_PEAK_FLOPS = 2.5e15    # MI355X dense bf16 MFMA (spec)
RES, MULTIRES = [64, 64, 64, 75], [1, 2]
AABB = [[7.0, 5.5, 10.5], [-7.0, -5.5, 1.5]]


def torch_kmeans(x, K, max_iter, chunk):
    """include/lsr_centers.h as batched torch ops on x [P, S, D]: centres [P, K, D]."""
    out = torch.empty(x.shape[0], K, x.shape[2], device=x.device)
    for p0 in range(0, x.shape[0], chunk):
        xs = x[p0:p0 + chunk]
        rows = torch.arange(xs.shape[0], device=x.device)
        d2 = lambda c: ((xs - c[:, None]) ** 2).sum(dim=2)   # noqa: E731
        c = [xs[rows, d2(xs.mean(dim=1)).argmax(dim=1)]]
        mind = d2(c[0])
        for _ in range(1, K):
            c.append(xs[rows, mind.argmax(dim=1)])
            mind = torch.minimum(mind, d2(c[-1]))
        c = torch.stack(c, dim=1)
        a = torch.cdist(xs, c).argmin(dim=2)
        for _ in range(max_iter):
            onehot = torch.nn.functional.one_hot(a, K).to(xs.dtype)                  # [p, S, K]
            n = onehot.sum(dim=1)                                                      # [p, K]
            mean = torch.einsum("psk,psd->pkd", onehot, xs) / n.clamp(min=1)[:, :, None]
            c = torch.where((n > 0)[:, :, None], mean, c)
            a_new = torch.cdist(xs, c).argmin(dim=2)
            done = bool((a_new == a).all())
            a = a_new
            if done:
                break
        out[p0:p0 + chunk] = c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=2_000_000)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--centers", type=int, default=3)
    ap.add_argument("--dims", type=int, nargs="+", default=[3, 6])
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=250_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_centers.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    P, S, K = a.gaussians, a.samples, a.centers
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)   # noqa: E731
    lo, hi = torch.tensor(AABB[1], device=dev), torch.tensor(AABB[0], device=dev)
    means = lo + (hi - lo) * torch.rand(P, 3, generator=g, device=dev)
    scales, rots, opac, shs = r(P, 3), r(P, 4), r(P, 1), r(P, 16, 3)
    res = {"workload": {"gaussians": P, "samples": S, "centers": K, "max_iter": a.max_iter, "rounds": a.rounds,
                        "field": {"resolution": RES, "multires": MULTIRES, "lang_mode": "residual"}},
           "device": torch.cuda.get_device_name(0)}
    for D in a.dims:
        p = DeformationField.init_params(RES, MULTIRES, AABB, seed=1, lang_mode=LANG_RESIDUAL, lang_dim=D)
        field = DeformationField({k: v.to(dev) for k, v in p.items()}, RES, MULTIRES, lang_mode=LANG_RESIDUAL, lang_dim=D)
        lang = r(P, D)
        unit = lang / (lang.norm(dim=-1, keepdim=True) + 1e-9)
        xs, ts = sample_centers(field, lang, k=K, samples=S, seed=0, max_iter=a.max_iter, debug=True)[4:]

        def torch_side():
            rows = [field.forward(means, scales, rots, opac, shs, unit, ts[:, s].contiguous())[5] for s in range(S)]
            return torch_kmeans(torch.stack(rows, dim=1), K, a.max_iter, a.chunk)

        calls = {"fused": lambda: sample_centers(field, lang, k=K, samples=S, seed=0, max_iter=a.max_iter),
                 "kmeans": lambda: kmeans_rows(xs, K, max_iter=a.max_iter),
                 "torch": torch_side}
        times = {k: [] for k in calls}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize()
                times[k].append(t0.elapsed_time(t1))
        c, n, inertia, it = calls["fused"]()
        one = {k: {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}
               for k, v in times.items()}
        kin = D + 1 + 2 * field.time_pe
        flop = 2.0 * S * (kin * 128 + 128 * 128 + 128 * D) * 3 * P
        one["mlp_floor_ms"] = round(flop / BF16_PEAK_FLOPS * 1e3, 3)
        one["fraction_of_bf16_peak"] = round(one["mlp_floor_ms"] / one["fused"]["ms_median"], 4)
        one["speedup_vs_torch"] = round(one["torch"]["ms_median"] / one["fused"]["ms_median"], 1)
        one["iters_mean"] = round(float(it.float().mean()), 2)
        one["iters_max"] = int(it.max())
        # the two sides answer the same question: the share of rows whose centres agree within 1e-4
        tc = torch_side()
        one["rows_agreeing_with_torch"] = round(float(((tc - c).abs().amax(dim=(1, 2)) < 1e-4).float().mean()), 4)
        res[f"D{D}"] = one
        del field, xs, ts, tc
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
