#!/usr/bin/env python3
"""Open-vocabulary query at the headline image size (csrc/query.hip): 1352 x 1014 pixels, 3 levels,
the default decoder 3 -> 16 -> 32 -> 64 -> 128 -> 256 -> 512, 8 positives and 4 negatives.

Three paths on the same card in one process, alternating, ROUNDS rounds each after a warm-up, timed
with device events around the work of all levels:
  fused_relevancy   relevancy() on the native path: [L, H, W, 3] -> [L, 8, H, W]
  fused_decode      LanguageDecoder.decode() on the native path: [L, H, W, 3] -> [L, H, W, 512]
                    (one level at a time: the features of three levels are 8.4 GB)
  torch             the reference's expression as torch ops (the fallback) on CUDA float32
Prints one JSON line (and writes it to --out): ms per level of each path (median, min, max of the
rounds), the fused relevancy's share of the f32 matrix peak, each path's peak memory above what was
allocated before it, and the fused paths' error against the torch path in float64 on a pixel sample."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4dlangsplat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import query_cases as qc  # noqa: E402
from language_query import LanguageDecoder, _relevancy_torch, relevancy  # noqa: E402

F32_MATRIX_PEAK_TFLOPS = 157.3    # MI355X_MICROARCH.md: v_mfma_f32_* (f32 in / f32 accumulate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1352)
    ap.add_argument("--height", type=int, default=1014)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--positives", type=int, default=8)
    ap.add_argument("--negatives", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_query.py measures on the GPU; none found")
    dev = "cuda"
    dims = qc.FIXTURE_DIMS
    ws, bs = qc.decoder_arrays(dims, 1)
    dec = LanguageDecoder.from_state_dict(qc.state_dict(ws, bs, torch)).to(dev)
    L, H, W = a.levels, a.height, a.width
    lat = torch.from_numpy(qc.latents((L, H, W, dims[0]), 2)).to(dev)
    e = torch.from_numpy(qc.phrase_embeddings(ws, bs, lat[0, :64].reshape(-1, dims[0]).cpu().numpy(),
                                              a.positives + a.negatives, 3)).to(dev)
    pos, neg = e[:a.positives], e[a.positives:]
    n_pix = H * W
    macs = sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1)) + dims[-1] * (a.positives + a.negatives)
    flop_level = 2.0 * macs * n_pix

    def fused_relevancy():
        return relevancy(lat, dec, pos, neg)

    def fused_decode():
        for l in range(L):
            dec.decode(lat[l])

    def torch_path():
        for l in range(L):
            _relevancy_torch(lat[l].reshape(n_pix, dims[0]), dec, pos, neg, 10.0)

    paths = {"fused_relevancy": fused_relevancy, "fused_decode": fused_decode, "torch": torch_path}
    assert dec.native_ok()
    times = {k: [] for k in paths}
    peaks = {}
    for k, fn in paths.items():                              # warm-up, and each path's peak memory
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peaks[k] = torch.cuda.max_memory_allocated() - before
    for _ in range(a.rounds):
        for k, fn in paths.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) / L)

    # the paths agree (a pixel sample in float64)
    idx = torch.randperm(n_pix, generator=torch.Generator().manual_seed(4))[:4096].to(dev)
    sample = lat[0].reshape(n_pix, dims[0])[idx]
    d64 = dec.to(torch.float64)
    ref = _relevancy_torch(sample.double(), d64, pos.double(), neg.double(), 10.0)
    rel_err = float((fused_relevancy()[0].reshape(a.positives, n_pix)[:, idx].double() - ref).abs().max())
    feat_err = float((dec.decode(sample).double() - d64.decode(sample.double())).abs().max())

    res = {"workload": {"width": W, "height": H, "levels": L, "decoder": dims, "positives": a.positives,
                        "negatives": a.negatives, "rounds": a.rounds, "gflop_per_level": round(flop_level / 1e9, 1)},
           "device": torch.cuda.get_device_name(0)}
    for k in paths:
        res[k] = {"ms_per_level_median": round(statistics.median(times[k]), 3), "ms_per_level_min": round(min(times[k]), 3),
                  "ms_per_level_max": round(max(times[k]), 3), "peak_memory_bytes": int(peaks[k])}
    med = res["fused_relevancy"]["ms_per_level_median"]
    res["fused_relevancy"]["tflops"] = round(flop_level / (med * 1e-3) / 1e12, 1)
    res["fused_relevancy"]["fraction_of_f32_matrix_peak"] = round(flop_level / (med * 1e-3) / 1e12 / F32_MATRIX_PEAK_TFLOPS, 3)
    res["fused_relevancy"]["floor_ms_per_level"] = round(flop_level / (F32_MATRIX_PEAK_TFLOPS * 1e12) * 1e3, 2)
    res["fused_relevancy"]["output_bytes"] = L * a.positives * n_pix * 4
    res["weights_bytes"] = int(sum(w.numel() + b.numel() for w, b in zip(dec.weights, dec.biases)) * 4)
    res["speedup_vs_torch"] = round(res["torch"]["ms_per_level_median"] / med, 2)
    res["max_abs_error_vs_float64"] = {"relevancy": rel_err, "features": feat_err}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
