#!/usr/bin/env python3
"""Time-sensitive query at the headline image size (csrc/video_query.hip): one 1352 x 1014 x 6 video latent,
the full-width decoder 6 -> 32 -> 64 -> 128 -> 256 -> 512 -> 1024 -> 2048 -> 4096, one mask covering a
stated share of the frame (default 2 %, 5 % and 20 %), one phrase.

Two paths on the same card in one process, alternating, ROUNDS rounds each after a warm-up, timed with
device events around one masked_similarity-sized piece of work:
  native   masked_similarity() on the native path (gather, the layer kernels in chunks of --chunk-rows rows,
           the finish and the segment mean)
  torch    the same formulas as torch ops on CUDA float32 (the fallback's expression: nn.functional.linear
           per layer on all rows of the mask at once, the product with the query, the norm, the mean)
Prints one JSON line (and writes it to --out): per share the rows, ms of each path (median, min, max), the
native path's TFLOP/s and share of the f32 matrix peak with FLOPs = 2 * sum(in * out) per row, each path's
peak memory above what was allocated before it, and both paths' error against float64 on a row sample."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4dlangsplat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import video_query_cases as vc  # noqa: E402
import video_query as vq  # noqa: E402
from language_query import LanguageDecoder  # noqa: E402

F32_MATRIX_PEAK_TFLOPS = 157.3    # v_mfma_f32_* (f32 in / f32 accumulate) on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1352)
    ap.add_argument("--height", type=int, default=1014)
    ap.add_argument("--shares", type=float, nargs="+", default=[0.02, 0.05, 0.20])
    ap.add_argument("--chunk-rows", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_video_query.py measures on the GPU; none found")
    dev = "cuda"
    dims = vc.FULL_DIMS
    ws, bs = vc.decoder_arrays(dims, 1)
    dec = LanguageDecoder.from_state_dict(vc.state_dict(ws, bs, torch)).to(dev)
    assert vq.native_ok(dec)
    H, W = a.height, a.width
    lat = torch.from_numpy(vc.latents((H, W, dims[0]), 2)).to(dev)
    q = torch.from_numpy(vc.queries(ws, bs, lat[0, :64].cpu().numpy(), 1, 3)).to(dev)
    qn = (q.double() / q.double().norm(dim=-1, keepdim=True)).float()
    flop_row = 2.0 * sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))

    res = {"workload": {"width": W, "height": H, "decoder": dims, "chunk_rows": a.chunk_rows, "rounds": a.rounds,
                        "mflop_per_row": round(flop_row / 1e6, 2)},
           "device": torch.cuda.get_device_name(0), "shares": []}
    for share in a.shares:
        rows_of_mask = max(1, int(round(share * H)))            # the top `share` of the frame's rows
        mask = torch.zeros(1, H, W, dtype=torch.uint8, device=dev)
        mask[0, :rows_of_mask] = 1
        n = rows_of_mask * W

        def native():
            return vq.masked_similarity(lat, mask, dec, q, chunk_rows=a.chunk_rows)[0]

        def torch_path():
            return vq._cosine_torch(lat[mask[0] == 1], dec, qn)[0].double().mean().float()

        paths = {"native": native, "torch": torch_path}
        times = {k: [] for k in paths}
        peaks, value = {}, {}
        for k, fn in paths.items():                            # warm-up, and each path's peak memory
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            value[k] = float(fn())
            torch.cuda.synchronize()
            peaks[k] = torch.cuda.max_memory_allocated() - before
        for _ in range(a.rounds):
            for k, fn in paths.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize()
                times[k].append(t0.elapsed_time(t1))
        # both paths against float64 on a sample of the mask's rows
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(4))[:512].to(dev)
        sample = lat[:rows_of_mask].reshape(n, dims[0])[idx].contiguous()
        ref = vq._cosine_torch(sample.double(), dec, qn.double())
        entry = {"share": share, "rows": n, "gflop": round(flop_row * n / 1e9, 1),
                 "similarity": value, "max_abs_error_vs_float64": {
                     "native": float((vq.row_cosines(sample, dec, q).double() - ref).abs().max()),
                     "torch": float((vq._cosine_torch(sample, dec, qn).double() - ref).abs().max())}}
        for k in paths:
            entry[k] = {"ms_median": round(statistics.median(times[k]), 3), "ms_min": round(min(times[k]), 3),
                        "ms_max": round(max(times[k]), 3), "peak_memory_bytes": int(peaks[k])}
            entry[k]["tflops"] = round(flop_row * n / (entry[k]["ms_median"] * 1e-3) / 1e12, 1)
        entry["native"]["fraction_of_f32_matrix_peak"] = round(entry["native"]["tflops"] / F32_MATRIX_PEAK_TFLOPS, 3)
        entry["torch_over_native"] = round(entry["torch"]["ms_median"] / entry["native"]["ms_median"], 2)
        res["shares"].append(entry)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
