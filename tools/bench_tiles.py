#!/usr/bin/env python3
"""Language-feature tiles at the headline size (csrc/tiles.hip): one 1352 x 1014 frame, four synthetic
Voronoi-style label maps of about 64 / 128 / 32 / 16 labels (levels default, s, m, l), int32 labels and
a uint8 image on the device.

Everything is timed on the same card in one process, ROUNDS rounds after a warm-up, alternating, with
device events around REPS calls:
  prepare_frame      the whole native frame: census, plan, the host read of the counts, render
                     (allocations included)
  census / plan / render   each step of the C ABI on its own (render split further: the segment maps
                     alone, n = 0 tiles, is `remap`)
  torch              language_tiles._prepare_torch: the same formulas as torch device ops
Prints one JSON line (and writes it to --out): ms per call (median, min, max of the rounds), the tile
count, the census' and the render's bytes over their times, and whether native and fallback agree
(segment maps, boxes and tile bytes, for equality)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4dlangsplat_amd"))

import torch  # noqa: E402

import language_tiles as lt  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402


def voronoi_labels(H, W, counts, seed, dev):
    """[4, H, W] int32: level j is the nearest of counts[j] seeded sites, labelled 1 .. counts[j]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    yy = torch.arange(H, device=dev)[:, None, None]
    xx = torch.arange(W, device=dev)[None, :, None]
    out = torch.empty((len(counts), H, W), dtype=torch.int32, device=dev)
    for j, k in enumerate(counts):
        sy = torch.randint(0, H, (k,), generator=g).to(dev)
        sx = torch.randint(0, W, (k,), generator=g).to(dev)
        for y0 in range(0, H, 64):
            d = (yy[y0:y0 + 64] - sy) ** 2 + (xx - sx) ** 2
            out[j, y0:y0 + 64] = (d.argmin(dim=-1) + 1).to(torch.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1352)
    ap.add_argument("--height", type=int, default=1014)
    ap.add_argument("--labels", type=int, nargs=4, default=[64, 128, 32, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiles.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    H, W, L = a.height, a.width, 4
    labels = voronoi_labels(H, W, a.labels, 1, dev)
    image = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    nbytes = lib.lsr_tiles_workspace_size(L)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    desc = torch.empty((_lib.TILES_MAX_TILES, _lib.TILES_DESC_INTS), dtype=torch.int32, device=dev)
    counts = torch.zeros(_lib.TILES_COUNTS, dtype=torch.int32, pin_memory=True)
    ref = lt.prepare_frame(image, labels)
    n = sum(ref.lengths)
    lengths = (ctypes.c_int32 * L)(*ref.lengths)
    none = (ctypes.c_int32 * L)(0, 0, 0, 0)
    seg, tiles = torch.empty_like(ref.seg_maps), torch.empty_like(ref.tiles)
    check = _lib.check

    calls = {
        "prepare_frame": lambda: lt.prepare_frame(image, labels),
        "census": lambda: check(lib.lsr_tiles_census(L, H, W, labels.data_ptr(), nbytes, ws.data_ptr(), stream),
                                "lsr_tiles_census"),
        "plan": lambda: check(lib.lsr_tiles_plan(L, H, W, nbytes, ws.data_ptr(), desc.data_ptr(), counts.data_ptr(),
                                                 stream), "lsr_tiles_plan"),
        "render": lambda: check(lib.lsr_tiles_render(L, H, W, labels.data_ptr(), image.data_ptr(), nbytes, ws.data_ptr(),
                                                     desc.data_ptr(), lengths, n, seg.data_ptr(), tiles.data_ptr(),
                                                     stream), "lsr_tiles_render"),
        "remap": lambda: check(lib.lsr_tiles_render(L, H, W, labels.data_ptr(), image.data_ptr(), nbytes, ws.data_ptr(),
                                                    desc.data_ptr(), none, 0, seg.data_ptr(), None, stream),
                               "lsr_tiles_render"),
        "torch": lambda: lt._prepare_torch(image, labels.long()),
    }
    reps = {k: a.reps for k in calls}
    reps["torch"] = 1
    times = {k: [] for k in calls}
    for fn in calls.values():                                  # warm-up, in the steps' order
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _i in range(reps[k]):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) / reps[k])

    fb = lt._prepare_torch(image, labels.long())
    as_bytes = lambda t: torch.round(t * 255.0).to(torch.uint8)          # (torch's / 255 is a product with 1 / 255)
    same = bool(fb.lengths == ref.lengths and torch.equal(fb.seg_maps, ref.seg_maps) and torch.equal(fb.boxes, ref.boxes)
                and torch.equal(as_bytes(fb.tiles), as_bytes(ref.tiles)) and torch.equal(seg, ref.seg_maps)
                and torch.equal(tiles, ref.tiles))
    res = {"workload": {"width": W, "height": H, "labels_per_level": a.labels, "tiles_per_level": ref.lengths,
                        "tiles": n, "rounds": a.rounds, "reps": a.reps},
           "device": torch.cuda.get_device_name(0)}
    for k in calls:
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4)}
    out_bytes = tiles.numel() * 4 + seg.numel() * 4
    res["render"]["output_bytes"] = out_bytes
    res["render"]["output_tb_per_s"] = round(out_bytes / (res["render"]["ms_median"] * 1e-3) / 1e12, 3)
    res["census"]["label_bytes"] = labels.numel() * 4
    res["census"]["tb_per_s"] = round(labels.numel() * 4 / (res["census"]["ms_median"] * 1e-3) / 1e12, 3)
    res["speedup_vs_torch"] = round(res["torch"]["ms_median"] / res["prepare_frame"]["ms_median"], 1)
    res["native_equals_fallback"] = same
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
