#!/usr/bin/env python3
"""PCA colouring of language images at the headline size (csrc/pca.hip): 1352 x 1014 pixels, C = 32,
[C, H, W] float32 on the device.

Everything is timed on the same card in one process, ROUNDS rounds after a warm-up, alternating, with
device events around REPS calls.  Each call takes the next of FRAMES distinct frames (8 x 175 MB,
past the 256 MiB Infinity Cache), so a sweep reads its frame from HBM:
  pca_image          the whole chain: sums, Gram, basis, project, colourise (float output)
  sums / gram / project    each sweep of the C ABI on its own, with its fold kernel
  basis              the Jacobi eigen-solve with the selection (one workgroup)
  colorize_f32 / colorize_u8
  transform_u8       LanguagePCA.transform(out="uint8"): the per-frame cost in sequence mode
  torch              the same five formulas as torch device ops in float32: mean, centred matmul,
                     torch.linalg.eigh, projection, min-max
  sklearn            gaussian_scene.pca_compress (host copy included), where scikit-learn is installed
Prints one JSON line (and writes it to --out): ms per call (median, min, max of the rounds), each
sweep's bytes over time as a fraction of the 8.0 TB/s HBM peak (and of the 6.29 TB/s a float4 copy
reaches), and the error of the native output and of the torch ops against the float64 restatement
(tests/pca_cases.py) on one whole frame."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4dlangsplat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pca_cases  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402
from language_query import LanguagePCA, pca_image  # noqa: E402

HBM_PEAK_TBS = 8.0          # MI355X_MICROARCH.md: HBM3E spec
HBM_COPY_TBS = 6.29         # the same table: what a float4 copy measures


def planted_frames(n, C, H, W, seed, dev):
    """n [C, H, W] frames of one planted spectrum (tests/pca_cases.py's, generated on the device)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(C, C)))
    std = 0.15 * np.array([1.0, 0.6, 0.36] + [0.16 * 0.8 ** i for i in range(C - 3)])
    mix = torch.from_numpy((q * std).astype(np.float32)).to(dev)                  # [C, C]: x = mean + mix z
    mean = torch.from_numpy((0.5 + 0.05 * rng.uniform(-1, 1, size=C)).astype(np.float32)).to(dev)
    return [(mix @ torch.randn(C, H * W, generator=g, device=dev) + mean[:, None]).reshape(C, H, W).contiguous()
            for _ in range(n)]


def torch_pca(x):
    """The five formulas as torch device ops in the frame's dtype: [C, H, W] -> [H, W, 3]."""
    C, H, W = x.shape
    p = x.reshape(C, -1)
    xc = p - p.mean(dim=1, keepdim=True)
    cov = xc @ xc.T / (p.shape[1] - 1)
    w, v = torch.linalg.eigh(cov)
    comps = v[:, -3:].flip(1).T
    big = comps.gather(1, comps.abs().argmax(dim=1, keepdim=True))
    comps = comps * torch.where(big < 0, -1.0, 1.0).to(comps.dtype)
    y = comps @ xc
    return ((y - y.min()) / (y.max() - y.min())).T.reshape(H, W, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1352)
    ap.add_argument("--height", type=int, default=1014)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pca.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    C, H, W = a.channels, a.height, a.width
    n = H * W
    frames = planted_frames(a.frames, C, H, W, 1, dev)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = torch.empty(lib.lsr_pca_workspace_bytes(C, n), dtype=torch.uint8, device=dev)
    sums = torch.empty(32, dtype=torch.float64, device=dev)
    gram = torch.empty(32 * 32, dtype=torch.float64, device=dev)
    y = torch.empty(n, 3, dtype=torch.float32, device=dev)
    rng = torch.empty(2, dtype=torch.float32, device=dev)
    img = torch.empty(n, 3, dtype=torch.float32, device=dev)
    img8 = torch.empty(n, 3, dtype=torch.uint8, device=dev)
    fitted = LanguagePCA().fit([frames[0]])
    mean, comps, ev = fitted.mean, fitted.components, fitted.explained_variance
    turn = [0]

    def frame():
        turn[0] += 1
        return frames[turn[0] % len(frames)]

    def check(rc, what):
        _lib.check(rc, what)

    calls = {
        "pca_image": lambda: pca_image(frame()),
        "sums": lambda: check(lib.lsr_pca_sums(C, n, frame().data_ptr(), 1, n, 1, sums.data_ptr(), ws.data_ptr(), stream),
                              "lsr_pca_sums"),
        "gram": lambda: check(lib.lsr_pca_gram(C, n, frame().data_ptr(), 1, n, sums.data_ptr(), n, 1, gram.data_ptr(),
                                               ws.data_ptr(), stream), "lsr_pca_gram"),
        "basis": lambda: check(lib.lsr_pca_basis(C, n, sums.data_ptr(), gram.data_ptr(), mean.data_ptr(), comps.data_ptr(),
                                                 ev.data_ptr(), stream), "lsr_pca_basis"),
        "project": lambda: check(lib.lsr_pca_project(C, n, frame().data_ptr(), 1, n, mean.data_ptr(), comps.data_ptr(), 1,
                                                     y.data_ptr(), rng.data_ptr(), ws.data_ptr(), stream),
                                 "lsr_pca_project"),
        "colorize_f32": lambda: check(lib.lsr_pca_colorize_f32(n, y.data_ptr(), rng.data_ptr(), img.data_ptr(), stream),
                                      "lsr_pca_colorize_f32"),
        "colorize_u8": lambda: check(lib.lsr_pca_colorize_u8(n, y.data_ptr(), rng.data_ptr(), img8.data_ptr(), stream),
                                     "lsr_pca_colorize_u8"),
        "transform_u8": lambda: fitted.transform(frame(), out="uint8"),
        "torch": lambda: torch_pca(frame()),
    }
    reps = {k: a.reps for k in calls}
    try:
        import sklearn  # noqa: F401
        import gaussian_scene
        calls["sklearn"] = lambda: gaussian_scene.pca_compress(frame())
        reps["sklearn"] = 1
    except ImportError:
        pass
    # (the warm-up below runs sums and gram before basis, so the solve times a real frame's moments)
    frame_bytes = 4 * C * n
    moved = {"sums": frame_bytes, "gram": frame_bytes, "project": frame_bytes + 12 * n, "colorize_f32": 24 * n,
             "colorize_u8": 15 * n, "pca_image": 3 * frame_bytes + 36 * n, "transform_u8": frame_bytes + 27 * n}
    times = {k: [] for k in calls}
    for k, fn in calls.items():                               # warm-up of every shape
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

    # the native chain against the float64 restatement (whole frame, on the host)
    x0 = frames[0]
    ref = pca_cases.pca_reference(x0.reshape(C, -1).T.cpu().numpy())
    err = float(np.abs(pca_image(x0).reshape(-1, 3).cpu().numpy().astype(np.float64) - ref["out"]).max())
    err_torch = float(np.abs(torch_pca(x0).reshape(-1, 3).cpu().numpy().astype(np.float64) - ref["out"]).max())

    res = {"workload": {"width": W, "height": H, "channels": C, "layout": "chw", "frames": a.frames, "rounds": a.rounds,
                        "reps": a.reps, "frame_bytes": frame_bytes},
           "device": torch.cuda.get_device_name(0)}
    for k in calls:
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4)}
        if k in moved:
            tbs = moved[k] / (med * 1e-3) / 1e12
            res[k].update({"bytes": moved[k], "tb_per_s": round(tbs, 3), "fraction_of_hbm_peak": round(tbs / HBM_PEAK_TBS, 3),
                           "fraction_of_copy_rate": round(tbs / HBM_COPY_TBS, 3)})
    res["floor_ms_three_reads_at_copy_rate"] = round(3 * frame_bytes / (HBM_COPY_TBS * 1e12) * 1e3, 4)
    res["speedup_vs_torch"] = round(res["torch"]["ms_median"] / res["pca_image"]["ms_median"], 2)
    if "sklearn" in res:
        res["speedup_vs_sklearn"] = round(res["sklearn"]["ms_median"] / res["pca_image"]["ms_median"], 1)
    res["max_abs_error_vs_float64"] = {"pca_image": err, "torch_float32": err_torch}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
