#!/usr/bin/env python3
"""The language autoencoder (csrc/autoencoder.hip) against the same formulas as torch ops, on one card in one
process, the paths alternating, ROUNDS rounds each after a warm-up.

(a) Training at batch 64 at the CLIP shape (512 -> 256 -> ... -> 3 -> 16 -> ... -> 512) and the video shape
    (4096 -> ... -> 6 -> ... -> 4096):
      native       AutoencoderTrainer.step
      torch        nn.Linear / nn.BatchNorm1d / nn.ReLU modules, the two losses and torch.optim.Adam, float32
      torch_fused  the same with Adam(fused=True)
    Per path: wall-clock per step over --steps back-to-back steps with one synchronisation at the end (the number
    that matters for a launch-bound loop), the device-event time of the same window, and kernel launches per step
    (the native plan's count, 3 (n_enc + n_dec) + 1; torch's counted by torch.profiler where it reports kernels).
    Bytes per step are what the algorithm needs: every weight read by the forward and by the input-gradient
    product, and Adam's read and write of parameter, m and v (32 bytes per parameter), against the HBM peak.
(b) encode and reconstruction_loss over 200 k x 512 and 20 k x 4096 rows: ms, and GB/s of input read.
Both paths' error against float64 is reported: for (a) after one step from the same state (the losses, and the
largest error of exp_avg over the tensors, each relative to its tensor's largest magnitude, without the biases in
front of a BatchNorm), for (b) on a sample of rows.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4dlangsplat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import autoencoder_cases as ac  # noqa: E402
from language_autoencoder import AutoencoderTrainer, LanguageAutoencoder  # noqa: E402

HBM_PEAK_TBS = 8.0                # MI355X HBM3E, specification


def unit(t):
    return t / t.norm(dim=-1, keepdim=True)


def torch_modules(ae):
    """nn layers holding a copy of a LanguageAutoencoder's tensors, built from its keys: (encoder, decoder) as
    nn.Sequential, whose layer numbers are the keys' (a ReLU wherever the keys leave a number out)."""
    halves = []
    for half in ("encoder", "decoder"):
        at = {}
        for k, v in ae.sd.items():
            name, idx, field = k.split(".")
            if name == half and field == "weight":
                at[int(idx)] = nn.Linear(v.shape[1], v.shape[0]) if v.dim() == 2 else nn.BatchNorm1d(v.shape[0])
        seq = nn.Sequential(*[at.get(i, nn.ReLU()) for i in range(max(at) + 1)])
        seq.load_state_dict({k[len(half) + 1:]: v for k, v in ae.sd.items() if k.startswith(half + ".")})
        halves.append(seq.to(ae.device).train())
    return halves


def torch_stepper(ae, fused, lr, cos_weight):
    encoder, decoder = torch_modules(ae)
    opt = torch.optim.Adam(list(encoder.parameters()) + list(decoder.parameters()), lr=lr, fused=fused)

    def step(x):
        out = unit(decoder(unit(encoder(x))))
        loss = ((out - x) ** 2).mean() + (1 - F.cosine_similarity(out, x, dim=1).mean()) * cos_weight
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def launches_per_step(step, x, n=3):
    """Kernel launches of one step, by torch.profiler; None where it reports no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                step(x)
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        return round(len(kernels) / n, 1) if kernels else None
    except Exception:                                          # a profiler that cannot trace this device
        return None


def timed_window(step, x, steps):
    """(wall ms per step, device-event ms per step) of `steps` back-to-back steps, one synchronisation at the end."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    t0.record()
    for _ in range(steps):
        step(x)
    t1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - w0) * 1e3 / steps, t0.elapsed_time(t1) / steps


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def train_errors(sd, shape, x, lr, cos_weight):
    """After one step from the same state: each path against the torch formulas in float64 on the device."""
    tr64, l64 = None, None
    out = {}
    for name, dtype, native in (("float64", torch.float64, False), ("native", torch.float32, True),
                                ("torch", torch.float32, False)):
        ae = LanguageAutoencoder(ac.torch_state_dict(sd, torch, dtype)).to("cuda")
        tr = AutoencoderTrainer(ae, lr=lr, cos_weight=cos_weight)
        tr.t = 1
        l = tr._step_native(x) if native else tr._step_torch(x.to(dtype))
        l = torch.stack([t.double() for t in l])
        if name == "float64":
            tr64, l64 = tr, l
            continue
        pre = set(ae.pre_bn_bias_keys())
        rel = max(float((tr.exp_avg[k].double() - tr64.exp_avg[k]).abs().max() / tr64.exp_avg[k].abs().max())
                  for k in tr.exp_avg if k not in pre)
        out[name] = {"losses_max_abs_error": float((l - l64).abs().max()), "exp_avg_max_error_over_tensor_max": rel}
    return out


def bench_training(name, shape, a):
    feature, enc, dec = shape
    sd = ac.state_dict_np(feature, enc, dec, 1)
    x = torch.from_numpy(ac.unit_rows(a.batch, feature, 2)).cuda()
    ae = LanguageAutoencoder(ac.torch_state_dict(sd, torch)).to("cuda")
    assert ae.native_ok()
    trainer = AutoencoderTrainer(ae, lr=a.lr, cos_weight=a.cos_weight)
    paths = {"native": trainer.step,
             "torch": torch_stepper(ae, False, a.lr, a.cos_weight),
             "torch_fused": torch_stepper(ae, True, a.lr, a.cos_weight)}
    for step in paths.values():                                # warm-up
        for _ in range(a.warmup):
            step(x)
    torch.cuda.synchronize()
    wall, dev = {k: [] for k in paths}, {k: [] for k in paths}
    for _ in range(a.rounds):
        for k, step in paths.items():
            w, d = timed_window(step, x, a.steps)
            wall[k].append(w)
            dev[k].append(d)
    n_params = sum(v.size for k, v in sd.items() if k.endswith((".weight", ".bias")))
    n_weights = sum(v.size for k, v in sd.items() if k.endswith(".weight") and v.ndim == 2)
    bytes_step = 4 * (2 * n_weights + 6 * n_params)
    flop_step = 6.0 * a.batch * n_weights
    entry = {"shape": {"feature_dim": feature, "encoder": enc, "decoder": dec}, "batch": a.batch, "parameters": n_params,
             "gflop_per_step": round(flop_step / 1e9, 3), "mbytes_per_step": round(bytes_step / 1e6, 2),
             "native_plan_launches_per_step": 3 * (len(enc) + len(dec)) + 1}
    for k, step in paths.items():
        entry[k] = {"wall_ms_per_step": stats(wall[k]), "device_ms_per_step": stats(dev[k]),
                    "launches_per_step_profiled": launches_per_step(step, x)}
        sec = entry[k]["device_ms_per_step"]["median"] * 1e-3
        entry[k]["gbytes_per_s"] = round(bytes_step / sec / 1e9, 1)
        entry[k]["fraction_of_hbm_peak"] = round(bytes_step / sec / (HBM_PEAK_TBS * 1e12), 4)
    for k in ("torch", "torch_fused"):
        entry[k + "_over_native_wall"] = round(entry[k]["wall_ms_per_step"]["median"] / entry["native"]["wall_ms_per_step"]["median"], 2)
    entry["error_vs_float64"] = train_errors(sd, shape, x, a.lr, a.cos_weight)
    return entry


def bench_eval(name, shape, n_rows, a):
    feature, enc, dec = shape
    sd = ac.state_dict_np(feature, enc, dec, 3, running=True)
    ae = LanguageAutoencoder(ac.torch_state_dict(sd, torch)).to("cuda")
    x = torch.from_numpy(ac.unit_rows(n_rows, feature, 4)).cuda()
    paths = {"encode": {"native": lambda: ae.encode(x), "torch": lambda: ae._encode_torch(x)},
             "reconstruction_loss": {"native": lambda: ae.reconstruction_loss(x), "torch": lambda: ae._loss_sums_torch(x)}}
    entry = {"shape": {"feature_dim": feature, "encoder": enc, "decoder": dec}, "rows": n_rows,
             "input_mbytes": round(x.numel() * 4 / 1e6, 1)}
    for what, two in paths.items():
        times = {k: [] for k in two}
        for fn in two.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in two.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize()
                times[k].append(t0.elapsed_time(t1))
        entry[what] = {k: {"ms": stats(v), "input_gbytes_per_s": round(x.numel() * 4 / (statistics.median(v) * 1e-3) / 1e9, 1)}
                       for k, v in times.items()}
        entry[what]["torch_over_native"] = round(entry[what]["torch"]["ms"]["median"] / entry[what]["native"]["ms"]["median"], 2)
    sample = x[:2048]
    a64 = ae.to(dtype=torch.float64)
    z64 = a64.encode(sample.double())
    s64 = torch.stack(a64._loss_sums_torch(sample.double()))
    entry["error_vs_float64_on_2048_rows"] = {
        "encode": {"native": float((ae.encode(sample).double() - z64).abs().max()),
                   "torch": float((ae._encode_torch(sample).double() - z64).abs().max())},
        "loss_sums_relative": {
            "native": float(((torch.stack(_sums(ae, sample)) - s64) / s64).abs().max()),
            "torch": float(((torch.stack(ae._loss_sums_torch(sample)) - s64) / s64).abs().max())}}
    return entry


def _sums(ae, x):
    l2, cos = ae.reconstruction_loss(x)
    return l2 * (x.shape[0] * ae.feature_dim), (1 - cos) * x.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--cos-weight", type=float, default=1e-3)
    ap.add_argument("--clip-rows", type=int, default=200_000)
    ap.add_argument("--video-rows", type=int, default=20_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_autoencoder.py measures on the GPU; none found")
    res = {"device": torch.cuda.get_device_name(0),
           "workload": {"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds},
           "training": {"clip": bench_training("clip", ac.CLIP, a), "video": bench_training("video", ac.VIDEO, a)},
           "eval": {"clip": bench_eval("clip", ac.CLIP, a.clip_rows, a), "video": bench_eval("video", ac.VIDEO, a.video_rows, a)}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
