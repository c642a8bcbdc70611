#!/usr/bin/env python3
"""Writes tests/golden/autoencoder_golden.npz and autoencoder_state_dict_layout.json from the reference
implementation's own code, on the CPU:

    python tests/golden/make_autoencoder_golden.py --reference /path/to/4DLangSplat

It needs the reference checkout, so it runs where the fixture is made, not in the test suite.

What runs is the reference's own code, unchanged: autoencoder/model.py's Autoencoder, autoencoder/train.py's
l2_loss and cos_loss, and torch.optim.Adam(model.parameters(), lr) in the order of train.py:114-129
(encode, decode, the two losses, zero_grad, backward, step).  train.py is imported with wandb and
torch.utils.tensorboard (with a SummaryWriter attribute) registered as stub modules; its training loop sits
under `if __name__ == '__main__':` and does not run.

Inputs: tests/autoencoder_cases.py, shared with the tests.  Everything runs in float64 (the stored results)
and again in float32: the float32 run's max abs error against float64 is stored beside each result as
<name>.f32_err, and the GPU tests bound the native error by a multiple of it.

Stored: the seed and checksums of the regenerated inputs;
  s1.*    after step 1: losses [2] (l2, cos), param.<key>, exp_avg.<key>, exp_avg_sq.<key>, buffer.<key>
  s8.*    after 8 steps: losses [8, 2], param.<key>
  eval.*  a fixed state dict with non-trivial running statistics on 200 rows: latents, losses [2]
The archive is written with fixed time stamps, so it regenerates byte for byte.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import autoencoder_cases as ac  # noqa: E402


def import_reference(root):
    sys.modules.setdefault("wandb", types.ModuleType("wandb"))
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    sys.path.insert(0, os.path.join(root, "autoencoder"))
    import model
    import train
    torch.autograd.set_detect_anomaly(False)                   # train.py switches it on at import
    return model.Autoencoder, train


def build(Autoencoder, sd, feature, enc, dec, dtype):
    with contextlib.redirect_stdout(io.StringIO()):            # the constructor prints its layers
        model = Autoencoder(list(enc), list(dec), feature_dim=feature)
    model.load_state_dict(ac.torch_state_dict(sd, torch))
    return model.to(dtype)


def train_run(Autoencoder, train, inp, dtype):
    model = build(Autoencoder, inp["train_sd"], ac.FEATURE, ac.ENC, ac.DEC, dtype)
    opt = torch.optim.Adam(model.parameters(), lr=ac.LR)
    names = {p: k for k, p in model.named_parameters()}
    out, losses = {}, []
    model.train()
    for s in range(ac.STEPS):
        data = torch.from_numpy(inp["batches"][s]).to(dtype)
        outputs = model.decode(model.encode(data))
        l2, cos = train.l2_loss(outputs, data), train.cos_loss(outputs, data)
        loss = l2 + cos * ac.COS_WEIGHT
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append([l2.item(), cos.item()])
        if s == 0:
            out["s1.losses"] = np.array(losses[0])
            for p, k in names.items():
                out[f"s1.param.{k}"] = p.detach().numpy().copy()
                out[f"s1.exp_avg.{k}"] = opt.state[p]["exp_avg"].numpy().copy()
                out[f"s1.exp_avg_sq.{k}"] = opt.state[p]["exp_avg_sq"].numpy().copy()
            for k, b in model.named_buffers():
                out[f"s1.buffer.{k}"] = b.numpy().copy()
    out["s8.losses"] = np.array(losses)
    for p, k in names.items():
        out[f"s8.param.{k}"] = p.detach().numpy().copy()
    return out


def eval_run(Autoencoder, train, inp, dtype):
    model = build(Autoencoder, inp["eval_sd"], ac.FEATURE, ac.ENC, ac.DEC, dtype).eval()
    data = torch.from_numpy(inp["eval_rows"]).to(dtype)
    with torch.no_grad():
        outputs = model(data)
        return {"eval.latents": model.encode(data).numpy(),
                "eval.losses": np.array([float(train.l2_loss(outputs, data)), float(train.cos_loss(outputs, data))])}


def layout(Autoencoder, feature, enc, dec):
    with contextlib.redirect_stdout(io.StringIO()):
        sd = Autoencoder(list(enc), list(dec), feature_dim=feature).state_dict()
    return {k: {"shape": list(v.shape), "dtype": str(v.dtype)} for k, v in sd.items()}


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps and a fixed member order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds autoencoder/train.py)")
    ap.add_argument("--out", default=os.path.join(HERE, "autoencoder_golden.npz"))
    ap.add_argument("--layout", default=os.path.join(HERE, "autoencoder_state_dict_layout.json"))
    a = ap.parse_args()
    Autoencoder, train = import_reference(os.path.abspath(a.reference))
    torch.set_num_threads(1)                                   # one summation order, whatever the machine
    inp = ac.fixture_inputs()
    r64 = {**train_run(Autoencoder, train, inp, torch.float64), **eval_run(Autoencoder, train, inp, torch.float64)}
    r32 = {**train_run(Autoencoder, train, inp, torch.float32), **eval_run(Autoencoder, train, inp, torch.float32)}
    store = {"seed": np.int64(ac.FIXTURE_SEED),
             "train_sd_sha256": np.array(ac.checksum(list(inp["train_sd"].values()))),
             "eval_sd_sha256": np.array(ac.checksum(list(inp["eval_sd"].values()))),
             "rows_sha256": np.array(ac.checksum([inp["batches"], inp["eval_rows"]]))}
    for k, v in r64.items():
        store[k] = v
        if v.dtype == np.int64:
            assert np.array_equal(v, r32[k])
            continue
        assert v.dtype == np.float64 and (r32[k].dtype == np.float32 or k.endswith("losses")), (k, v.dtype, r32[k].dtype)
        store[k + ".f32_err"] = np.float64(np.abs(r32[k].astype(np.float64) - v).max())
    write_npz(a.out, store)
    with open(a.layout, "w") as f:
        json.dump({"fixture": layout(Autoencoder, ac.FEATURE, ac.ENC, ac.DEC), "clip": layout(Autoencoder, *ac.CLIP)},
                  f, indent=1, sort_keys=False)
        f.write("\n")
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")
    pre = set(ac.pre_bn_bias_keys(len(ac.ENC)))
    for k in sorted(store):
        if k.endswith(".f32_err"):
            name = k[:-8]
            tag = "  (a bias in front of a BatchNorm)" if name.split(".", 2)[-1] in pre else ""
            print(f"  {name}: max |value| {np.abs(store[name]).max():.3g}, float32 reference error {float(store[k]):.3g}{tag}")


if __name__ == "__main__":
    main()
