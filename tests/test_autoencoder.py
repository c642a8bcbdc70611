"""CPU checks of the language autoencoder (language_autoencoder.py): its torch formulas in float64 against
the reference's recorded results (tests/golden/autoencoder_golden.npz, made by make_autoencoder_golden.py
from the reference's own Autoencoder, l2_loss, cos_loss and torch.optim.Adam), the state-dict layout, the
training loop's rules, the compression pass and the C ABI's refusals.

Float64 against float64: the two sides order their sums differently, so a tensor may differ by float64's
rounding (2.2e-16) times the conditioning of a training step; 1e-9 of the tensor's largest magnitude allows a
conditioning of several million and is still a thousandth of the float32 reference's own error.  The biases in
front of a BatchNorm are not compared per element (autoencoder_cases.PRE_BN_RULE)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import autoencoder_cases as ac
from diff_gaussian_rasterization import _lib
from language_autoencoder import (AutoencoderTrainer, LanguageAutoencoder, compress_feature_dir, fit,
                                  load_feature_dir)
from language_query import LanguageDecoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REL = 1e-9


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "autoencoder_golden.npz")))


@pytest.fixture(scope="module")
def inputs():
    return ac.fixture_inputs()


def ae_of(sd, dtype=torch.float64):
    return LanguageAutoencoder(ac.torch_state_dict(sd, torch, dtype))


def close(a, ref, what):
    a, ref = a.detach().cpu().double().numpy(), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    e, bound = np.abs(a - ref).max(), REL * max(np.abs(ref).max(), 1e-300)
    assert e <= bound, f"{what}: error {e:.3g} > {bound:.3g}"


def test_fixture_inputs_are_the_generators(gold, inputs):
    assert int(gold["seed"]) == ac.FIXTURE_SEED
    assert str(gold["train_sd_sha256"]) == ac.checksum(list(inputs["train_sd"].values()))
    assert str(gold["eval_sd_sha256"]) == ac.checksum(list(inputs["eval_sd"].values()))
    assert str(gold["rows_sha256"]) == ac.checksum([inputs["batches"], inputs["eval_rows"]])


def test_training_steps_match_the_reference_in_float64(gold, inputs):
    ae = ae_of(inputs["train_sd"])
    tr = AutoencoderTrainer(ae, lr=ac.LR, cos_weight=ac.COS_WEIGHT)
    pre = set(ae.pre_bn_bias_keys())
    assert pre == set(ac.pre_bn_bias_keys(len(ac.ENC)))
    start = {k: v.clone() for k, v in ae.sd.items()}
    losses = []
    for s in range(ac.STEPS):
        l2, cos = tr.step(torch.from_numpy(inputs["batches"][s]).double())
        losses.append([float(l2), float(cos)])
        if s == 0:
            close(torch.tensor(losses[0], dtype=torch.float64), gold["s1.losses"], "losses of step 1")
            for k in ae.parameter_keys():
                if k in pre:
                    for t in (ae.sd[k], tr.exp_avg[k], tr.exp_avg_sq[k]):
                        assert bool(torch.isfinite(t).all())
                    assert float((ae.sd[k] - start[k]).abs().max()) <= ac.adam_step_bound(ac.LR)
                    continue
                close(ae.sd[k], gold[f"s1.param.{k}"], f"step 1 {k}")
                close(tr.exp_avg[k], gold[f"s1.exp_avg.{k}"], f"step 1 exp_avg {k}")
                close(tr.exp_avg_sq[k], gold[f"s1.exp_avg_sq.{k}"], f"step 1 exp_avg_sq {k}")
            for k in ae.sd:
                if k.endswith(("running_mean", "running_var")):
                    close(ae.sd[k], gold[f"s1.buffer.{k}"], f"step 1 {k}")
                if k.endswith("num_batches_tracked"):
                    assert ae.sd[k].dtype == torch.int64 and int(ae.sd[k]) == int(gold[f"s1.buffer.{k}"]) == 1
    close(torch.tensor(losses, dtype=torch.float64), gold["s8.losses"], "the loss trajectory")
    for k in ae.parameter_keys():
        if k in pre:
            assert bool(torch.isfinite(ae.sd[k]).all())
            assert float((ae.sd[k] - start[k]).abs().max()) <= ac.STEPS * ac.adam_step_bound(ac.LR)
        else:
            close(ae.sd[k], gold[f"s8.param.{k}"], f"step 8 {k}")
    assert tr.t == ac.STEPS and tr.state_dict()["t"] == ac.STEPS


def test_eval_mode_matches_the_reference_in_float64(gold, inputs):
    ae = ae_of(inputs["eval_sd"])
    x = torch.from_numpy(inputs["eval_rows"]).double()
    z = ae.encode(x)
    close(z, gold["eval.latents"], "eval-mode latents")
    assert float((z.norm(dim=-1) - 1).abs().max()) <= 1e-12
    l2, cos = ae.reconstruction_loss(x)
    close(torch.stack([l2, cos]), gold["eval.losses"], "eval-mode losses")
    # the reconstruction is decode(encode(x)), and the decoder half is LanguageDecoder's
    out = ae.decode(z)
    assert abs(float(((out - x) ** 2).mean()) - float(l2)) <= 1e-12
    assert torch.equal(LanguageDecoder.from_state_dict(ae.state_dict()).decode(z), out)


def test_state_dict_layout_is_the_references():
    with open(os.path.join(GOLD, "autoencoder_state_dict_layout.json")) as f:
        want = json.load(f)
    for name, (feature, enc, dec) in (("fixture", (ac.FEATURE, ac.ENC, ac.DEC)), ("clip", ac.CLIP)):
        sd = LanguageAutoencoder.init(enc, dec, feature, seed=3).state_dict()
        assert list(sd) == list(want[name])                    # names, in the reference's order
        for k, v in sd.items():
            assert list(v.shape) == want[name][k]["shape"] and str(v.dtype) == want[name][k]["dtype"], k
    ae = LanguageAutoencoder.init(ac.ENC, ac.DEC, ac.FEATURE, seed=3)
    for i, w in enumerate(ae.encoder_dims):
        b = 1 / np.sqrt(ae.sd[f"{ac.enc_key(i)}.weight"].shape[1])
        assert float(ae.sd[f"{ac.enc_key(i)}.weight"].abs().max()) <= b and float(ae.sd[f"{ac.enc_key(i)}.bias"].abs().max()) <= b
    assert float(ae.sd["encoder.1.weight"].min()) == 1 and float(ae.sd["encoder.1.running_var"].min()) == 1
    assert float(ae.sd["encoder.1.bias"].abs().max()) == 0 and int(ae.sd["encoder.1.num_batches_tracked"]) == 0
    same = LanguageAutoencoder.init(ac.ENC, ac.DEC, ac.FEATURE, seed=3)
    other = LanguageAutoencoder.init(ac.ENC, ac.DEC, ac.FEATURE, seed=4)
    assert all(torch.equal(same.sd[k], ae.sd[k]) for k in ae.sd)
    assert not torch.equal(other.sd["encoder.0.weight"], ae.sd["encoder.0.weight"])
    with pytest.raises(KeyError):
        LanguageAutoencoder({k: v for k, v in ae.sd.items() if k != "encoder.1.running_var"})


def test_checkpoints_round_trip(tmp_path, inputs):
    ae = ae_of(inputs["eval_sd"], torch.float32)
    path = str(tmp_path / "best_ckpt.pth")
    ae.save(path)
    raw = torch.load(path, map_location="cpu")
    assert list(raw) == list(ae.sd) and raw["encoder.1.num_batches_tracked"].dtype == torch.int64
    back = LanguageAutoencoder.load(path)
    assert all(torch.equal(back.sd[k], ae.sd[k]) and back.sd[k].dtype == ae.sd[k].dtype for k in ae.sd)
    dec = LanguageDecoder.load(path)
    z = ae.encode(torch.from_numpy(inputs["eval_rows"]))
    assert dec.dims == [ac.ENC[-1]] + ac.DEC and torch.equal(dec.decode(z), ae.decode(z))
    # the decoder shares the weights: an update in place shows through
    shared = ae.decoder()
    ae.sd["decoder.0.bias"].add_(1.0)
    assert torch.equal(shared.biases[0], ae.sd["decoder.0.bias"])
    # to(): a copy; the count stays int64
    d = ae.to(dtype=torch.float64)
    assert d.sd["encoder.0.weight"].dtype == torch.float64 and d.sd["encoder.1.num_batches_tracked"].dtype == torch.int64
    assert d.sd["encoder.0.weight"].data_ptr() != ae.sd["encoder.0.weight"].data_ptr() and not ae.native_ok()


def _fit(rows, epochs, **kw):
    ae = LanguageAutoencoder.init(ac.ENC, ac.DEC, ac.FEATURE, seed=11)
    return ae, fit(ae, rows, num_epochs=epochs, batch_size=64, lr=ac.LR, cos_weight=ac.COS_WEIGHT, seed=5, **kw)


def test_fit_follows_the_references_loop(tmp_path):
    rows = torch.from_numpy(ac.unit_rows(300, ac.FEATURE, 77))
    ckpt = str(tmp_path / "ckpt")
    ae, res = _fit(rows, 3, eval_from_epoch=0, ckpt_dir=ckpt)
    # 300 rows in batches of 64: four full batches and one of 44, every epoch
    assert int(ae.sd["encoder.1.num_batches_tracked"]) == 3 * 5
    again, res2 = _fit(rows, 3, eval_from_epoch=0)
    assert all(torch.equal(again.sd[k], ae.sd[k]) for k in ae.sd)
    assert (res2.best_epoch, res2.best_loss) == (res.best_epoch, res.best_loss)
    # the loss after each epoch, from runs that stop there (the same seed gives the same permutations)
    after, states = [], []
    for e in range(1, 4):
        a, _ = _fit(rows, e, eval_from_epoch=99)
        l2, cos = a.reconstruction_loss(rows)
        after.append(float(l2 + cos))
        states.append(a.sd)
    best = min(range(3), key=lambda e: (after[e], e))
    assert after[best] < 100 and res.best_epoch == best and res.best_loss == after[best]
    saved = torch.load(os.path.join(ckpt, "best_ckpt.pth"), map_location="cpu")
    assert all(torch.equal(saved[k], states[best][k]) and torch.equal(res.state_dict[k], states[best][k]) for k in saved)
    # evaluated from epoch 2 on only: whatever the earlier losses were, epoch 2 is the best
    _, late = _fit(rows, 3, eval_from_epoch=2)
    assert late.best_epoch == 2 and late.best_loss == after[2]
    # never evaluated: the reference's initial values, and nothing is saved
    none_dir = str(tmp_path / "none")
    _, never = _fit(rows, 2, eval_from_epoch=91, ckpt_dir=none_dir)
    assert (never.best_epoch, never.best_loss, never.state_dict) == (0, 100.0, None)
    assert not os.path.exists(os.path.join(none_dir, "best_ckpt.pth"))


def test_compress_feature_dir(tmp_path, inputs):
    ae = ae_of(inputs["eval_sd"], torch.float32)
    src, dst = tmp_path / "language_features", tmp_path / "language_features_dim3"
    src.mkdir()
    tables = {"frame_00001": 5, "frame_00002": 1, "frame_00010": 70}
    for i, (name, n) in enumerate(tables.items()):
        np.save(src / f"{name}_f.npy", ac.unit_rows(n, ac.FEATURE, 100 + i))
        np.save(src / f"{name}_s.npy", np.full((4, 6, 7), i, np.int32))
    np.save(src / "notes.npy", np.zeros(3))                     # neither a table nor a segment map
    rows, counts = load_feature_dir(str(src))
    assert dict(counts) == {f"{k}_f": v for k, v in tables.items()} and list(counts) == sorted(counts)
    assert rows.shape == (76, ac.FEATURE) and rows.dtype == torch.float32
    done = compress_feature_dir(ae, str(src), str(dst))
    assert dict(done) == dict(counts)
    assert sorted(os.listdir(dst)) == sorted([f"{k}_f.npy" for k in tables] + [f"{k}_s.npy" for k in tables])
    z = ae.encode(rows).numpy()
    start = 0
    for i, (name, n) in enumerate(tables.items()):
        got = np.load(dst / f"{name}_f.npy")
        assert got.shape == (n, ac.ENC[-1]) and got.dtype == np.float32
        # eval mode: a row does not depend on its file, up to float32 rounding (torch's CPU GEMM blocks by size;
        # the native path repeats bit for bit, tests/test_autoencoder_gpu.py)
        assert np.abs(got - z[start:start + n]).max() <= 1e-6
        np.testing.assert_array_equal(np.load(dst / f"{name}_s.npy"), np.full((4, 6, 7), i, np.int32))
        start += n
    with pytest.raises(FileNotFoundError):
        compress_feature_dir(ae, str(dst / "nothing"), str(tmp_path / "out"))


def test_a_batch_of_one_row_is_refused(inputs):
    ae = ae_of(inputs["train_sd"], torch.float32)
    tr = AutoencoderTrainer(ae)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        tr.step(torch.from_numpy(inputs["batches"][0][:1]))
    assert tr.t == 0
    with pytest.raises(ValueError, match="wide"):
        tr.step(torch.zeros(4, ac.FEATURE + 16))


# ---- the C ABI without a device -------------------------------------------------------------------------------
FAKE = 64                                                       # never dereferenced: every call returns early


def net_struct(feature=ac.FEATURE, enc=ac.ENC, dec=ac.DEC, ptr=FAKE):
    s = _lib.Autoencoder()
    s.n_enc, s.n_dec, s.feature_dim = len(enc), len(dec), feature
    for i, d in enumerate(enc):
        s.enc_dims[i] = d
        s.p.enc_w[i] = s.p.enc_b[i] = ptr
        if i:
            s.p.bn_w[i] = s.p.bn_b[i] = s.bn_mean[i] = s.bn_var[i] = s.bn_count[i] = ptr
    for j, d in enumerate(dec):
        s.dec_dims[j] = d
        s.p.dec_w[j] = s.p.dec_b[j] = ptr
    return s


def test_abi_refuses_bad_arguments_before_the_device():
    lib = _lib.load()
    err = lambda: lib.lsr_last_error().decode()
    net = net_struct()
    ref, p = ctypes.byref(net), ctypes.c_void_p(FAKE)
    big = 1 << 40

    def refused(rc, text):
        assert rc == 1 and text in err(), (rc, err())           # LSR_EINVAL

    def step(n=ref, m=ctypes.byref(net.p), v=ctypes.byref(net.p), batch=37, rows=p, losses=p, ws=p, ws_bytes=big, t=1):
        return lib.lsr_ae_train_step(n, m, v, batch, rows, ac.LR, 0.9, 0.999, 1e-8, t, ac.COS_WEIGHT, losses, ws, ws_bytes, None)

    # the size queries
    train_bytes = lib.lsr_ae_workspace_size(ref, 37, 1)
    eval_bytes = lib.lsr_ae_workspace_size(ref, 200, 0)
    assert train_bytes > 37 * 4 * 2 * (sum(ac.ENC) + sum(ac.DEC)) and eval_bytes > 0
    assert lib.lsr_ae_workspace_size(ref, 64, 1) > train_bytes
    assert lib.lsr_ae_workspace_size(ref, 10 ** 7, 0) == lib.lsr_ae_workspace_size(ref, _lib.AE_EVAL_CHUNK, 0)
    assert lib.lsr_ae_workspace_size(None, 37, 1) == -1 and "null autoencoder" in err()
    assert lib.lsr_ae_workspace_size(ref, 65, 1) == -1 and "[2, 64]" in err()
    assert lib.lsr_ae_workspace_size(ref, 1, 1) == -1 and "[2, 64]" in err()
    assert lib.lsr_ae_workspace_size(ref, -1, 0) == -1 and "n_rows must be >= 0" in err()
    # shapes
    for bad in (net_struct(feature=40, dec=[16, 32, 40]), net_struct(enc=[24, 16, 3]), net_struct(dec=[16, 8200, 48]),
                net_struct(feature=8192, dec=[16, 32, 8192])):
        refused(lib.lsr_ae_encode(ctypes.byref(bad), 4, p, p, p, big, None), "multiple of 16")
        assert lib.lsr_ae_workspace_size(ctypes.byref(bad), 4, 0) == -1
    refused(lib.lsr_ae_encode(ctypes.byref(net_struct(enc=[32, 16, 48])), 4, p, p, p, big, None), "latent width")
    refused(lib.lsr_ae_encode(ctypes.byref(net_struct(dec=[16, 32, 64])), 4, p, p, p, big, None), "end at feature_dim")
    nine = net_struct()
    nine.n_dec = 9
    refused(lib.lsr_ae_encode(ctypes.byref(nine), 4, p, p, p, big, None), "[1, 8]")
    # null pointers
    refused(lib.lsr_ae_encode(None, 4, p, p, p, big, None), "null autoencoder")
    refused(lib.lsr_ae_encode(ref, 4, None, p, p, big, None), "rows and latents")
    refused(lib.lsr_ae_encode(ref, 4, p, None, p, big, None), "rows and latents")
    refused(lib.lsr_ae_encode(ref, 4, p, p, None, big, None), "workspace is required")
    refused(lib.lsr_ae_eval_loss(ref, 4, p, None, p, big, None), "rows and sums")
    hole = net_struct()
    hole.p.enc_b[1] = None
    refused(lib.lsr_ae_encode(ctypes.byref(hole), 4, p, p, p, big, None), "weight or bias")
    hole = net_struct()
    hole.bn_var[2] = None
    refused(lib.lsr_ae_eval_loss(ctypes.byref(hole), 4, p, p, p, big, None), "BatchNorm buffer of encoder layer 2")
    hole = net_struct()
    hole.bn_count[1] = None
    assert lib.lsr_ae_encode(ctypes.byref(hole), 0, p, p, p, big, None) == 0     # eval mode does not count batches
    refused(step(n=ctypes.byref(hole)), "BatchNorm buffer of encoder layer 1")
    moments = net_struct().p
    moments.dec_w[2] = None
    refused(step(m=ctypes.byref(moments)), "moments of every parameter")
    refused(step(v=None), "moments of every parameter")
    refused(step(rows=None), "rows and losses")
    refused(step(losses=None), "rows and losses")
    # the batch, the step number, the workspace
    refused(step(batch=65), "[2, 64]")
    refused(step(batch=1), "[2, 64]")
    refused(step(t=0), "t must be >= 1")
    refused(step(ws_bytes=train_bytes - 1), f"{train_bytes} are needed")
    refused(step(ws=ctypes.c_void_p(72)), "16-byte aligned")
    refused(lib.lsr_ae_encode(ref, 200, p, p, p, eval_bytes - 1, None), f"{eval_bytes} are needed")
    refused(lib.lsr_ae_eval_loss(ref, 200, p, p, p, eval_bytes - 1, None), f"{eval_bytes} are needed")
    refused(lib.lsr_ae_encode(ref, -1, p, p, p, big, None), "n_rows must be >= 0")
    assert lib.lsr_ae_encode(ref, 0, p, p, p, big, None) == 0   # no rows: nothing is launched


# lsr_ae_workspace_size at (batch 2, 37, 64 in training; 0, 1, 63, 64, 65, 2048, 2049 rows in eval mode): what the
# build that introduced the unit returned, written down, not recomputed.  A changed number is a changed layout
# (tests/test_workspace_layout.py does the same for the queries named *_bytes).
WORKSPACE_SIZES = {
    "fixture": ((ac.FEATURE, ac.ENC, ac.DEC), (6400, 48128, 78592), (1792, 1792, 21760, 21760, 23040, 680448, 680448)),
    "odd": (ac.ODD, (13056, 132608, 222208), (3328, 3328, 80896, 81920, 84224, 2589696, 2589696)),
    "clip": (ac.CLIP, (37632, 527360, 903936), (5120, 5120, 157184, 159488, 162560, 5040128, 5040128)),
    "video": (ac.VIDEO, (262400, 3687936, 6329344), (36352, 36352, 1244672, 1264128, 1284096, 39944192, 39944192)),
}


@pytest.mark.parametrize("name", sorted(WORKSPACE_SIZES))
def test_workspace_sizes_are_the_recorded_ones(name):
    (feature, enc, dec), train, evals = WORKSPACE_SIZES[name]
    lib, net = _lib.load(), net_struct(feature, enc, dec, ptr=None)     # the query reads no pointer
    assert tuple(lib.lsr_ae_workspace_size(ctypes.byref(net), B, 1) for B in (2, 37, 64)) == train
    assert tuple(lib.lsr_ae_workspace_size(ctypes.byref(net), N, 0) for N in (0, 1, 63, 64, 65, 2048, 2049)) == evals


def test_ctypes_mirrors_match_the_header(tmp_path):
    """AeParams and Autoencoder have the C compiler's field offsets and sizes."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{os.path.join(ROOT, "include", "lsr_autoencoder.h")}"',
             "int main(void) {"]
    want = {}
    for cls, c in ((_lib.AeParams, "lsr_ae_params"), (_lib.Autoencoder, "lsr_autoencoder")):
        lines.append(f'printf("{c} size %zu\\n", sizeof({c}));')
        want[(c, "size")] = ctypes.sizeof(cls)
        for n, _ in cls._fields_:
            lines.append(f'printf("{c} {n} %zu\\n", offsetof({c}, {n}));')
            want[(c, n)] = getattr(cls, n).offset
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = {}
    for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines():
        c, n, v = line.split()
        got[(c, n)] = int(v)
    assert got == want
    text = open(os.path.join(ROOT, "include", "lsr_autoencoder.h")).read()
    for name in ("MAX_LAYERS", "MAX_WIDTH", "MAX_LATENT", "MAX_BATCH", "EVAL_CHUNK", "API_VERSION"):
        assert getattr(_lib, "AE_" + name) == int(re.search(rf"^#define LSR_AE_{name} (\d+)", text, re.M).group(1)), name
