"""GPU checks of the native language autoencoder (csrc/autoencoder.hip through language_autoencoder.py).

Tolerance rule (tests/test_query_gpu.py:3-8): against the float64 value, the native max abs error of a tensor
may be at most 8x the float32 reference's error for that tensor.  For the committed fixture that float32
error is the one its generator measured on the reference's own code; for other shapes it is measured here the
same way, the torch formulas in float32 against the same formulas in float64, both on the CPU.

Gradients are checked without an extra output: after one step from zero moments exp_avg = (1 - beta1) g and
exp_avg_sq = (1 - beta2) g^2, compared per tensor under the rule; the parameter update is checked against
Adam's formula evaluated in float64 from the native path's own moments.  That formula is four float32
operations on an update of at most adam_step_bound(lr), then one rounding of the parameter, so the native
value may differ from it by 2^-24 max|p| + 8 * 2^-24 * adam_step_bound(lr).

The biases of the Linear layers in front of a BatchNorm have a true gradient of zero and a float32 gradient
of rounding noise (autoencoder_cases.PRE_BN_RULE): they, and their moments, are required to be finite and to
move by at most Adam's own bound per step; running_mean is compared after a single step only; eval-mode
latents are compared only between paths that share one state dict."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import autoencoder_cases as ac
from diff_gaussian_rasterization import _lib
from language_autoencoder import COS_EPS, AutoencoderTrainer, LanguageAutoencoder, compress_feature_dir, fit
from language_query import LanguageDecoder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = ac.TOL
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "autoencoder_golden.npz")))


@pytest.fixture(scope="module")
def inputs():
    return ac.fixture_inputs()


def ae_of(sd, dtype=torch.float32, device="cpu"):
    return LanguageAutoencoder(ac.torch_state_dict(sd, torch, dtype)).to(device=device)


def err(a, ref):
    ref = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.asarray(ref))
    return float((a.detach().cpu().double() - ref.double().cpu()).abs().max())


class Rule:
    """Collects (what, native error, float32 reference error), prints every figure, then asserts the rule."""

    def __init__(self, what):
        self.what, self.rows = what, []

    def add(self, name, native, ref64, ref32_err):
        self.rows.append((name, err(native, ref64), float(ref32_err)))

    def check(self):
        bad = []
        for name, e, r in self.rows:
            print(f"{self.what}: {name}: native error {e:.3g}, float32 reference {r:.3g}")
            if not e <= TOL * r:
                bad.append((name, e, r))
        assert not bad, f"{self.what}: beyond {TOL} x the float32 reference's error: {bad}"


def step_with(ae, x, lr=ac.LR, cos_weight=ac.COS_WEIGHT):
    tr = AutoencoderTrainer(ae, lr=lr, cos_weight=cos_weight)
    l2, cos = tr.step(x)
    return tr, torch.stack([l2.detach().cpu().double(), cos.detach().cpu().double()])


def check_pre_bn(ae, tr, start, steps, lr=ac.LR):
    for k in ae.pre_bn_bias_keys():
        for t in (ae.sd[k], tr.exp_avg[k], tr.exp_avg_sq[k]):
            assert bool(torch.isfinite(t).all()), k
        moved = float((ae.sd[k].cpu().double() - start[k].double()).abs().max())
        assert moved <= steps * ac.adam_step_bound(lr) * (1 + 1e-6), (k, moved)


def check_adam_formula(ae, tr, start, lr=ac.LR):
    """After step 1: every parameter against Adam's formula in float64 from the native moments."""
    b1, b2 = ac.BETAS
    for k in ae.parameter_keys():
        m, v, p0 = tr.exp_avg[k].cpu().double(), tr.exp_avg_sq[k].cpu().double(), start[k].double()
        want = p0 - lr / (1 - b1) * m / (v.sqrt() / math.sqrt(1 - b2) + ac.ADAM_EPS)
        bound = EPS32 * float(want.abs().max()) + 8 * EPS32 * ac.adam_step_bound(lr)
        e = err(ae.sd[k], want)
        assert e <= bound, f"{k}: {e:.3g} from Adam's formula, bound {bound:.3g}"


def one_step(feature, enc, dec, B, seed, what):
    """One native training step against the torch formulas in float64, the float32 error measured here."""
    sd = ac.state_dict_np(feature, enc, dec, seed)
    x = torch.from_numpy(ac.unit_rows(B, feature, seed + 1))
    a64, a32, nat = ae_of(sd, torch.float64), ae_of(sd), ae_of(sd, device="cuda")
    start = {k: v.clone() for k, v in a32.sd.items()}
    t64, l64 = step_with(a64, x.double())
    t32, l32 = step_with(a32, x)
    assert nat.native_ok()
    tn, ln = step_with(nat, x.cuda())
    torch.cuda.synchronize()
    pre = set(nat.pre_bn_bias_keys())
    rule = Rule(what)
    rule.add("losses", ln, l64, err(l32, l64))
    for k in nat.parameter_keys():
        if k in pre:
            continue
        rule.add(f"exp_avg {k}", tn.exp_avg[k], t64.exp_avg[k], err(t32.exp_avg[k], t64.exp_avg[k]))
        rule.add(f"exp_avg_sq {k}", tn.exp_avg_sq[k], t64.exp_avg_sq[k], err(t32.exp_avg_sq[k], t64.exp_avg_sq[k]))
    for k in nat.sd:
        if k.endswith(("running_mean", "running_var")):
            rule.add(k, nat.sd[k], a64.sd[k], err(a32.sd[k], a64.sd[k]))
        if k.endswith("num_batches_tracked"):
            assert nat.sd[k].dtype == torch.int64 and int(nat.sd[k]) == 1
    rule.check()
    check_adam_formula(nat, tn, start)
    check_pre_bn(nat, tn, start, 1)


def test_one_step_at_the_fixture_batch(gold, inputs):
    """Against the reference's recorded float64 step, with the float32 errors its generator measured."""
    nat = ae_of(inputs["train_sd"], device="cuda")
    start = {k: v.cpu().clone() for k, v in nat.sd.items()}
    tn, ln = step_with(nat, torch.from_numpy(inputs["batches"][0]).cuda())
    pre = set(nat.pre_bn_bias_keys())
    rule = Rule("fixture, B = 37")
    rule.add("losses", ln, gold["s1.losses"], gold["s1.losses.f32_err"])
    for k in nat.parameter_keys():
        if k in pre:
            continue
        rule.add(f"param {k}", nat.sd[k], gold[f"s1.param.{k}"], gold[f"s1.param.{k}.f32_err"])
        rule.add(f"exp_avg {k}", tn.exp_avg[k], gold[f"s1.exp_avg.{k}"], gold[f"s1.exp_avg.{k}.f32_err"])
        rule.add(f"exp_avg_sq {k}", tn.exp_avg_sq[k], gold[f"s1.exp_avg_sq.{k}"], gold[f"s1.exp_avg_sq.{k}.f32_err"])
    for k in nat.sd:
        if k.endswith(("running_mean", "running_var")):
            rule.add(k, nat.sd[k], gold[f"s1.buffer.{k}"], gold[f"s1.buffer.{k}.f32_err"])
        if k.endswith("num_batches_tracked"):
            assert int(nat.sd[k]) == int(gold[f"s1.buffer.{k}"]) == 1
    rule.check()
    check_adam_formula(nat, tn, start)
    check_pre_bn(nat, tn, start, 1)


@pytest.mark.parametrize("B", [2, 64])
def test_one_step_at_the_fixture_shape(B):
    one_step(ac.FEATURE, ac.ENC, ac.DEC, B, 300 + B, f"fixture shape, B = {B}")


def test_one_step_at_odd_widths():
    """A width of 16, a width of 144 (no multiple of the 32-column slab or the 64-row weight tile), a latent of 6."""
    one_step(*ac.ODD, 37, 410, "80 -> 144 -> 16 -> 6 -> 32 -> 144 -> 80, B = 37")


def test_one_step_at_the_clip_shape():
    one_step(*ac.CLIP, 64, 420, "CLIP shape, B = 64")


def test_one_step_at_the_video_shape():
    one_step(*ac.VIDEO, 16, 430, "video shape, B = 16")


def test_eight_steps_at_the_fixture_shape(gold, inputs):
    nat = ae_of(inputs["train_sd"], device="cuda")
    start = {k: v.cpu().clone() for k, v in nat.sd.items()}
    tr = AutoencoderTrainer(nat, lr=ac.LR, cos_weight=ac.COS_WEIGHT)
    losses = []
    for s in range(ac.STEPS):
        losses.append(torch.stack(tr.step(torch.from_numpy(inputs["batches"][s]).cuda())))
    losses = torch.stack(losses)
    pre = set(nat.pre_bn_bias_keys())
    rule = Rule("fixture, 8 steps")
    rule.add("loss trajectory", losses, gold["s8.losses"], gold["s8.losses.f32_err"])
    for k in nat.parameter_keys():
        if k not in pre:
            rule.add(f"param {k}", nat.sd[k], gold[f"s8.param.{k}"], gold[f"s8.param.{k}.f32_err"])
    rule.check()
    check_pre_bn(nat, tr, start, ac.STEPS)
    assert int(nat.sd["encoder.1.num_batches_tracked"]) == ac.STEPS and tr.t == ac.STEPS


@pytest.fixture(scope="module")
def eval_case(inputs):
    """The fixture's eval state on 2049 rows (one more than a pass of the kernels takes): float64 and float32
    torch results on the CPU, computed once."""
    x = torch.from_numpy(ac.unit_rows(_lib.AE_EVAL_CHUNK + 1, ac.FEATURE, 510))
    a64, a32 = ae_of(inputs["eval_sd"], torch.float64), ae_of(inputs["eval_sd"])
    return dict(x=x, a64=a64, a32=a32, z64=a64.encode(x.double()), z32=a32.encode(x))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 200, _lib.AE_EVAL_CHUNK + 1])
def test_encode_and_reconstruction_loss(eval_case, inputs, N):
    c = eval_case
    nat = ae_of(inputs["eval_sd"], device="cuda")
    x = c["x"][:N]
    z = nat.encode(x.cuda())
    assert z.shape == (N, ac.ENC[-1]) and z.dtype == torch.float32 and z.is_cuda
    rule = Rule(f"eval mode, N = {N}")
    rule.add("latents", z, c["z64"][:N], err(c["a32"].encode(x), c["z64"][:N]))
    l64 = torch.stack(c["a64"].reconstruction_loss(x.double()))
    l32 = torch.stack(c["a32"].reconstruction_loss(x))
    ln = torch.stack(nat.reconstruction_loss(x.cuda()))
    assert ln.dtype == torch.float64 and ln.is_cuda
    rule.add("reconstruction loss", ln, l64, err(l32, l64))
    rule.check()
    assert float((z.norm(dim=-1) - 1).abs().max()) <= 1e-6
    # the eval-mode statistics are read, not written
    assert all(torch.equal(nat.sd[k].cpu(), c["a32"].sd[k]) for k in nat.sd)
    # [..., feature_dim] keeps its leading shape; no rows: no launch
    if N == 200:
        assert torch.equal(nat.encode(x.cuda().reshape(4, 50, ac.FEATURE)), z.reshape(4, 50, -1))
        assert nat.encode(x[:0].cuda()).shape == (0, ac.ENC[-1])


def test_a_zero_latent_gives_nan_in_its_own_row_only(inputs):
    """With no bias anywhere and zero running means a zero row passes through every layer as zero: z = 0, and
    z / |z| is NaN (no epsilon, as lsr_query.h) in that row alone."""
    sd = {k: (np.zeros_like(v) if k.endswith((".bias", "running_mean")) else v) for k, v in inputs["eval_sd"].items()}
    nat, cpu = ae_of(sd, device="cuda"), ae_of(sd, torch.float64)
    x = torch.from_numpy(ac.unit_rows(70, ac.FEATURE, 520))
    x[5] = 0
    x[64] = 0
    z = nat.encode(x.cuda()).cpu()
    bad = torch.isnan(z).any(dim=1)
    assert bad.nonzero().flatten().tolist() == [5, 64] and bool(torch.isnan(z[5]).all())
    assert bool(torch.isnan(cpu.encode(x.double())[5]).all())
    keep = ~bad
    assert torch.equal(z[keep], nat.encode(x[keep].cuda()).cpu())
    l2, cos = nat.reconstruction_loss(x.cuda())
    assert bool(torch.isnan(l2)) and bool(torch.isnan(cos))     # as the reference's mean over rows


def test_results_repeat_bit_for_bit(inputs):
    a, b = ae_of(inputs["train_sd"], device="cuda"), ae_of(inputs["train_sd"], device="cuda")
    ta, tb = AutoencoderTrainer(a, lr=ac.LR), AutoencoderTrainer(b, lr=ac.LR)
    for s in range(3):
        x = torch.from_numpy(inputs["batches"][s]).cuda()
        la, lb = ta.step(x), tb.step(x.clone())
        assert torch.equal(torch.stack(la), torch.stack(lb))
    for k in a.sd:
        assert torch.equal(a.sd[k], b.sd[k]), k
    for k in ta.exp_avg:
        assert torch.equal(ta.exp_avg[k], tb.exp_avg[k]) and torch.equal(ta.exp_avg_sq[k], tb.exp_avg_sq[k]), k
    nat = ae_of(inputs["eval_sd"], device="cuda")
    x = torch.from_numpy(ac.unit_rows(200, ac.FEATURE, 530)).cuda()
    z = nat.encode(x)
    assert torch.equal(z, nat.encode(x))
    assert torch.equal(torch.stack(nat.reconstruction_loss(x)), torch.stack(nat.reconstruction_loss(x)))
    # a row's latent does not depend on the other rows of the call
    assert torch.equal(z[131:132], nat.encode(x[131:132]))
    assert torch.equal(z.flip(0), nat.encode(x.flip(0)))
    assert torch.equal(z[60:70], nat.encode(x[60:70]))


SENT = 12345.0


def guarded(t, pad=64):
    """A copy of t inside a buffer with `pad` sentinel elements on each side (the copy stays 256-byte aligned)."""
    fill = SENT if t.is_floating_point() else 12345
    buf = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype, device="cuda")
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf, pad


def intact(buf, pad):
    fill = SENT if buf.is_floating_point() else (12345 if buf.dtype == torch.int64 else 0xA5)
    return bool((buf[:pad] == fill).all()) and bool((buf[-pad:] == fill).all())


def guarded_bytes(n):
    buf = torch.full((n + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf[256:256 + n], buf, 256


def test_nothing_is_written_outside_the_buffers(inputs):
    guards = []

    def keep(t):
        view, buf, pad = guarded(t)
        guards.append((buf, pad))
        return view

    sd = {k: keep(v.cuda()) for k, v in ac.torch_state_dict(inputs["train_sd"], torch).items()}
    nat = LanguageAutoencoder(sd)
    assert nat.native_ok() and all(nat.sd[k].data_ptr() == sd[k].data_ptr() for k in sd)
    tr = AutoencoderTrainer(nat, lr=ac.LR)
    tr.exp_avg = {k: keep(v) for k, v in tr.exp_avg.items()}
    tr.exp_avg_sq = {k: keep(v) for k, v in tr.exp_avg_sq.items()}
    lib, net = _lib.load(), nat._struct()
    stream = torch.cuda.current_stream().cuda_stream
    for B in (37, 64, 2):
        n = lib.lsr_ae_workspace_size(ctypes.byref(net), B, 1)
        ws, buf, pad = guarded_bytes(n)                         # exactly the queried size
        guards.append((buf, pad))
        tr._ws[B] = (ws, n)
        x = keep(torch.from_numpy(inputs["batches"][0][:B]).cuda())
        tr.step(x)
    for N in (1, 65, 200):
        n = lib.lsr_ae_workspace_size(ctypes.byref(net), N, 0)
        ws, buf, pad = guarded_bytes(n)
        guards.append((buf, pad))
        x = keep(torch.from_numpy(inputs["eval_rows"][:N]).cuda())
        z = keep(torch.zeros(N, ac.ENC[-1], device="cuda"))
        sums = keep(torch.zeros(2, dtype=torch.float64, device="cuda"))
        _lib.check(lib.lsr_ae_encode(ctypes.byref(net), N, x.data_ptr(), z.data_ptr(), ws.data_ptr(), n, stream), "encode")
        _lib.check(lib.lsr_ae_eval_loss(ctypes.byref(net), N, x.data_ptr(), sums.data_ptr(), ws.data_ptr(), n, stream), "loss")
        assert torch.equal(z, nat.encode(x))
        assert torch.equal(sums[0] / (N * ac.FEATURE), nat.reconstruction_loss(x)[0])
    torch.cuda.synchronize()
    assert all(intact(buf, pad) for buf, pad in guards)
    assert all(bool(torch.isfinite(v).all()) for v in nat.sd.values() if v.is_floating_point())


def test_fit_compress_and_decode_end_to_end(tmp_path):
    """fit on the device, compress a directory, decode the compressed rows with LanguageDecoder: the mean
    cosine with the inputs is 1 - cos of reconstruction_loss.

    Per row: the rule applied to the tensor of the 500 cosines.  The float64 values are the torch formulas' on the
    trained state dict, the float32 reference error e32 is the largest per-row error of the same pipeline as
    float32 torch ops, and every native per-row cosine must lie within 8 e32.

    The means: the float32 reference's error of its own mean is one sample of an average of N = 500 roundings of
    either sign, anywhere between nothing and a few e32 / sqrt(N) (3.8e-11 on one recorded run, 1.5e-9 on
    another), so a single sample of it is no yardstick.  What the float32 reference's mean can be expected to miss
    by is the spread of that average, e32 / sqrt(N): row errors of size up to e32 that do not share a sign.  Each
    native mean (of the decoded compressed rows, and 1 - cos of reconstruction_loss) must lie within 8 e32 / sqrt(N)
    of the float64 mean, and the two must agree with each other within the same bound.  An error that every row
    shares does not shrink with N and fails this."""
    rows = torch.from_numpy(ac.unit_rows(500, ac.FEATURE, 610))
    src, dst = tmp_path / "language_features", tmp_path / "language_features_dim3"
    src.mkdir()
    np.save(src / "a_f.npy", rows[:180].numpy())
    np.save(src / "b_f.npy", rows[180:].numpy())
    np.save(src / "a_s.npy", np.zeros((4, 5, 6), np.int32))
    ae = LanguageAutoencoder.init(ac.ENC, ac.DEC, ac.FEATURE, seed=21).to("cuda")
    res = fit(ae, rows.cuda(), num_epochs=2, batch_size=64, lr=ac.LR, cos_weight=ac.COS_WEIGHT, seed=6,
              eval_from_epoch=0, ckpt_dir=str(tmp_path / "ckpt"))
    assert int(ae.sd["encoder.1.num_batches_tracked"]) == 2 * 8 and res.best_epoch in (0, 1) and res.best_loss < 100
    saved = LanguageAutoencoder.load(str(tmp_path / "ckpt" / "best_ckpt.pth"))
    assert all(torch.equal(saved.sd[k], res.state_dict[k].cpu()) for k in saved.sd)
    counts = compress_feature_dir(ae, str(src), str(dst))
    assert dict(counts) == {"a_f": 180, "b_f": 320} and os.path.exists(dst / "a_s.npy")
    z = torch.from_numpy(np.concatenate([np.load(dst / "a_f.npy"), np.load(dst / "b_f.npy")]))
    assert z.shape == (500, ac.ENC[-1]) and torch.equal(z, ae.encode(rows.cuda()).cpu())

    def row_cosines(decoder, latents, x):
        return torch.nn.functional.cosine_similarity(decoder.decode(latents), x, dim=1, eps=COS_EPS).double().cpu()

    dec = LanguageDecoder.from_state_dict(ae.state_dict())
    assert dec.native_ok()
    native = row_cosines(dec, z.cuda(), rows.cuda())
    l2, cos = ae.reconstruction_loss(rows.cuda())
    a64, a32 = ae.to("cpu", torch.float64), ae.to("cpu")
    want = row_cosines(LanguageDecoder.from_state_dict(a64.state_dict()), a64.encode(rows.double()), rows.double())
    ref32 = row_cosines(LanguageDecoder.from_state_dict(a32.state_dict()), a32.encode(rows), rows)
    assert abs(float(want.mean()) - float(1 - a64.reconstruction_loss(rows.double())[1])) <= 1e-12
    e32 = err(ref32, want)
    print(f"end to end: the float32 reference's own mean is {err(ref32.mean(), want.mean()):.3g} from float64")
    rule = Rule("end to end")
    rule.add("cosines of the decoded compressed rows, per row", native, want, e32)
    e32_mean = e32 / math.sqrt(rows.shape[0])
    rule.add("their mean", native.mean(), want.mean(), e32_mean)
    rule.add("1 - cos of reconstruction_loss", 1 - cos, want.mean(), e32_mean)
    rule.add("the two native means, one against the other", native.mean(), (1 - cos).double().cpu(), e32_mean)
    rule.check()
