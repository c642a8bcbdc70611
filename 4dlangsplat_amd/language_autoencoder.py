"""The language autoencoder on the MI355X: the reference's autoencoder/model.py (Autoencoder),
autoencoder/train.py (the training loop, the eval loss and the best-checkpoint rule) and
autoencoder/test.py (the compression of every *_f.npy table to the latent width).

    rows, counts = load_feature_dir(f"{scene}/language_features")
    ae = LanguageAutoencoder.init([256, 128, 64, 32, 3], [16, 32, 64, 128, 256, 256, 512], 512, seed=0).to("cuda")
    best = fit(ae, rows.to("cuda"), num_epochs=100, batch_size=64, ckpt_dir=f"ckpt/{name}")
    ae = LanguageAutoencoder.load(f"ckpt/{name}/best_ckpt.pth").to("cuda")
    compress_feature_dir(ae, f"{scene}/language_features", f"{scene}/language_features_dim3")

The state dict has the reference's keys (encoder.{0,3,6,...} Linear, encoder.{1,4,...} BatchNorm1d with
its running statistics and num_batches_tracked, decoder.{0,2,4,...} Linear), so checkpoints pass both ways;
LanguageDecoder.from_state_dict reads the decoder half of the same file.

The native path (include/lsr_autoencoder.h, csrc/autoencoder.hip) takes float32 CUDA tensors on one
device, nets inside the library's limits and training batches of 2..64 rows; everything else (CPU,
float64, larger batches, other widths) runs the same formulas as torch ops in the input's dtype, as
language_query does.
"""
from __future__ import annotations

import collections
import ctypes
import glob
import math
import os
import re
import shutil

import numpy as np
import torch
import torch.nn.functional as F

from diff_gaussian_rasterization import _lib
from language_query import LanguageDecoder

__all__ = ["LanguageAutoencoder", "AutoencoderTrainer", "FitResult", "fit", "load_feature_dir",
           "compress_feature_dir"]

BN_EPS, BN_MOMENTUM, COS_EPS = 1e-5, 0.1, 1e-8
FitResult = collections.namedtuple("FitResult", ["best_epoch", "best_loss", "state_dict"])


def _enc_key(i):
    return f"encoder.{3 * i}"          # Linear i; its BatchNorm sits at 3 i - 2, the ReLU at 3 i - 1


def _bn_key(i):
    return f"encoder.{3 * i - 2}"


def _c_dtype(t):
    """What the library reads a state-dict tensor as: float32, num_batches_tracked int64."""
    return torch.float32 if t.is_floating_point() else torch.int64


def _dec_key(j):
    return f"decoder.{2 * j}"          # a ReLU sits between the Linear layers


class LanguageAutoencoder:
    """The reference Autoencoder as a flat state dict of tensors, updated in place by training."""

    def __init__(self, sd):
        sd = {re.sub(r"^module\.", "", k): v for k, v in sd.items()}
        n_enc = 0
        while f"{_enc_key(n_enc)}.weight" in sd:
            n_enc += 1
        n_dec = 0
        while f"{_dec_key(n_dec)}.weight" in sd:
            n_dec += 1
        if not n_enc or not n_dec:
            raise KeyError("no encoder.0.weight / decoder.0.weight in the state dict")
        self.n_enc, self.n_dec = n_enc, n_dec
        self.sd = collections.OrderedDict()
        for k in self.keys(n_enc, n_dec):
            if k not in sd:
                raise KeyError(f"{k} is missing from the state dict")
            self.sd[k] = sd[k].detach().contiguous()
        extra = sorted(set(sd) - set(self.sd))
        if extra:
            raise KeyError(f"unexpected keys in the state dict: {extra}")
        prev = self.feature_dim
        for i in range(n_enc):
            w = self.sd[f"{_enc_key(i)}.weight"]
            if w.dim() != 2 or w.shape[1] != prev or tuple(self.sd[f"{_enc_key(i)}.bias"].shape) != (w.shape[0],):
                raise ValueError(f"encoder layer {i}: the shapes do not chain")
            if i and any(tuple(self.sd[f"{_bn_key(i)}.{p}"].shape) != (prev,)
                         for p in ("weight", "bias", "running_mean", "running_var")):
                raise ValueError(f"encoder layer {i}: the BatchNorm is not {prev} wide")
            prev = w.shape[0]
        for j in range(n_dec):
            w = self.sd[f"{_dec_key(j)}.weight"]
            if w.dim() != 2 or w.shape[1] != prev or tuple(self.sd[f"{_dec_key(j)}.bias"].shape) != (w.shape[0],):
                raise ValueError(f"decoder layer {j}: the shapes do not chain")
            prev = w.shape[0]
        self._struct_cache = None

    @staticmethod
    def keys(n_enc, n_dec):
        """The reference's state-dict keys, in its order."""
        out = []
        for i in range(n_enc):
            if i:
                out += [f"{_bn_key(i)}.{p}" for p in ("weight", "bias", "running_mean", "running_var",
                                                      "num_batches_tracked")]
            out += [f"{_enc_key(i)}.weight", f"{_enc_key(i)}.bias"]
        for j in range(n_dec):
            out += [f"{_dec_key(j)}.weight", f"{_dec_key(j)}.bias"]
        return out

    @classmethod
    def init(cls, encoder_dims, decoder_dims, feature_dim=512, seed=0):
        """nn.Linear's default distributions (weight and bias uniform in +-1 / sqrt(fan_in)), BatchNorm
        1 / 0 / 0 / 1, from a seeded CPU generator; the reference's random stream is not reproduced."""
        g = torch.Generator().manual_seed(int(seed))
        sd = {}

        def linear(key, fan_in, fan_out):
            bound = 1.0 / math.sqrt(fan_in)
            sd[f"{key}.weight"] = (torch.rand(fan_out, fan_in, generator=g) * 2 - 1) * bound
            sd[f"{key}.bias"] = (torch.rand(fan_out, generator=g) * 2 - 1) * bound

        prev = int(feature_dim)
        for i, d in enumerate(encoder_dims):
            if i:
                sd[f"{_bn_key(i)}.weight"], sd[f"{_bn_key(i)}.bias"] = torch.ones(prev), torch.zeros(prev)
                sd[f"{_bn_key(i)}.running_mean"], sd[f"{_bn_key(i)}.running_var"] = torch.zeros(prev), torch.ones(prev)
                sd[f"{_bn_key(i)}.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
            linear(_enc_key(i), prev, int(d))
            prev = int(d)
        for j, d in enumerate(decoder_dims):
            linear(_dec_key(j), prev, int(d))
            prev = int(d)
        return cls(sd)

    @classmethod
    def from_state_dict(cls, sd):
        return cls(sd)

    @classmethod
    def load(cls, path, map_location="cpu"):
        """torch.load of a checkpoint of the reference (best_ckpt.pth) or of save()."""
        return cls(torch.load(path, map_location=map_location))

    def state_dict(self):
        """The reference's keys; the tensors are the live ones (clone them to keep a snapshot)."""
        return collections.OrderedDict(self.sd)

    def save(self, path):
        torch.save(collections.OrderedDict((k, v.detach().cpu().clone()) for k, v in self.sd.items()), path)

    # ---- shape ----
    @property
    def feature_dim(self):
        return self.sd["encoder.0.weight"].shape[1]

    @property
    def encoder_dims(self):
        return [self.sd[f"{_enc_key(i)}.weight"].shape[0] for i in range(self.n_enc)]

    @property
    def decoder_dims(self):
        return [self.sd[f"{_dec_key(j)}.weight"].shape[0] for j in range(self.n_dec)]

    @property
    def latent_dim(self):
        return self.encoder_dims[-1]

    @property
    def device(self):
        return self.sd["encoder.0.weight"].device

    @property
    def dtype(self):
        return self.sd["encoder.0.weight"].dtype

    def parameter_keys(self):
        """The trainable tensors, in torch.optim's order (model.parameters())."""
        return [k for k in self.sd if k.endswith((".weight", ".bias"))]

    def pre_bn_bias_keys(self):
        """The biases of the Linear layers that feed a BatchNorm: their true gradient is zero."""
        return [f"{_enc_key(i)}.bias" for i in range(self.n_enc - 1)]

    def to(self, device=None, dtype=None):
        """A copy on `device` with floating tensors of `dtype`; num_batches_tracked stays int64."""
        out = {}
        for k, v in self.sd.items():
            v = v.to(device=device) if device is not None else v
            if dtype is not None and v.is_floating_point():
                v = v.to(dtype)
            out[k] = v.clone() if v is self.sd[k] else v
        return LanguageAutoencoder(out)

    def native_ok(self):
        """Inside include/lsr_autoencoder.h's limits, float32 (the counts int64), on one CUDA device."""
        hidden = self.encoder_dims[:-1] + self.decoder_dims + [self.feature_dim]
        B = _lib.Boundary(self.device)
        return (self.n_enc <= _lib.AE_MAX_LAYERS and self.n_dec <= _lib.AE_MAX_LAYERS
                and all(x % 16 == 0 and 16 <= x <= _lib.AE_MAX_WIDTH for x in hidden)
                and 1 <= self.latent_dim <= _lib.AE_MAX_LATENT and self.decoder_dims[-1] == self.feature_dim
                and self.device.type == "cuda" and all(B.ok(t, _c_dtype(t)) for t in self.sd.values()))

    def _params_struct(self, tensors):
        """lsr_ae_params of a dict with the parameter keys (the parameters, or one of Adam's moments)."""
        s, B = _lib.AeParams(), _lib.Boundary(self.device)

        def ptr(k):
            return B.ptr(tensors[k], k)

        for i in range(self.n_enc):
            s.enc_w[i], s.enc_b[i] = ptr(f"{_enc_key(i)}.weight"), ptr(f"{_enc_key(i)}.bias")
            if i:
                s.bn_w[i], s.bn_b[i] = ptr(f"{_bn_key(i)}.weight"), ptr(f"{_bn_key(i)}.bias")
        for j in range(self.n_dec):
            s.dec_w[j], s.dec_b[j] = ptr(f"{_dec_key(j)}.weight"), ptr(f"{_dec_key(j)}.bias")
        return s

    def _struct(self):
        """lsr_autoencoder over the live tensors (they are updated in place, so it is built once)."""
        if self._struct_cache is None:
            s = _lib.Autoencoder()
            s.n_enc, s.n_dec, s.feature_dim = self.n_enc, self.n_dec, self.feature_dim
            for i, d in enumerate(self.encoder_dims):
                s.enc_dims[i] = d
            for j, d in enumerate(self.decoder_dims):
                s.dec_dims[j] = d
            s.p = self._params_struct(self.sd)
            B = _lib.Boundary(self.device)
            for i in range(1, self.n_enc):
                s.bn_mean[i] = B.ptr(self.sd[f"{_bn_key(i)}.running_mean"], "running_mean")
                s.bn_var[i] = B.ptr(self.sd[f"{_bn_key(i)}.running_var"], "running_var")
                s.bn_count[i] = B.ptr(self.sd[f"{_bn_key(i)}.num_batches_tracked"], "num_batches_tracked", torch.int64)
            self._struct_cache = s
        return self._struct_cache

    def _workspace(self, n_rows, training):
        n = _lib.load().lsr_ae_workspace_size(ctypes.byref(self._struct()), n_rows, 1 if training else 0)
        if n < 0:
            _lib.check(int(-n), "lsr_ae_workspace_size")
        return torch.empty(n, dtype=torch.uint8, device=self.device), n

    def _takes_native(self, x):
        return x.dtype == torch.float32 and x.device == self.device and self.native_ok()

    def _check_rows(self, x):
        if x.shape[-1] != self.feature_dim:
            raise ValueError(f"the rows are {x.shape[-1]} wide, the autoencoder takes {self.feature_dim}")
        if x.device != self.device:
            raise ValueError(f"the rows are on {x.device} but the autoencoder is on {self.device}; move one of them")

    # ---- the formulas as torch ops ----
    def _forward_torch(self, p, x, train, halves="both"):
        """p: the tensors by key, in x's dtype.  Returns (result, [(batch mean, unbiased variance)] of
        the BatchNorms in train mode): the unit latent for halves == "encoder", else the reconstruction."""
        stats = []
        h = x
        for i in range(self.n_enc):
            if i:
                bn = _bn_key(i)
                if train:
                    mean, var = h.mean(dim=0), h.var(dim=0, unbiased=False)
                    stats.append((mean.detach(), (var * (h.shape[0] / (h.shape[0] - 1))).detach()))
                else:
                    mean, var = p[f"{bn}.running_mean"], p[f"{bn}.running_var"]
                h = torch.relu((h - mean) / torch.sqrt(var + BN_EPS) * p[f"{bn}.weight"] + p[f"{bn}.bias"])
            h = F.linear(h, p[f"{_enc_key(i)}.weight"], p[f"{_enc_key(i)}.bias"])
        h = h / h.norm(dim=-1, keepdim=True)
        if halves == "encoder":
            return h, stats
        for j in range(self.n_dec):
            h = F.linear(torch.relu(h) if j else h, p[f"{_dec_key(j)}.weight"], p[f"{_dec_key(j)}.bias"])
        return h / h.norm(dim=-1, keepdim=True), stats

    def _cast(self, dtype):
        return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in self.sd.items()}

    def _encode_torch(self, x):
        return self._forward_torch(self._cast(x.dtype), x, False, "encoder")[0]

    def _loss_sums_torch(self, x, chunk=4096):
        """(sum over rows and features of (out - x)^2, sum over rows of the cosine), float64."""
        p = self._cast(x.dtype)
        sq = torch.zeros((), dtype=torch.float64, device=x.device)
        cs = torch.zeros((), dtype=torch.float64, device=x.device)
        for r0 in range(0, x.shape[0], chunk):
            xb = x[r0:r0 + chunk]
            out = self._forward_torch(p, xb, False)[0]
            sq += ((out - xb) ** 2).sum(dtype=torch.float64)
            cs += F.cosine_similarity(out, xb, dim=1, eps=COS_EPS).sum(dtype=torch.float64)
        return sq, cs

    # ---- eval mode ----
    @torch.no_grad()
    def encode(self, x):
        """[..., feature_dim] -> [..., latent] unit vectors: Autoencoder.encode under model.eval()."""
        self._check_rows(x)
        x = x.detach()
        flat = x.reshape(-1, self.feature_dim)
        if not self._takes_native(flat):
            return self._encode_torch(flat).reshape(*x.shape[:-1], self.latent_dim)
        flat = flat.contiguous()
        out = torch.empty(flat.shape[0], self.latent_dim, dtype=torch.float32, device=x.device)
        if flat.shape[0]:
            with torch.cuda.device(x.device):
                ws, n = self._workspace(flat.shape[0], False)
                B = _lib.Boundary(x.device)
                _lib.check(_lib.load().lsr_ae_encode(ctypes.byref(self._struct()), flat.shape[0], B.ptr(flat, "rows"),
                                                     B.ptr(out, "out"), B.ptr(ws, "workspace", torch.uint8), n,
                                                     B.stream()), "lsr_ae_encode")
        return out.reshape(*x.shape[:-1], self.latent_dim)

    def decoder(self):
        """The decoder half as language_query's LanguageDecoder, sharing the weights."""
        return LanguageDecoder([self.sd[f"{_dec_key(j)}.weight"] for j in range(self.n_dec)],
                               [self.sd[f"{_dec_key(j)}.bias"] for j in range(self.n_dec)])

    def decode(self, z):
        """[..., latent] -> [..., feature_dim] unit vectors: Autoencoder.decode."""
        return self.decoder().decode(z)

    @torch.no_grad()
    def reconstruction_loss(self, x):
        """rows [N, feature_dim] -> (l2, cos) of the eval-mode reconstruction, float64 tensors on the rows'
        device: l2 the mean over all N * feature_dim elements of (out - x)^2, cos = 1 - the mean cosine
        (train.py:149-167, whose batches of 256 weighted by their length give the same means)."""
        if x.dim() != 2:
            raise ValueError(f"rows must be [N, {self.feature_dim}], got {tuple(x.shape)}")
        self._check_rows(x)
        x = x.detach()
        n = x.shape[0]
        if self._takes_native(x):
            x = x.contiguous()
            sums = torch.empty(2, dtype=torch.float64, device=x.device)
            with torch.cuda.device(x.device):
                ws, nb = self._workspace(n, False)
                B = _lib.Boundary(x.device)
                _lib.check(_lib.load().lsr_ae_eval_loss(ctypes.byref(self._struct()), n, B.ptr(x, "rows"),
                                                        B.ptr(sums, "sums", torch.float64),
                                                        B.ptr(ws, "workspace", torch.uint8), nb, B.stream()),
                           "lsr_ae_eval_loss")
            sq, cs = sums[0], sums[1]
        else:
            sq, cs = self._loss_sums_torch(x)
        return sq / (n * self.feature_dim), 1 - cs / n


class AutoencoderTrainer:
    """torch.optim.Adam(model.parameters(), lr) and the reference's training step on a LanguageAutoencoder,
    whose tensors it updates in place."""

    def __init__(self, ae, lr=1e-4, cos_weight=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.ae, self.lr, self.cos_weight, self.betas, self.eps = ae, float(lr), float(cos_weight), tuple(betas), float(eps)
        self.t = 0
        self.exp_avg = {k: torch.zeros_like(ae.sd[k]) for k in ae.parameter_keys()}
        self.exp_avg_sq = {k: torch.zeros_like(ae.sd[k]) for k in ae.parameter_keys()}
        self._structs = None
        self._ws = {}

    def state_dict(self):
        return {"t": self.t, "exp_avg": dict(self.exp_avg), "exp_avg_sq": dict(self.exp_avg_sq)}

    def load_state_dict(self, state):
        self.t = int(state["t"])
        for name in ("exp_avg", "exp_avg_sq"):
            for k, v in getattr(self, name).items():
                v.copy_(state[name][k])

    def _step_torch(self, x):
        ae, (b1, b2) = self.ae, self.betas
        p = ae._cast(x.dtype)
        keys = ae.parameter_keys()
        with torch.enable_grad():
            leaves = {k: p[k].detach().clone().requires_grad_(True) for k in keys}
            out, stats = ae._forward_torch({**p, **leaves}, x, True)
            l2 = ((out - x) ** 2).mean()
            cos = 1 - F.cosine_similarity(out, x, dim=1, eps=COS_EPS).mean()
            grads = torch.autograd.grad(l2 + cos * self.cos_weight, [leaves[k] for k in keys])
        with torch.no_grad():
            for i, (mean, var) in enumerate(stats, start=1):
                bn = _bn_key(i)
                rm, rv = ae.sd[f"{bn}.running_mean"], ae.sd[f"{bn}.running_var"]
                rm.copy_((1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean.to(rm.dtype))
                rv.copy_((1 - BN_MOMENTUM) * rv + BN_MOMENTUM * var.to(rv.dtype))
                ae.sd[f"{bn}.num_batches_tracked"] += 1
            bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
            for k, g in zip(keys, grads):
                m, v, w = self.exp_avg[k], self.exp_avg_sq[k], ae.sd[k]
                g = g.to(w.dtype)
                m.lerp_(g, 1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                w.addcdiv_(m, (v.sqrt() / math.sqrt(bc2)).add_(self.eps), value=-self.lr / bc1)
        return l2.detach(), cos.detach()

    def _step_native(self, x):
        ae, rows, B = self.ae, x.shape[0], _lib.Boundary(x.device)
        if self._structs is None:
            self._structs = (ae._params_struct(self.exp_avg), ae._params_struct(self.exp_avg_sq))
        if rows not in self._ws:
            self._ws[rows] = ae._workspace(rows, True)
        ws, n = self._ws[rows]
        losses = torch.empty(2, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().lsr_ae_train_step(
                ctypes.byref(ae._struct()), ctypes.byref(self._structs[0]), ctypes.byref(self._structs[1]), rows,
                B.ptr(x, "batch"), self.lr, self.betas[0], self.betas[1], self.eps, self.t, self.cos_weight,
                B.ptr(losses, "losses"), B.ptr(ws, "workspace", torch.uint8), n, B.stream()), "lsr_ae_train_step")
        return losses[0], losses[1]

    def step(self, batch):
        """One step on batch [B, feature_dim] -> (l2, cos) of the batch before the update, 0-d tensors on
        the batch's device (nothing is synchronised)."""
        if batch.dim() != 2:
            raise ValueError(f"the batch must be [B, {self.ae.feature_dim}], got {tuple(batch.shape)}")
        self.ae._check_rows(batch)
        if batch.shape[0] < 2:
            raise ValueError("Expected more than 1 value per channel when training (a batch of one row)")
        x = batch.detach()
        self.t += 1
        if self.ae._takes_native(x) and x.shape[0] <= _lib.AE_MAX_BATCH:
            return self._step_native(x.contiguous())
        return self._step_torch(x)


def fit(ae, rows, num_epochs=100, batch_size=64, lr=1e-4, cos_weight=1e-3, seed=0, eval_from_epoch=91, ckpt_dir=None):
    """The reference's training loop (train.py:113-182) on rows [N, feature_dim], which stay on their device.

    One seeded host randperm per epoch, the last short batch kept.  After every epoch >= eval_from_epoch
    the eval-mode loss l2 + cos (unweighted) over all rows is computed; the state dict of the lowest one
    below 100 is kept, and saved as ckpt_dir/best_ckpt.pth if ckpt_dir is given.  Returns FitResult(best_epoch,
    best_loss, state_dict): 0, 100.0 and None if no epoch was evaluated."""
    if rows.dim() != 2:
        raise ValueError(f"rows must be [N, {ae.feature_dim}], got {tuple(rows.shape)}")
    trainer = AutoencoderTrainer(ae, lr=lr, cos_weight=cos_weight)
    gen = torch.Generator().manual_seed(int(seed))
    n = rows.shape[0]
    best_epoch, best_loss, best_state = 0, 100.0, None
    if ckpt_dir is not None:
        os.makedirs(ckpt_dir, exist_ok=True)
    for epoch in range(num_epochs):
        perm = torch.randperm(n, generator=gen).to(rows.device)
        for s in range(0, n, batch_size):
            trainer.step(rows[perm[s:s + batch_size]])
        if epoch >= eval_from_epoch:
            l2, cos = ae.reconstruction_loss(rows)
            loss = float(l2 + cos)
            if loss < best_loss:
                best_epoch, best_loss = epoch, loss
                best_state = collections.OrderedDict((k, v.detach().clone()) for k, v in ae.sd.items())
                if ckpt_dir is not None:
                    ae.save(os.path.join(ckpt_dir, "best_ckpt.pth"))
    return FitResult(best_epoch, best_loss, best_state)


def load_feature_dir(data_dir):
    """Every *_f.npy table of a language_features directory, in name order -> (rows [N, D] float32 on the
    CPU, {file name without .npy: its row count}) (autoencoder/dataset.py)."""
    paths = sorted(glob.glob(os.path.join(data_dir, "*_f.npy")))
    if not paths:
        raise FileNotFoundError(f"no *_f.npy tables in {data_dir}")
    tables = [np.load(p) for p in paths]
    counts = collections.OrderedDict((os.path.basename(p)[:-4], t.shape[0]) for p, t in zip(paths, tables))
    return torch.from_numpy(np.concatenate(tables, axis=0).astype(np.float32)), counts


def compress_feature_dir(ae, data_dir, out_dir):
    """autoencoder/test.py: the eval-mode latent of every row of every *_f.npy of data_dir, saved under the
    same file name in out_dir, with the *_s.npy segment maps copied beside them.  Returns {name: rows}."""
    paths = sorted(glob.glob(os.path.join(data_dir, "*_f.npy")))
    if not paths:
        raise FileNotFoundError(f"no *_f.npy tables in {data_dir}")
    os.makedirs(out_dir, exist_ok=True)
    for p in sorted(glob.glob(os.path.join(data_dir, "*_s.npy"))):
        shutil.copy(p, os.path.join(out_dir, os.path.basename(p)))
    counts = collections.OrderedDict()
    for p in paths:
        x = torch.from_numpy(np.load(p).astype(np.float32)).to(ae.device)
        np.save(os.path.join(out_dir, os.path.basename(p)), ae.encode(x).float().cpu().numpy())
        counts[os.path.basename(p)[:-4]] = x.shape[0]
    return counts
