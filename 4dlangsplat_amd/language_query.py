"""Open-vocabulary query on the MI355X: the reference's eval/eval.py decode + relevancy step.

What the reference does per frame (eval/eval.py:604-616, eval/openclip_encoder.py:41-56, 96-112):
    restored = model.decode(sem_feat.flatten(0, 2))            # [L*H*W, 512] unit vectors
    relev    = clip_model.get_max_across(restored.view(L, H, W, -1))   # [L, n_phrases, H, W]
Here both are one fused kernel per level (include/lsr_query.h, csrc/query.hip): the 512-wide
vector is never written, only n_pos floats per pixel.

    dec = LanguageDecoder.load(ae_ckpt_path).to("cuda")
    rel = relevancy(sem_feat, dec, pos_embeds, neg_embeds)                 # [L, H, W, C] -> [L, n_pos, H, W]
    rel = relevancy(render_pkg["language_feature_image"], dec, pos, neg, layout="chw")   # no host round trip

The embeddings are used as given (the reference normalises them in set_positives); there is no
text encoder here.

The native path takes float32 CUDA tensors on one device and decoders inside the library's limits;
everything else (CPU, float64, odd widths) runs the same formulas as torch ops in the input's
dtype.  That fallback is the CPU implementation, and in float64 the yardstick of the tests.
"""
from __future__ import annotations

import ctypes
import glob
import os
import re

import numpy as np
import torch

from diff_gaussian_rasterization import _lib

__all__ = ["LanguageDecoder", "relevancy", "query_frames"]


class LanguageDecoder:
    """The decoder half of the reference Autoencoder (autoencoder/model.py): Linear layers with a ReLU
    between them and an L2 normalisation at the end."""

    def __init__(self, weights, biases):
        weights, biases = list(weights), list(biases)
        if not weights or len(weights) != len(biases):
            raise ValueError("a decoder needs as many biases as weights, and at least one layer")
        for i, (w, b) in enumerate(zip(weights, biases)):
            if w.dim() != 2:
                raise ValueError(f"decoder layer {i}: weight must be [out, in], got {tuple(w.shape)}")
            if tuple(b.shape) != (w.shape[0],):
                raise ValueError(f"decoder layer {i}: bias {tuple(b.shape)} does not match weight {tuple(w.shape)}")
            if i and w.shape[1] != weights[i - 1].shape[0]:
                raise ValueError(f"decoder layer {i} takes {w.shape[1]} inputs but layer {i - 1} gives "
                                 f"{weights[i - 1].shape[0]}: the layers do not chain")
        self.weights = [w.detach().contiguous() for w in weights]
        self.biases = [b.detach().contiguous() for b in biases]

    @classmethod
    def from_state_dict(cls, sd):
        """From the state dict of the reference Autoencoder (or of its decoder alone): the keys
        decoder.{0,2,4,...}.weight|bias; encoder.* and BatchNorm keys are ignored."""
        found = {}
        for k, v in sd.items():
            m = re.fullmatch(r"(?:module\.)?decoder\.(\d+)\.(weight|bias)", k)
            if m:
                found.setdefault(int(m.group(1)), {})[m.group(2)] = v
        if not found:
            raise KeyError("no decoder.N.weight / decoder.N.bias keys in the state dict")
        idx = sorted(found)
        want = list(range(0, 2 * len(idx), 2))            # Linear at 0, 2, 4, ...: a ReLU sits between them
        if idx != want:
            raise KeyError(f"decoder layers {idx} found, expected {want}: a layer is missing")
        for i in idx:
            for part in ("weight", "bias"):
                if part not in found[i]:
                    raise KeyError(f"decoder.{i}.{part} is missing")
        return cls([found[i]["weight"] for i in idx], [found[i]["bias"] for i in idx])

    @classmethod
    def load(cls, path, map_location="cpu"):
        """torch.load of an ae_ckpt_path file (the Autoencoder's state dict)."""
        return cls.from_state_dict(torch.load(path, map_location=map_location))

    @property
    def dims(self):
        return [self.weights[0].shape[1]] + [w.shape[0] for w in self.weights]

    @property
    def c_in(self):
        return self.weights[0].shape[1]

    @property
    def d_out(self):
        return self.weights[-1].shape[0]

    @property
    def device(self):
        return self.weights[0].device

    def to(self, *args, **kwargs):
        return LanguageDecoder([w.to(*args, **kwargs) for w in self.weights],
                               [b.to(*args, **kwargs) for b in self.biases])

    def native_ok(self):
        """Inside the library's limits (include/lsr_query.h), float32, on one CUDA device."""
        d = self.dims
        ts = self.weights + self.biases
        return (len(self.weights) <= _lib.QUERY_MAX_LAYERS and 1 <= d[0] <= _lib.QUERY_MAX_INPUT
                and all(x % 16 == 0 and 16 <= x <= _lib.QUERY_MAX_WIDTH for x in d[1:])
                and all(t.dtype == torch.float32 and t.device.type == "cuda" and t.device == ts[0].device for t in ts))

    def _struct(self):
        s = _lib.Decoder()
        s.n_layers = len(self.weights)
        for i, x in enumerate(self.dims):
            s.dims[i] = x
        for i, (w, b) in enumerate(zip(self.weights, self.biases)):
            s.weight[i] = w.data_ptr()
            s.bias[i] = b.data_ptr()
        return s

    def _check_input(self, x):
        if x.device != self.device:
            raise ValueError(f"the latent is on {x.device} but the decoder's weights are on {self.device}; "
                             "move one of them (LanguageDecoder.to)")

    def _decode_torch(self, x):
        for i, (w, b) in enumerate(zip(self.weights, self.biases)):
            x = torch.nn.functional.linear(torch.relu(x) if i else x, w.to(x.dtype), b.to(x.dtype))
        return x / x.norm(dim=-1, keepdim=True)

    @torch.no_grad()
    def decode(self, x):
        """[..., c_in] -> [..., d_out] unit vectors, as Autoencoder.decode."""
        if x.shape[-1] != self.c_in:
            raise ValueError(f"the latent has {x.shape[-1]} channels, the decoder takes {self.c_in}")
        self._check_input(x)
        x = x.detach()
        if not (x.dtype == torch.float32 and x.device.type == "cuda" and self.native_ok()):
            return self._decode_torch(x)
        flat = x.reshape(-1, self.c_in).contiguous()
        out = torch.empty(flat.shape[0], self.d_out, dtype=torch.float32, device=x.device)
        if flat.shape[0]:
            with torch.cuda.device(x.device):
                stream = torch.cuda.current_stream(x.device).cuda_stream
                dec = self._struct()
                _lib.check(_lib.load().lsr_query_decode(ctypes.byref(dec), flat.shape[0], flat.data_ptr(), self.c_in, 1,
                                                        out.data_ptr(), stream), "lsr_query_decode")
        return out.reshape(*x.shape[:-1], self.d_out)


def _relevancy_torch(pix, decoder, pos, neg, scale):
    """[N, C] latents -> [n_pos, N]: sigmoid(scale (s_pos - max s_neg)), which is get_max_across's
    minimum over the negatives of the pairwise softmax."""
    f = decoder._decode_torch(pix)
    s = f @ torch.cat([pos, neg]).to(f.dtype).T
    return torch.sigmoid(scale * (s[:, :pos.shape[0]] - s[:, pos.shape[0]:].amax(dim=1, keepdim=True))).T.contiguous()


@torch.no_grad()
def relevancy(latent, decoder, pos_embeds, neg_embeds, layout="hwc", scale=10.0):
    """Relevancy maps of every positive phrase (OpenCLIPNetwork.get_max_across of the decoded
    features).  latent: [H, W, C] or [L, H, W, C] (layout "hwc", the renders_npy files) or
    [C, H, W] / [L, C, H, W] ("chw", render()'s language_feature_image).  Returns [n_pos, H, W] or
    [L, n_pos, H, W]."""
    if layout not in ("hwc", "chw"):
        raise ValueError('layout must be "hwc" or "chw"')
    if latent.dim() not in (3, 4):
        raise ValueError(f"latent must have 3 or 4 dimensions, got {tuple(latent.shape)}")
    if pos_embeds.dim() != 2 or neg_embeds.dim() != 2 or pos_embeds.shape[1] != decoder.d_out \
            or neg_embeds.shape[1] != decoder.d_out or not pos_embeds.shape[0] or not neg_embeds.shape[0]:
        raise ValueError(f"pos_embeds and neg_embeds must be [n >= 1, {decoder.d_out}]")
    latent = latent.detach()
    levels = latent if latent.dim() == 4 else latent[None]
    if layout == "chw":
        levels = levels.permute(0, 2, 3, 1)                   # a view: [L, H, W, C]
    L, H, W, C = levels.shape
    if C != decoder.c_in:
        raise ValueError(f"the latent has {C} channels, the decoder takes {decoder.c_in}")
    decoder._check_input(latent)
    if pos_embeds.device != latent.device or neg_embeds.device != latent.device:
        raise ValueError(f"the embeddings must be on the latent's device ({latent.device})")
    n_pos, n_neg = pos_embeds.shape[0], neg_embeds.shape[0]
    native = (latent.dtype == torch.float32 and latent.device.type == "cuda" and decoder.native_ok()
              and pos_embeds.dtype == torch.float32 and neg_embeds.dtype == torch.float32
              and n_neg < _lib.QUERY_MAX_PHRASES)
    if not native:
        out = torch.stack([_relevancy_torch(levels[l].reshape(H * W, C), decoder, pos_embeds.detach(),
                                            neg_embeds.detach(), scale) for l in range(L)])
    else:
        out = torch.empty(L, n_pos, H * W, dtype=torch.float32, device=latent.device)
        if H * W:
            pos, neg = pos_embeds.detach().contiguous(), neg_embeds.detach().contiguous()
            lib, dec = _lib.load(), decoder._struct()
            chunk = _lib.QUERY_MAX_PHRASES - n_neg            # positives of one launch
            with torch.cuda.device(latent.device):
                stream = torch.cuda.current_stream(latent.device).cuda_stream
                for l in range(L):
                    x = levels[l]
                    if H > 1 and W > 1 and x.stride(0) != W * x.stride(1):   # the pixels must share one stride
                        x = x.contiguous()
                    pix_stride = x.stride(1) if W > 1 else x.stride(0)
                    for p0 in range(0, n_pos, chunk):
                        n = min(chunk, n_pos - p0)
                        _lib.check(lib.lsr_query_relevancy(ctypes.byref(dec), H * W, x.data_ptr(), pix_stride,
                                                           x.stride(2), n, pos[p0:].data_ptr(), n_neg, neg.data_ptr(),
                                                           float(scale), out[l, p0:].data_ptr(), stream),
                                   "lsr_query_relevancy")
    out = out.reshape(L, n_pos, H, W)
    return out if latent.dim() == 4 else out[0]


def query_frames(level_dirs, decoder, pos_embeds, neg_embeds, out_dir, rescale="auto", scale=10.0):
    """Query every rendered frame: reads renders_npy/{idx:05d}.npy ([H, W, C], what render_set wrote)
    from each level's folder, and writes out_dir/relevancy_npy/{idx:05d}.npy as [L, n_pos, H, W]
    float32.  rescale="auto" applies eval/eval.py:604-605: a frame whose minimum over all levels is
    > 0 was saved in (0, 1) and is mapped back by x * 2 - 1; rescale=False leaves every frame as it
    is.  Runs on the decoder's device.  Returns the written paths."""
    if rescale not in ("auto", False):
        raise ValueError('rescale must be "auto" or False')
    level_dirs = list(level_dirs)
    if not level_dirs:
        raise ValueError("no level folders given")
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(level_dirs[0], "renders_npy", "*.npy")))
    if not names:
        raise FileNotFoundError(f"no renders_npy/*.npy under {level_dirs[0]}")
    dst = os.path.join(out_dir, "relevancy_npy")
    os.makedirs(dst, exist_ok=True)
    dev = decoder.device
    pos, neg = pos_embeds.to(dev), neg_embeds.to(dev)
    written = []
    for name in names:
        frame = np.stack([np.load(os.path.join(d, "renders_npy", name)) for d in level_dirs])
        x = torch.from_numpy(frame).float().to(dev)
        if rescale == "auto" and x.min() > 0:
            x = x * 2.0 - 1
        rel = relevancy(x, decoder, pos, neg, layout="hwc", scale=scale)
        path = os.path.join(dst, name)
        np.save(path, rel.float().cpu().numpy())
        written.append(path)
    return written
