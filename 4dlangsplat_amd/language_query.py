"""Open-vocabulary query on the MI355X: the reference's eval/eval.py decode + relevancy step.

What the reference does per frame (eval/eval.py:604-616, eval/openclip_encoder.py:41-56, 96-112):
    restored = model.decode(sem_feat.flatten(0, 2))            # [L*H*W, 512] unit vectors
    relev    = clip_model.get_max_across(restored.view(L, H, W, -1))   # [L, n_phrases, H, W]
Here both are one fused kernel per level (include/lsr_query.h, csrc/query.hip): the 512-wide
vector is never written, only n_pos floats per pixel.

    dec = LanguageDecoder.load(ae_ckpt_path).to("cuda")
    rel = relevancy(sem_feat, dec, pos_embeds, neg_embeds)                 # [L, H, W, C] -> [L, n_pos, H, W]
    rel = relevancy(render_pkg["language_feature_image"], dec, pos, neg, layout="chw")   # no host round trip

    seg = segment(rel, gt_masks)        # masks, level scores, chosen level and IoU per phrase (activate_stream)

    rgb = pca_image(render_pkg["language_feature_image"])          # [H, W, 3] in [0, 1]: render.py's pca_compress
    pca = LanguagePCA().fit(frames)                                # one basis and one range for a whole sequence
    rgb8 = pca.transform(frame, out="uint8")

The embeddings are used as given (the reference normalises them in set_positives); there is no
text encoder here.

The native path takes float32 CUDA tensors on one device and decoders inside the library's limits;
everything else (CPU, float64, odd widths) runs the same formulas as torch ops in the input's
dtype.  That fallback is the CPU implementation, and in float64 the yardstick of the tests.
"""
from __future__ import annotations

import collections
import collections.abc
import ctypes
import glob
import os
import re

import numpy as np
import torch

from diff_gaussian_rasterization import _lib

__all__ = ["LanguageDecoder", "relevancy", "query_frames", "Segmentation", "segment", "segment_frames", "pca_image",
           "LanguagePCA"]


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
        B = _lib.Boundary(self.device)
        return (len(self.weights) <= _lib.QUERY_MAX_LAYERS and 1 <= d[0] <= _lib.QUERY_MAX_INPUT
                and all(x % 16 == 0 and 16 <= x <= _lib.QUERY_MAX_WIDTH for x in d[1:])
                and self.device.type == "cuda" and all(B.ok(t) for t in self.weights + self.biases))

    def _struct(self):
        s, B = _lib.Decoder(), _lib.Boundary(self.device)
        s.n_layers = len(self.weights)
        for i, x in enumerate(self.dims):
            s.dims[i] = x
        for i, (w, b) in enumerate(zip(self.weights, self.biases)):
            s.weight[i] = B.ptr(w, f"decoder weight {i}")
            s.bias[i] = B.ptr(b, f"decoder bias {i}")
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
                dec, B = self._struct(), _lib.Boundary(x.device)
                _lib.check(_lib.load().lsr_query_decode(ctypes.byref(dec), flat.shape[0], B.ptr(flat, "latent"),
                                                        self.c_in, 1, B.ptr(out, "out"), B.stream()), "lsr_query_decode")
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
            lib, dec, B = _lib.load(), decoder._struct(), _lib.Boundary(latent.device)
            chunk = _lib.QUERY_MAX_PHRASES - n_neg            # positives of one launch
            with torch.cuda.device(latent.device):
                stream = B.stream()
                for l in range(L):
                    x = levels[l]
                    if H > 1 and W > 1 and x.stride(0) != W * x.stride(1):   # the pixels must share one stride
                        x = x.contiguous()
                    pix_stride = x.stride(1) if W > 1 else x.stride(0)
                    for p0 in range(0, n_pos, chunk):
                        n = min(chunk, n_pos - p0)
                        _lib.check(lib.lsr_query_relevancy(ctypes.byref(dec), H * W, B.ptr(x, "latent", strided=True),
                                                           pix_stride, x.stride(2), n, B.ptr(pos[p0:], "pos_embeds"),
                                                           n_neg, B.ptr(neg, "neg_embeds"), float(scale),
                                                           B.ptr(out[l, p0:], "out"), stream), "lsr_query_relevancy")
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


Segmentation = collections.namedtuple(
    "Segmentation", ["blended", "mask_raw", "mask", "score", "level", "chosen_mask", "inter", "union", "iou",
                     "chosen_iou"], defaults=[None, None, None, None])
Segmentation.__doc__ = """What segment() returns.  For rel [L, n_pos, H, W]: blended float, mask_raw and mask
bool, all [L, n_pos, H, W]; score [L, n_pos]; level [n_pos] int64, the level with the greatest score;
chosen_mask [n_pos, H, W], mask at that level.  With annotations also inter, union (int64) and iou
[L, n_pos] and chosen_iou [n_pos]; None without.  For rel [n_pos, H, W] the L axis is dropped."""


def _segment_torch(v, gt, thresh, scale, strategy):
    """activate_stream's lines (eval/eval.py:172-276) and smooth_cuda on [M, H, W] maps as torch ops in
    v's dtype.  gt: [G, H, W] bool or None, map m uses gt[m % G]."""
    F = torch.nn.functional
    M = v.shape[0]
    per_map = lambda x: x.reshape(M, -1)
    a = F.avg_pool2d(v[:, None], scale, 1, scale // 2, count_include_pad=False)[:, 0]
    b = 0.5 * (a + v)
    o = b - per_map(b).min(dim=1).values[:, None, None]
    o = o / (per_map(o).max(dim=1).values[:, None, None] + 1e-9)
    o = o * 2.0 + (-1.0)
    o = torch.clip(o, 0, 1)
    raw = o > thresh
    # smooth_cuda: AvgPool2d(7, 1, 3, count_include_pad=False)(raw) > 0.5 as the integer test 2 ones > valid
    ones = F.avg_pool2d(raw.to(v.dtype)[:, None], 7, 1, 3, divisor_override=1)[:, 0]
    valid = F.avg_pool2d(torch.ones_like(v[:1])[:, None], 7, 1, 3, divisor_override=1)[:, 0]
    mask = 2 * ones > valid
    if strategy == "point":
        score = per_map(b).max(dim=1).values
    else:                                              # the mean of b over raw, summed in double; 0 where raw is empty
        cnt = per_map(raw).sum(dim=1)
        tot = per_map(torch.where(raw, b.double(), torch.zeros((), dtype=torch.float64, device=v.device))).sum(dim=1)
        score = torch.where(cnt > 0, tot / cnt.clamp(min=1), torch.zeros_like(tot)).to(v.dtype)
    inter = union = None
    if gt is not None:
        g = gt[torch.arange(M, device=v.device) % gt.shape[0]]
        inter = per_map(g & mask).sum(dim=1)
        union = per_map(g | mask).sum(dim=1)
    return b, raw, mask, score, inter, union


@torch.no_grad()
def segment(rel, gt_masks=None, thresh=0.4, scale=29, strategy="point"):
    """Relevancy maps to masks, level scores and IoU (eval/eval.py activate_stream with smooth_cuda; the
    contract is spelled out in include/lsr_segment.h).  rel: [L, n_pos, H, W] or [n_pos, H, W], not
    modified.  gt_masks: [n_pos, H, W] bool or uint8 (non-zero is inside), or None.  thresh is
    --mask_tresh, scale the smoothing window (odd, 1 ... 63), strategy "point" (score = max of the
    blended map) or "mean" (its mean over mask_raw, 0 where that is empty).  Returns a Segmentation."""
    if rel.dim() not in (3, 4):
        raise ValueError(f"rel must be [L, n_pos, H, W] or [n_pos, H, W], got {tuple(rel.shape)}")
    if not rel.dtype.is_floating_point:
        raise ValueError(f"rel must be a floating-point tensor, got {rel.dtype}")
    if int(scale) != scale or scale % 2 == 0 or not 1 <= scale <= _lib.SEGMENT_MAX_SCALE:
        raise ValueError(f"scale must be odd and in 1 ... {_lib.SEGMENT_MAX_SCALE}, got scale = {scale}")
    if strategy not in _lib.SEGMENT_STRATEGIES:
        raise ValueError(f'strategy must be "point" or "mean", got {strategy!r}')
    scale = int(scale)
    levels = rel.detach() if rel.dim() == 4 else rel.detach()[None]
    L, n_pos, H, W = levels.shape
    if L < 1:
        raise ValueError(f"rel has no levels: {tuple(rel.shape)}")
    if not (1 <= H <= _lib.SEGMENT_MAX_SIDE and 1 <= W <= _lib.SEGMENT_MAX_SIDE):
        raise ValueError(f"rel's H and W must be in 1 ... {_lib.SEGMENT_MAX_SIDE}, got {tuple(rel.shape)}")
    gt = None
    if gt_masks is not None:
        if tuple(gt_masks.shape) != (n_pos, H, W):
            raise ValueError(f"gt_masks must be [n_pos, H, W] = {(n_pos, H, W)} to go with rel "
                             f"{tuple(rel.shape)}, got {tuple(gt_masks.shape)}")
        if gt_masks.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"gt_masks must be bool or uint8, got {gt_masks.dtype}")
        if gt_masks.device != rel.device:
            raise ValueError(f"gt_masks is on {gt_masks.device} but rel is on {rel.device}")
        gt = gt_masks.detach().contiguous()
    M = L * n_pos
    maps = levels.reshape(M, H, W).contiguous()
    native = rel.dtype == torch.float32 and rel.device.type == "cuda"
    if not native or M == 0:
        b, raw, mask, score, inter, union = _segment_torch(maps, None if gt is None else gt != 0, float(thresh), scale,
                                                           strategy)
    else:
        dev = rel.device
        lib = _lib.load()
        ws_bytes = lib.lsr_segment_workspace_bytes(M, H, W)
        if ws_bytes < 0:
            _lib.check(1, "lsr_segment_workspace_bytes")
        b = torch.empty(M, H, W, dtype=torch.float32, device=dev)
        raw8 = torch.empty(M, H, W, dtype=torch.uint8, device=dev)
        mask8 = torch.empty(M, H, W, dtype=torch.uint8, device=dev)
        score = torch.empty(M, dtype=torch.float32, device=dev)
        inter = union = None
        gt8 = None
        if gt is not None:
            gt8 = gt.view(torch.uint8) if gt.dtype == torch.bool else gt
            inter = torch.empty(M, dtype=torch.int64, device=dev)
            union = torch.empty(M, dtype=torch.int64, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        B, u8, i64 = _lib.Boundary(dev), torch.uint8, torch.int64
        with torch.cuda.device(dev):
            _lib.check(lib.lsr_segment(M, H, W, B.ptr(maps, "rel"), scale, float(thresh),
                                       _lib.SEGMENT_STRATEGIES[strategy], B.opt(gt8, "gt_masks", u8), n_pos,
                                       B.ptr(b, "blended"), B.ptr(raw8, "mask_raw", u8), B.ptr(mask8, "mask", u8),
                                       B.ptr(score, "score"), B.opt(inter, "inter", i64), B.opt(union, "union", i64),
                                       B.ptr(ws, "workspace", u8), B.stream()), "lsr_segment")
        raw, mask = raw8.view(torch.bool), mask8.view(torch.bool)
    shape = (L, n_pos)
    b, raw, mask, score = b.reshape(*shape, H, W), raw.reshape(*shape, H, W), mask.reshape(*shape, H, W), score.reshape(shape)
    level = torch.argmax(score, dim=0)                 # the lowest index wins ties, NaN counts as greatest
    pick = torch.arange(n_pos, device=rel.device)
    chosen_mask = mask[level, pick]
    iou = chosen_iou = None
    if gt is not None:
        inter, union = inter.reshape(shape), union.reshape(shape)
        iou = inter.to(rel.dtype) / union.to(rel.dtype)                    # 0 / 0 is NaN, as in the reference
        chosen_iou = iou[level, pick]
    if rel.dim() == 3:
        b, raw, mask, score = b[0], raw[0], mask[0], score[0]
        if gt is not None:
            inter, union, iou = inter[0], union[0], iou[0]
    return Segmentation(b, raw, mask, score, level, chosen_mask, inter, union, iou, chosen_iou)


def segment_frames(level_dirs, decoder, pos_embeds, neg_embeds, out_dir, gt=None, **segment_kwargs):
    """Segment every rendered frame: reads renders_npy/{idx:05d}.npy from each level's folder as
    query_frames does (with its rescale="auto"), runs relevancy() and segment() on the decoder's
    device, and writes out_dir/mask_npy/{idx:05d}.npy: the chosen masks, [n_pos, H, W] uint8.
    gt: a mapping from frame name ("00007" or "00007.npy") to [n_pos, H, W] annotations (array or
    tensor); frames without an entry are segmented but not scored.  Returns a dict: "paths", and with
    gt also "table" {frame name: [(iou, level, scores [L]) per phrase]}, "phrase_iou" (each phrase's
    mean over its frames) and "mean_iou" (their mean), as eval/eval.py:667-690 tabulates them."""
    level_dirs = list(level_dirs)
    if not level_dirs:
        raise ValueError("no level folders given")
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(level_dirs[0], "renders_npy", "*.npy")))
    if not names:
        raise FileNotFoundError(f"no renders_npy/*.npy under {level_dirs[0]}")
    dst = os.path.join(out_dir, "mask_npy")
    os.makedirs(dst, exist_ok=True)
    dev = decoder.device
    pos, neg = pos_embeds.to(dev), neg_embeds.to(dev)
    out = {"paths": []}
    table = {}
    for name in names:
        frame = np.stack([np.load(os.path.join(d, "renders_npy", name)) for d in level_dirs])
        x = torch.from_numpy(frame).float().to(dev)
        if x.min() > 0:                                # eval/eval.py:604-605
            x = x * 2.0 - 1
        rel = relevancy(x, decoder, pos, neg, layout="hwc")
        ann = None
        if gt is not None:
            ann = gt.get(name, gt.get(os.path.splitext(name)[0]))
        if ann is not None:
            ann = torch.as_tensor(ann)
            ann = (ann if ann.dtype in (torch.bool, torch.uint8) else ann != 0).to(dev)
        seg = segment(rel, ann, **segment_kwargs)
        path = os.path.join(dst, name)
        np.save(path, seg.chosen_mask.to(torch.uint8).cpu().numpy())
        out["paths"].append(path)
        if ann is not None:
            iou, level, scores = seg.chosen_iou.cpu(), seg.level.cpu(), seg.score.cpu()
            table[os.path.splitext(name)[0]] = [(float(iou[k]), int(level[k]), scores[:, k].tolist())
                                                for k in range(iou.shape[0])]
    if gt is not None:
        out["table"] = table
        n_pos = pos.shape[0]
        rows = list(table.values())
        out["phrase_iou"] = [sum(r[k][0] for r in rows) / len(rows) if rows else float("nan") for k in range(n_pos)]
        out["mean_iou"] = sum(out["phrase_iou"]) / n_pos
    return out


# ---- PCA colouring of language images (include/lsr_pca.h, csrc/pca.hip) --------------------------------
def _pca_frame(frame, layout):
    """The checks of the native PCA path: returns (C, H, W, pix_stride, chan_stride) of a frame the
    library can address as frame[pixel * pix_stride + channel * chan_stride], or raises ValueError."""
    if layout not in ("hwc", "chw"):
        raise ValueError('layout must be "hwc" or "chw"')
    if not isinstance(frame, torch.Tensor) or frame.dim() != 3:
        raise ValueError("a frame must be a 3-dimensional tensor ([C, H, W] or [H, W, C]), got "
                         f"{tuple(frame.shape) if isinstance(frame, torch.Tensor) else type(frame).__name__}")
    if frame.dtype != torch.float32:
        raise ValueError(f"the native PCA takes float32 frames, got {frame.dtype}")
    if layout == "chw":
        (C, H, W), (sc, sh, sw) = frame.shape, frame.stride()
    else:
        (H, W, C), (sh, sw, sc) = frame.shape, frame.stride()
    if not _lib.PCA_MIN_CHANNELS <= C <= _lib.PCA_MAX_CHANNELS:
        raise ValueError(f"the native PCA takes {_lib.PCA_MIN_CHANNELS} ... {_lib.PCA_MAX_CHANNELS} channels, the frame "
                         f"has C = {C} (layout {layout!r}, shape {tuple(frame.shape)}); an image of three channels or "
                         "fewer needs no PCA")
    if H > 1 and W > 1 and sh != W * sw:
        raise ValueError(f"the frame's pixels do not share one stride (row stride {sh}, column stride {sw}, W = {W}): "
                         "two strides cannot describe it; pass frame.contiguous()")
    if frame.device.type != "cuda":
        raise ValueError(f"the native PCA runs on the GPU: the frame is on {frame.device} (a CPU tensor has no device "
                         "pointer to hand to the kernels); move it with .cuda()")
    return C, H, W, (sw if W > 1 else sh), sc


class LanguagePCA:
    """A three-component PCA of language images that stays on the device: fit() takes the mean, the
    covariance and the value range over one frame or a whole sequence, transform() colours a frame
    with them.  One basis for a sequence keeps the colours of a video steady, where a per-frame fit
    (the reference's pca_compress, and pca_image here) lets axes swap and flip between frames.

    After fit(): mean [C], components [3, C] (sklearn's sign rule), explained_variance [3], range [2]
    (min and max of the projections over every fitted frame), float32 tensors on the frames' device;
    n_samples the pixel count.  Frames are float32 CUDA tensors of 4 ... 32 channels, [C, H, W]
    (layout "chw") or [H, W, C] ("hwc"); anything else is a ValueError."""

    def __init__(self):
        self.mean = self.components = self.explained_variance = self.range = None
        self.n_channels = self.n_samples = None

    def fit(self, frames, layout="chw"):
        """frames: a sequence (or any re-iterable) of same-C frames.  It is walked three times (sums, centred
        Gram, range) and a frame is only held while its sweep is enqueued, so an object whose __iter__
        computes each frame afresh keeps one temporary alive at a time.  A one-shot iterator (a generator)
        is put into a list first, which holds every frame for the length of the fit."""
        self._fit(frames, layout)
        return self

    @torch.no_grad()
    def _fit(self, frames, layout, keep_y=False):
        """The sweeps of fit(); keep_y: return the projections [n_pix, 3] of the last frame."""
        if isinstance(frames, collections.abc.Iterator):      # one shot: it cannot be walked again
            frames = list(frames)
        lib = _lib.load()
        C = dev = ws = sums = gram = B = None
        count = total = 0

        def sweeps():
            """(index, frame pointer, geometry, n_pix, workspace pointer) of every frame, checked against the first."""
            nonlocal ws
            for i, f in enumerate(frames):
                g = _pca_frame(f, layout)
                if C is not None and (g[0] != C or f.device != dev):
                    raise ValueError(f"the frames of one fit share the channel count and the device: got C = {g[0]} "
                                     f"on {f.device} after C = {C} on {dev}")
                n = g[1] * g[2]
                need = lib.lsr_pca_workspace_bytes(g[0], n)
                if ws is None or ws.numel() < need:
                    ws = torch.empty(need, dtype=torch.uint8, device=f.device)
                Bf = B or _lib.Boundary(f.device)
                yield i, Bf.ptr(f.detach(), f"frame {i}", strided=True), g, n, Bf.ptr(ws, "workspace", torch.uint8)

        first, f64 = True, torch.float64
        for i, f, g, n, wp in sweeps():
            if C is None:
                C, dev = g[0], ws.device
                B = _lib.Boundary(dev)
                acc = torch.empty(_lib.PCA_MAX_CHANNELS * (_lib.PCA_MAX_CHANNELS + 1), dtype=torch.float64, device=dev)
                sums, gram = acc[:_lib.PCA_MAX_CHANNELS], acc[_lib.PCA_MAX_CHANNELS:]
            count, total = i + 1, total + n
            if n:                                             # an empty frame launches nothing
                with torch.cuda.device(dev):
                    _lib.check(lib.lsr_pca_sums(C, n, f, g[3], g[4], int(first), B.ptr(sums, "sums", f64), wp, B.stream()),
                               "lsr_pca_sums")
                first = False
        if not count:
            raise ValueError("fit() needs at least one frame")
        if total < 2:
            raise ValueError(f"a covariance needs at least two pixels, the frames have {total}")
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        comps = torch.empty(3, C, dtype=torch.float32, device=dev)
        evals = torch.empty(3, dtype=torch.float32, device=dev)
        rng = torch.empty(2, dtype=torch.float32, device=dev)
        y = None
        with torch.cuda.device(dev):
            stream = B.stream()
            first, seen = True, 0
            for i, f, g, n, wp in sweeps():
                seen += n
                if n:
                    _lib.check(lib.lsr_pca_gram(C, n, f, g[3], g[4], B.ptr(sums, "sums", f64), total, int(first),
                                                B.ptr(gram, "gram", f64), wp, stream), "lsr_pca_gram")
                    first = False
            if seen != total:
                raise ValueError(f"the frames changed between two walks of fit(): {total} pixels, then {seen}")
            _lib.check(lib.lsr_pca_basis(C, total, B.ptr(sums, "sums", f64), B.ptr(gram, "gram", f64),
                                         B.ptr(mean, "mean"), B.ptr(comps, "components"), B.ptr(evals, "variance"),
                                         stream), "lsr_pca_basis")
            first = True
            for i, f, g, n, wp in sweeps():
                if not n:
                    continue
                last = keep_y and i == count - 1
                if last:
                    y = torch.empty(n, 3, dtype=torch.float32, device=dev)
                _lib.check(lib.lsr_pca_project(C, n, f, g[3], g[4], B.ptr(mean, "mean"), B.ptr(comps, "components"),
                                               int(first), B.ptr(y, "y") if last else None, B.ptr(rng, "range"), wp,
                                               stream), "lsr_pca_project")
                first = False
        self.mean, self.components, self.explained_variance, self.range = mean, comps, evals, rng
        self.n_channels, self.n_samples = C, total
        return y

    def _colorize(self, y, H, W, out):
        dev = y.device
        img = torch.empty(H, W, 3, dtype=torch.uint8 if out == "uint8" else torch.float32, device=dev)
        lib = _lib.load()
        fn, what = ((lib.lsr_pca_colorize_u8, "lsr_pca_colorize_u8") if out == "uint8"
                    else (lib.lsr_pca_colorize_f32, "lsr_pca_colorize_f32"))
        B = _lib.Boundary(dev)
        with torch.cuda.device(dev):
            _lib.check(fn(H * W, B.ptr(y, "y"), B.ptr(self.range, "range"), B.ptr(img, "image", img.dtype), B.stream()),
                       what)
        return img

    @torch.no_grad()
    def transform(self, frame, layout="chw", out="float"):
        """The frame coloured with the fitted basis and range: [H, W, 3] float32 in [0, 1] (values outside
        the fitted range are clipped), or uint8 by floor(255 x) with out="uint8", on the frame's device."""
        if out not in ("float", "uint8"):
            raise ValueError('out must be "float" or "uint8"')
        if self.components is None:
            raise ValueError("transform() before fit(): there is no basis yet")
        C, H, W, ps, cs = _pca_frame(frame, layout)
        if C != self.n_channels or frame.device != self.mean.device:
            raise ValueError(f"the frame has C = {C} on {frame.device}, the basis was fitted for C = {self.n_channels} "
                             f"on {self.mean.device}")
        dev, n = frame.device, H * W
        y = torch.empty(n, 3, dtype=torch.float32, device=dev)
        if n:                                                 # y alone: no range is taken, so no workspace either
            B = _lib.Boundary(dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.load().lsr_pca_project(C, n, B.ptr(frame.detach(), "frame", strided=True), ps, cs,
                                                       B.ptr(self.mean, "mean"), B.ptr(self.components, "components"),
                                                       0, B.ptr(y, "y"), None, None, B.stream()), "lsr_pca_project")
        return self._colorize(y, H, W, out)


def pca_image(frame, layout="chw", out="float"):
    """gaussian_scene.pca_compress without the host trip: [C, H, W] (or [H, W, C] with layout "hwc")
    -> [H, W, 3] float32 in [0, 1], or uint8 (the reference's to8b of it) with out="uint8", on the
    frame's device.  The same as LanguagePCA().fit([frame]).transform(frame), in three reads of the
    frame.  A constant frame, where the reference divides 0 by 0, gives zeros."""
    if out not in ("float", "uint8"):
        raise ValueError('out must be "float" or "uint8"')
    pca = LanguagePCA()
    y = pca._fit([frame], layout, keep_y=True)
    _, H, W, _, _ = _pca_frame(frame, layout)
    return pca._colorize(y, H, W, out)
