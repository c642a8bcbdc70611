"""Language supervision of the 'lang' stages from the files the reference trains on, kept in the form
they are stored in, and the stages' loss computed straight from that form.

The reference's Camera.get_language_feature (scene/cameras.py:69-118) reads, per training view,
`<stem>_s.npy` (segment maps [4, H, W]: one per feature level, -1 where a pixel has no segment) and
`<stem>_f.npy` (the segments' features [S, C]), gathers feature_map[seg] into a dense [C, H, W]
tensor on the host and uploads it every iteration.  Here a view's supervision stays a
SegmentSupervision (an int32 map and the table: a whole training set's fits on the device), and
segment_lang_loss evaluates train.py:287-292's loss from (language image, map, table) in one fused
forward and one fused backward (lsr_seg_loss_views, include/lsr_train.h), the dense ground truth and
the masked copies never built.

    sups = load_all(lf_path, [supervision_stem(cam.colmap_id, "nerfies") for cam in cams], level, "cuda")
    loss = step(cams_of_batch, gts, lang_sup=[sups[i] for i in batch])        # train_step.TrainStep
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np
import torch

COS_EPS = 1e-8           # torch.nn.functional.cosine_similarity's eps (utils/loss_utils.py:26-27)
MAX_NATIVE_VIEWS = 8     # lsr_seg_loss_views' V


class SegmentSupervision:
    """One view's language supervision at one feature level: seg [H, W] int32, table [S, C] float32.
    A pixel is labelled iff 0 <= seg < S; -1 is the files' marker for "no segment"."""

    def __init__(self, seg: torch.Tensor, table: torch.Tensor):
        seg, table = torch.as_tensor(seg), torch.as_tensor(table)
        if seg.dim() != 2 or seg.dtype != torch.int32:
            raise ValueError(f"seg must be [H, W] int32, got {tuple(seg.shape)} {seg.dtype}")
        if table.dim() != 2 or table.dtype != torch.float32 or table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError(f"table must be [S, C] float32 with S, C >= 1, got {tuple(table.shape)} {table.dtype}")
        if seg.device != table.device:
            raise ValueError(f"seg is on {seg.device}, table on {table.device}")
        self.seg, self.table = seg.contiguous(), table.contiguous()

    @property
    def device(self) -> torch.device:
        return self.seg.device

    @property
    def n_seg(self) -> int:
        return int(self.table.shape[0])

    @property
    def channels(self) -> int:
        return int(self.table.shape[1])

    def to(self, device) -> "SegmentSupervision":
        return SegmentSupervision(self.seg.to(device), self.table.to(device))

    def labelled(self) -> torch.Tensor:
        """[H, W] bool: 0 <= seg < S."""
        return (self.seg >= 0) & (self.seg < self.n_seg)

    def dense(self):
        """(gt [C, H, W] float32, mask [1, H, W] bool): what get_language_feature returns for these
        files, bit for bit (unlabelled pixels carry the table's last row, as its feature_map[-1]
        does).  Values outside [-1, S), which the loader refuses, count as unlabelled too."""
        m = self.labelled()
        idx = torch.where(m, self.seg, torch.full_like(self.seg, self.n_seg - 1)).long()
        return self.table[idx].permute(2, 0, 1).contiguous(), m.unsqueeze(0)


def supervision_stem(colmap_id: int, data_type: str, split: str = "train", cam_name: Optional[str] = None):
    """The file stem get_language_feature builds (scene/cameras.py:70-87); None where it returns no
    supervision (dynerf's video split)."""
    if data_type == "nerfies":
        real_id = colmap_id * 4 + 1 if split == "train" else colmap_id * 4 + 3 if split == "test" else colmap_id + 1
        return f"{real_id:06}"
    if data_type == "dynerf":
        if split == "video":
            return None
        if split == "test" and colmap_id >= 300:
            raise ValueError(f"dynerf test views have colmap_id < 300, got {colmap_id}")
        if cam_name is None:
            raise ValueError("dynerf stems need cam_name")
        return f"{cam_name}-{colmap_id % 300:04}"
    raise ValueError(f"data_type {data_type!r}: 'nerfies' or 'dynerf'")


def load_language_supervision(language_feature_dir: str, stem: str, feature_level: int) -> SegmentSupervision:
    """<stem>_s.npy [4, H, W] and <stem>_f.npy [S, C] at feature_level 0..3 (default, s, m, l:
    scene/cameras.py:92-114), on the CPU."""
    if isinstance(feature_level, bool) or not isinstance(feature_level, (int, np.integer)) \
            or not 0 <= feature_level <= 3:
        raise ValueError(f"feature_level must be 0, 1, 2 or 3, got {feature_level!r}")
    base = os.path.join(language_feature_dir, stem)
    seg_map, table = np.load(base + "_s.npy"), np.load(base + "_f.npy")
    if seg_map.ndim != 3 or seg_map.shape[0] <= feature_level:
        raise ValueError(f"{base}_s.npy: expected [4, H, W] segment maps, got shape {seg_map.shape}")
    if table.ndim != 2 or table.shape[0] < 1 or table.shape[1] < 1:
        raise ValueError(f"{base}_f.npy: expected an [S, C] feature table, got shape {table.shape}")
    if not (np.issubdtype(table.dtype, np.floating) or np.issubdtype(table.dtype, np.integer)):
        raise ValueError(f"{base}_f.npy: expected numbers, got {table.dtype}")
    seg = seg_map[feature_level]
    if not np.issubdtype(seg.dtype, np.integer):
        if not np.issubdtype(seg.dtype, np.floating) or not np.all(np.isfinite(seg)) or np.any(seg != np.trunc(seg)):
            raise ValueError(f"{base}_s.npy: level {feature_level} holds values that are not whole numbers")
    S = table.shape[0]
    if seg.size and (seg.max() >= S or seg.min() < -1):
        raise ValueError(f"{base}_s.npy: level {feature_level} holds segment indices in [{seg.min()}, {seg.max()}], "
                         f"outside [-1, {S}) of the {S}-row table")
    return SegmentSupervision(torch.from_numpy(np.ascontiguousarray(seg.astype(np.int32))),
                              torch.from_numpy(np.ascontiguousarray(table.astype(np.float32))))


def load_all(language_feature_dir: str, stems: Sequence[Optional[str]], feature_level: int,
             device="cpu") -> List[Optional[SegmentSupervision]]:
    """One SegmentSupervision per stem on `device` (None for a None stem): a training set's language
    supervision, resident where the loss runs."""
    return [None if s is None else load_language_supervision(language_feature_dir, s, feature_level).to(device)
            for s in stems]


def _fallback(images, sups, lam, beta, addcosloss):
    """The loss as torch ops in the images' dtype (the CPU implementation; in float64 the tests'
    yardstick): train.py:287-292 on a = x m, b = table[seg] m, with every seg outside [0, S) unlabelled."""
    a, b = [], []
    for x, s in zip(images, sups):
        s = s if s.device == x.device else s.to(x.device)
        m = s.labelled()
        t = s.table.to(x.dtype)[torch.where(m, s.seg, torch.zeros_like(s.seg)).long()].permute(2, 0, 1)
        a.append(x * m)
        b.append(t * m)
    a, b = torch.stack(a), torch.stack(b)
    loss = lam * (a - b).abs().mean()
    if addcosloss:
        loss = loss + beta * (1 - torch.nn.functional.cosine_similarity(a, b, dim=-1, eps=COS_EPS).mean())
    return loss


def _views(B, imgs, grads, sups):
    from diff_gaussian_rasterization import _lib
    arr = (_lib.SegView * len(imgs))()
    for v, (x, s) in enumerate(zip(imgs, sups)):
        arr[v].image, arr[v].n_seg = B.ptr(x, f"images[{v}]"), s.n_seg
        arr[v].seg, arr[v].table = B.ptr(s.seg, f"seg {v}", torch.int32), B.ptr(s.table, f"table {v}")
        arr[v].d_image = B.ptr(grads[v], f"grads[{v}]") if grads is not None else None
    return arr


class _SegLoss(torch.autograd.Function):
    """lsr_seg_loss_views / _backward over the views' language images, unstacked: two launches forward,
    one backward; between them only the workspace (the rows' sums, with the cosine term) is kept."""

    @staticmethod
    def forward(ctx, sups, lam, beta, with_cos, *images):
        from diff_gaussian_rasterization import _lib
        L = _lib.load()
        imgs = [x.contiguous() for x in images]
        V, (C, H, W) = len(imgs), imgs[0].shape
        dev = imgs[0].device
        B = _lib.Boundary(dev)
        nbytes = int(L.lsr_seg_loss_workspace_bytes(V, C, H, W))
        if nbytes < 0:
            raise ValueError(L.lsr_last_error().decode())
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.lsr_seg_loss_views(V, C, H, W, _views(B, imgs, None, sups), lam, beta, int(with_cos),
                                            B.ptr(loss, "loss"), B.ptr(ws, "workspace", torch.uint8), B.stream()),
                       "lsr_seg_loss_views")
        ctx.sups, ctx.scalars = sups, (lam, beta, int(with_cos))
        ctx.save_for_backward(ws, *imgs)
        return loss

    @staticmethod
    def backward(ctx, g):
        from diff_gaussian_rasterization import _lib
        ws, *imgs = ctx.saved_tensors
        lam, beta, with_cos = ctx.scalars
        V, (C, H, W) = len(imgs), imgs[0].shape
        dev = imgs[0].device
        grads = [torch.empty_like(x) for x in imgs]
        g = g.to(device=dev, dtype=torch.float32).contiguous()
        B = _lib.Boundary(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().lsr_seg_loss_views_backward(V, C, H, W, _views(B, imgs, grads, ctx.sups), lam, beta,
                                                               with_cos, B.ptr(g, "grad"),
                                                               B.ptr(ws, "workspace", torch.uint8), B.stream()),
                       "lsr_seg_loss_views_backward")
        return (None, None, None, None) + tuple(grads)


def native_eligible(images, sups) -> bool:
    """Whether segment_lang_loss takes the HIP path: 1..8 float32 [C, H, W] images on one CUDA device
    (any strides: they are made contiguous), with int32 maps and float32 tables on that device."""
    x0 = images[0]
    if not (1 <= len(images) <= MAX_NATIVE_VIEWS and x0.is_cuda):
        return False
    from diff_gaussian_rasterization import _lib
    B = _lib.Boundary(x0.device)   # the images are confirmed once _SegLoss has made them contiguous
    return all(x.dtype == torch.float32 and x.device == x0.device and B.ok(s.seg, torch.int32) and B.ok(s.table)
               for x, s in zip(images, sups))


def segment_lang_loss(images: Sequence[torch.Tensor], sups: Sequence[SegmentSupervision], lam: float = 0.2,
                      beta: float = 0.01, addcosloss: bool = False) -> torch.Tensor:
    """lam * l1_loss(lang * mask, gt * mask) (+ beta * cos_loss(...) with addcosloss) of train.py:287-292
    over the views' language images [C, H, W] against their SegmentSupervision, with its gradient
    towards the images.  cos_loss's similarity runs along the width axis (dim = -1 of [V, C, H, W]):
    one per image row and channel, 0 for a row without labelled pixels.

    Native (lsr_seg_loss_views) when native_eligible(); otherwise (CPU, float64, more than 8 views,
    supervision on another device) the same formulas as torch ops in the images' dtype."""
    images, sups = list(images), list(sups)
    if not images or len(images) != len(sups):
        raise ValueError(f"one SegmentSupervision per image: {len(images)} images, {len(sups)} supervisions")
    shape = tuple(images[0].shape)
    for x, s in zip(images, sups):
        if not isinstance(s, SegmentSupervision):
            raise ValueError(f"expected a SegmentSupervision per view, got {type(s).__name__}")
        if x.dim() != 3 or tuple(x.shape) != shape or x.dtype != images[0].dtype or x.device != images[0].device:
            raise ValueError("the views' language images must share one [C, H, W] shape, dtype and device")
        if tuple(s.seg.shape) != shape[1:] or s.channels != shape[0]:
            raise ValueError(f"supervision of a {tuple(s.seg.shape)} map with {s.channels} channels "
                             f"for a {shape} image")
    if native_eligible(images, sups):
        return _SegLoss.apply(tuple(sups), float(lam), float(beta), bool(addcosloss), *images)
    return _fallback(images, sups, lam, beta, addcosloss)
