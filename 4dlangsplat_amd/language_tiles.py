"""Language-feature tiles: from a frame and its four label maps to the segment maps and the 224 x 224
crops an image embedder consumes, and from the embeddings to the `<stem>_s.npy` / `<stem>_f.npy` files
that language_autoencoder and language_supervision read.

The reference's preprocess/generate_clip_features.py (sam_encoder, mask2segmap, get_seg_img, pad_img,
create, sava_numpy, with --precompute_seg) takes, per level and label, a full-frame np.where, a
full-frame image copy, a crop, a pad and a cv2.resize on the host.  Here a frame is three native steps
(include/lsr_tiles.h: lsr_tiles_census, lsr_tiles_plan, lsr_tiles_render) with one host read between
them, the levels' tile counts.  SAM and CLIP stay external: the embedder is a callable.

    ft = prepare_frame(image_hw3_uint8, label_maps_4hw_int32, bgr=True)      # FrameTiles
    build_language_features(images, label_map_paths, clip_embed, save_folder, names, bgr=True)

The tile arithmetic is exact integer arithmetic (lsr_tiles.h states it), so the native path, the
torch-ops fallback and a plain numpy loop agree byte for byte.  cv2.resize quantises its bilinear
coefficients to 1/2048, so its bytes can differ from these by one grey level.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

LEVELS = ("default", "s", "m", "l")    # the label maps' order, and the files' (scene/cameras.py:92-114)
SIDE = 224                             # LSR_TILES_SIDE
MAX_NATIVE_LABEL = 1023                # LSR_TILES_MAX_LABEL
_FALLBACK_CHUNK = 16                   # tiles the fallback resizes at once


@dataclass
class FrameTiles:
    """One frame's tiles [n, 3, 224, 224] float32 in [0, 1] (levels default, s, m, l; ascending label
    inside a level), seg_maps [4, H, W] int32 (a pixel's tile index, -1 without one), the levels' tile
    counts lengths [4], and per tile its label [n] and its box [n, 4] = (x, y, w, h), both int32."""
    tiles: torch.Tensor
    seg_maps: torch.Tensor
    lengths: List[int]
    labels: torch.Tensor
    boxes: torch.Tensor


def _check_lengths(lengths):
    for j, n in enumerate(lengths):
        if n == 0:
            raise ValueError(f"level {j} ('{LEVELS[j]}') has no label with pixels and a bounding box of non-zero "
                             "width and height: the frame has no tiles at that level")


# ---- the formulas as torch ops: the CPU implementation and the fallback -----------------------------

def _census_torch(label_maps):
    """Per level the kept labels in ascending order: (seg_maps, lengths, levels, labels, boxes), the
    last three per tile as int64."""
    L, H, W = label_maps.shape
    dev = label_maps.device
    seg = torch.full((L, H, W), -1, dtype=torch.int32, device=dev)
    lengths, levels, labels, boxes = [], [], [], []
    base = 0
    for j in range(L):
        lab = label_maps[j].long()
        ys, xs = torch.nonzero(lab >= 1, as_tuple=True)
        ids, inv = torch.unique(lab[ys, xs], sorted=True, return_inverse=True)
        K = ids.numel()
        lo = lambda v, big: torch.full((K,), big, dtype=torch.int64, device=dev).scatter_reduce(0, inv, v, "amin")
        hi = lambda v: torch.full((K,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, inv, v, "amax")
        x, y = lo(xs, W), lo(ys, H)
        w, h = hi(xs) - x, hi(ys) - y
        keep = (w != 0) & (h != 0)
        rank = torch.where(keep, torch.cumsum(keep, 0) - 1 + base, torch.full_like(x, -1))
        seg[j][ys, xs] = rank[inv].to(torch.int32)
        n = int(keep.sum())
        lengths.append(n)
        levels.append(torch.full((n,), j, dtype=torch.int64, device=dev))
        labels.append(ids[keep])
        boxes.append(torch.stack([x, y, w, h], 1)[keep])
        base += n
    return seg, lengths, torch.cat(levels), torch.cat(labels), torch.cat(boxes)


def _taps(l):
    """lsr_tiles.h's resize taps of sides l [n]: (s, s1, a), each [n, 224] int64."""
    d = torch.arange(SIDE, device=l.device)
    t = ((2 * d + 1)[None, :] * l[:, None] - SIDE).clamp(min=0)       # t < 0: s = 0, a = 0
    s = torch.div(t, 2 * SIDE, rounding_mode="floor")
    a = t - s * (2 * SIDE)
    last = (l - 1)[:, None]
    edge = s >= last
    s, a = torch.where(edge, last, s), torch.where(edge, torch.zeros_like(a), a)
    return s, torch.minimum(s + 1, last), a


def _tiles_torch(image, label_maps, levels, labels, boxes):
    """tiles [n, 3, 224, 224] float32 of the descriptors, in chunks."""
    L, H, W = label_maps.shape
    flat_lab = label_maps.reshape(-1).long()
    flat_img = image.reshape(-1, 3).to(torch.int32)
    out = torch.empty((labels.numel(), 3, SIDE, SIDE), dtype=torch.float32, device=image.device)
    for c0 in range(0, labels.numel(), _FALLBACK_CHUNK):
        sl = slice(c0, c0 + _FALLBACK_CHUNK)
        x, y, w, h = (boxes[sl, k] for k in range(4))
        l = torch.maximum(w, h)
        tall = h > w
        ox = torch.where(tall, torch.div(h - w, 2, rounding_mode="floor"), torch.zeros_like(w))
        oy = torch.where(tall, torch.zeros_like(w), torch.div(w - h, 2, rounding_mode="floor"))
        s0, s1, a = _taps(l)
        col = lambda v: v[:, None, None]
        S = torch.zeros((l.numel(), SIDE, SIDE, 3), dtype=torch.int32, device=image.device)
        for py, wy in ((s0, 2 * SIDE - a), (s1, a)):
            cy, wy = py[:, :, None] - col(oy), wy[:, :, None]
            for px, wx in ((s0, 2 * SIDE - a), (s1, a)):
                cx, wx = px[:, None, :] - col(ox), wx[:, None, :]
                inside = (cy >= 0) & (cy < col(h)) & (cx >= 0) & (cx < col(w))
                at = (col(y) + cy).clamp(0, H - 1) * W + (col(x) + cx).clamp(0, W - 1)
                hit = inside & (flat_lab[col(levels[sl]) * (H * W) + at] == col(labels[sl]))
                S += ((wy * wx) * hit).to(torch.int32)[..., None] * flat_img[at]
        byte = torch.div(S + 2 * SIDE * SIDE, 4 * SIDE * SIDE, rounding_mode="floor")
        out[sl] = byte.permute(0, 3, 1, 2).to(torch.float32) / 255.0
    return out


def _prepare_torch(image, label_maps):
    seg, lengths, levels, labels, boxes = _census_torch(label_maps)
    _check_lengths(lengths)
    tiles = _tiles_torch(image, label_maps, levels, labels, boxes)
    return FrameTiles(tiles, seg, lengths, labels.to(torch.int32), boxes.to(torch.int32))


# ---- the native path --------------------------------------------------------------------------------

def native_eligible(image, label_maps) -> bool:
    """Whether prepare_frame tries the HIP path: a uint8 image and int32 label maps on one CUDA device.
    (Labels above 1023 are found by the census itself, which then hands the frame to the fallback.)"""
    if not image.is_cuda:
        return False
    from diff_gaussian_rasterization import _lib
    B = _lib.Boundary(image.device)   # any strides: _prepare_native makes both contiguous, then takes their addresses
    return B.ok(image, torch.uint8, strided=True) and B.ok(label_maps, torch.int32, strided=True)


def _prepare_native(image, label_maps) -> Optional[FrameTiles]:
    """None if a label exceeds MAX_NATIVE_LABEL."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    L, H, W = label_maps.shape
    dev = image.device
    B, u8, i32 = _lib.Boundary(dev), torch.uint8, torch.int32
    image, label_maps = image.contiguous(), label_maps.contiguous()
    nbytes = int(lib.lsr_tiles_workspace_size(L))
    if nbytes < 0:
        raise ValueError(lib.lsr_last_error().decode())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    desc = torch.empty((_lib.TILES_MAX_TILES, _lib.TILES_DESC_INTS), dtype=torch.int32, device=dev)
    counts = torch.zeros(_lib.TILES_COUNTS, dtype=torch.int32, pin_memory=True)
    stream = torch.cuda.current_stream(dev)
    st, maps, wp = B.stream(stream), B.ptr(label_maps, "label_maps", i32), B.ptr(ws, "workspace", u8)
    with torch.cuda.device(dev):
        _lib.check(lib.lsr_tiles_census(L, H, W, maps, nbytes, wp, st), "lsr_tiles_census")
        _lib.check(lib.lsr_tiles_plan(L, H, W, nbytes, wp, B.ptr(desc, "desc", i32),
                                      _lib.HOST.ptr(counts, "counts", i32), st), "lsr_tiles_plan")
        stream.synchronize()                                   # the frame's one host read
        got = counts.tolist()
        if got[L]:
            return None
        lengths = got[:L]
        _check_lengths(lengths)
        n = sum(lengths)
        seg = torch.empty((L, H, W), dtype=torch.int32, device=dev)
        tiles = torch.empty((n, 3, SIDE, SIDE), dtype=torch.float32, device=dev)
        _lib.check(lib.lsr_tiles_render(L, H, W, maps, B.ptr(image, "image", u8), nbytes, wp, B.ptr(desc, "desc", i32),
                                        (ctypes.c_int32 * L)(*lengths), n, B.ptr(seg, "seg", i32),
                                        B.ptr(tiles, "tiles"), st), "lsr_tiles_render")
    d = desc[:n]
    return FrameTiles(tiles, seg, lengths, d[:, 1].clone(), d[:, 2:6].clone())


def prepare_frame(image, label_maps, bgr: bool = False) -> FrameTiles:
    """The tiles and segment maps of one frame: image [H, W, 3] (bytes; bgr=True for the channel order
    cv2.imread gives, flipped as the reference's cvtColor does) and label_maps [4, H, W] (whole numbers;
    a label >= 1 is a segment, everything else is background).

    Native (lsr_tiles_*) for a uint8 image and int32 label maps on one CUDA device with every label
    <= 1023; otherwise the same formulas as torch ops on the image's device (the CPU implementation).
    A level without a kept label raises ValueError naming the level, before any tile is made."""
    image, label_maps = torch.as_tensor(image), torch.as_tensor(label_maps)
    if image.dim() != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"image must be [H, W, 3], got {tuple(image.shape)}")
    if label_maps.dim() != 3 or label_maps.shape[0] != len(LEVELS) or tuple(label_maps.shape[1:]) != tuple(image.shape[:2]):
        raise ValueError(f"label_maps must be [4, H, W] with the image's H and W, got {tuple(label_maps.shape)} "
                         f"for a {tuple(image.shape)} image")
    if bgr:
        image = image.flip(-1)
    if native_eligible(image, label_maps):
        ft = _prepare_native(image, label_maps)
        if ft is not None:
            return ft
    if label_maps.is_floating_point():
        if not bool(torch.all(label_maps == torch.trunc(label_maps))):
            raise ValueError("label_maps holds values that are not whole numbers")
    return _prepare_torch(image.to(torch.uint8), label_maps.to(device=image.device, dtype=torch.int64))


# ---- the files --------------------------------------------------------------------------------------

def write_language_features(path_stem: str, seg_maps, features) -> None:
    """<path_stem>_s.npy (float32 [4, H, W]) and <path_stem>_f.npy (float32 [S, D]): sava_numpy's files,
    with its dtypes."""
    as_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    seg, feat = as_np(seg_maps), as_np(features)
    if seg.ndim != 3 or seg.shape[0] != len(LEVELS):
        raise ValueError(f"seg_maps must be [4, H, W], got {seg.shape}")
    if feat.ndim != 2 or feat.shape[0] < 1:
        raise ValueError(f"features must be [S, D] with S >= 1, got {feat.shape}")
    if seg.max() != feat.shape[0] - 1:
        raise ValueError(f"seg_maps index {int(seg.max()) + 1} segments, features has {feat.shape[0]} rows")
    np.save(path_stem + "_s.npy", seg.astype(np.float32))
    np.save(path_stem + "_f.npy", feat.astype(np.float32))


def build_language_features(images: Sequence, label_maps: Sequence, embed: Callable[[torch.Tensor], torch.Tensor],
                            save_folder: str, names: Sequence[str], bgr: bool = False, device=None) -> List[int]:
    """create()'s loop: per frame the tiles, embed(tiles) -> [n, D], every row divided by its norm and
    rounded through float16 (the reference's .half() into its float32 img_embeds), and the two files
    <save_folder>/<name.split('.')[0]>_{s,f}.npy.  label_maps' items are arrays or .npy paths; with
    `device`, images and label maps are moved there first (integer label maps as int32 where that is
    lossless, so a CUDA device takes the native path).  Returns the frames' segment counts."""
    if not (len(images) == len(label_maps) == len(names)):
        raise ValueError(f"{len(images)} images, {len(label_maps)} label maps, {len(names)} names")
    os.makedirs(save_folder, exist_ok=True)
    totals = []
    for img, lab, name in zip(images, label_maps, names):
        if isinstance(lab, (str, os.PathLike)):
            lab = np.load(lab)
        img, lab = torch.as_tensor(img), torch.as_tensor(lab)
        if device is not None:
            if not lab.is_floating_point() and lab.numel() and int(lab.max()) < 2 ** 31 and int(lab.min()) >= -2 ** 31:
                lab = lab.to(torch.int32)
            img, lab = img.to(device), lab.to(device)
        ft = prepare_frame(img, lab, bgr=bgr)
        with torch.no_grad():
            emb = torch.as_tensor(embed(ft.tiles))
        if emb.dim() != 2 or emb.shape[0] != ft.tiles.shape[0]:
            raise ValueError(f"embed returned {tuple(emb.shape)} for {ft.tiles.shape[0]} tiles: expected [n, D]")
        emb = emb.detach().to(torch.float32)
        emb = (emb / emb.norm(dim=-1, keepdim=True)).to(torch.float16).to(torch.float32)
        write_language_features(os.path.join(save_folder, name.split(".")[0]), ft.seg_maps, emb)
        totals.append(sum(ft.lengths))
    return totals
