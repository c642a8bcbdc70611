"""Time-sensitive query on the MI355X: the reference's video-feature search (eval/eval.py
cal_avg_video_feature :317-327, the smoothing / threshold / vIoU block :712-790 and
evaluate_video_feature :355-402).

What the reference does per frame and video phrase:
    feats = video_model.decode(video_latent[mask == 1])              # [n, 4096] unit vectors
    sim   = cosine_similarity(feats.cpu().numpy(), e5_embedding).mean()
Here the decode, the product with the phrase embedding and the norm are one pass of tiled GEMMs
(include/lsr_video.h, csrc/video_query.hip): the 4096-wide vectors are never written and nothing
crosses to the host but the per-mask means.

    vdec = LanguageDecoder.load(video_ae_ckpt_path).to("cuda")       # 6 -> 32 -> ... -> 4096
    sims, counts = masked_similarity(video_latent, seg.mask_raw[seg.level, pick], vdec, e5_embeddings)
    res = time_sensitive_query(frames, masks, ious, vdec, e5_embedding, gt_intervals, coeffs=[0.1, 0.8, 0.1],
                               clip_scores=clip_scores)
    res["video"]["viou"], res["video"]["accuracy"], res["clip"]["viou"]

The native path takes float32 CUDA tensors on one device and decoders inside the library's limits;
everything else (CPU, float64, other widths) runs the same formulas as torch ops in the input's
dtype, as language_query does.  smooth_similarity, evaluate_frames and the thresholds are plain
Python on a few hundred numbers.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from diff_gaussian_rasterization import _lib

__all__ = ["masked_similarity", "row_cosines", "smooth_similarity", "evaluate_frames", "evaluate_sequence",
           "time_sensitive_query",
           "native_ok", "ROW_TILE"]

ROW_TILE = _lib.VIDEO_ROW_TILE      # rows of one block of the layer kernel (LSR_VIDEO_ROW_TILE)


def native_ok(decoder):
    """The decoder is inside include/lsr_video.h's limits, float32, on one CUDA device."""
    d = decoder.dims
    B = _lib.Boundary(decoder.device)
    return (len(decoder.weights) <= _lib.QUERY_MAX_LAYERS and 1 <= d[0] <= _lib.QUERY_MAX_INPUT
            and all(x % 16 == 0 and 16 <= x <= _lib.VIDEO_MAX_WIDTH for x in d[1:])
            and decoder.device.type == "cuda" and all(B.ok(t) for t in decoder.weights + decoder.biases))


def _unit_queries(queries, d_out):
    """[n, d_out] -> float64 unit vectors (sklearn's cosine_similarity normalises the embedding)."""
    if queries.dim() != 2 or queries.shape[1] != d_out:
        raise ValueError(f"queries must be [n, {d_out}], got {tuple(queries.shape)}")
    q = queries.detach().double()
    return q / q.norm(dim=-1, keepdim=True)


def _cosine_torch(rows, decoder, qn):
    """[N, C] rows, [n_q, d_out] unit queries of the rows' dtype -> [n_q, N]: (y . q) / |y| with y the
    decoder's last layer."""
    y = rows
    for i, (w, b) in enumerate(zip(decoder.weights, decoder.biases)):
        y = torch.nn.functional.linear(torch.relu(y) if i else y, w.to(y.dtype), b.to(y.dtype))
    return ((y @ qn.T) / y.norm(dim=-1, keepdim=True)).T.contiguous()


def _cosine_native(rows, decoder, qn, chunk_rows):
    """The same through lsr_video_cosine, `chunk_rows` rows at a time so the workspace stays bounded."""
    n, n_q, dev = rows.shape[0], qn.shape[0], rows.device
    out = torch.empty(n_q, n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    lib, dec, B = _lib.load(), decoder._struct(), _lib.Boundary(dev)
    step = min(n, chunk_rows)
    ws_bytes = lib.lsr_video_workspace_bytes(ctypes.byref(dec), step)
    if ws_bytes < 0:
        _lib.check(int(-ws_bytes), "lsr_video_workspace_bytes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    part = out if step == n else torch.empty(n_q * step, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = B.stream()
        for r0 in range(0, n, step):
            m = min(step, n - r0)
            _lib.check(lib.lsr_video_cosine(ctypes.byref(dec), m, B.ptr(rows[r0:], "rows"), n_q, B.ptr(qn, "queries"),
                                            B.ptr(part, "out"), B.ptr(ws, "workspace", torch.uint8), ws_bytes, stream),
                       "lsr_video_cosine")
            if part is not out:
                out[:, r0:r0 + m] = part[:n_q * m].view(n_q, m)
    return out


def _takes_native(x, decoder, queries):
    return (x.dtype == torch.float32 and x.device.type == "cuda" and native_ok(decoder)
            and queries.device == x.device)


@torch.no_grad()
def row_cosines(rows, decoder, queries, chunk_rows=8192):
    """[N, c_in] latents, [n_q, d_out] queries -> [n_q, N]: every row's cosine with every query (the
    queries are normalised here in float64).  Native for float32 CUDA rows and 1 <= n_q <= 16."""
    if rows.dim() != 2 or rows.shape[1] != decoder.c_in:
        raise ValueError(f"rows must be [N, {decoder.c_in}], got {tuple(rows.shape)}")
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be >= 1")
    decoder._check_input(rows)
    qn = _unit_queries(queries, decoder.d_out).to(rows.device)
    rows = rows.detach()
    if _takes_native(rows, decoder, queries) and 1 <= qn.shape[0] <= _lib.VIDEO_MAX_QUERIES:
        return _cosine_native(rows.contiguous(), decoder, qn.float().contiguous(), int(chunk_rows))
    return _cosine_torch(rows, decoder, qn.to(rows.dtype))


@torch.no_grad()
def masked_similarity(latent, masks, decoder, queries, layout="hwc", chunk_rows=8192):
    """Mean cosine similarity of the decoded video features under each mask with that mask's query
    (cal_avg_video_feature for K masks of one frame at once).

    latent: [H, W, C] (layout "hwc", the renders_npy files) or [C, H, W] ("chw", render()'s image).
    masks: [K, H, W] bool or integer: only pixels == 1 count, as in the reference.
    queries: [K, d_out], one per mask; normalised here in float64.
    Returns (sims [K], counts [K] int64): sims float32 on the native path and in the latent's dtype on
    the fallback; an empty mask gives NaN and count 0."""
    if layout not in ("hwc", "chw"):
        raise ValueError('layout must be "hwc" or "chw"')
    if latent.dim() != 3:
        raise ValueError(f"latent must be [H, W, C] or [C, H, W], got {tuple(latent.shape)}")
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be >= 1")
    x = latent.detach()
    if layout == "chw":
        x = x.permute(1, 2, 0)                                 # a view: [H, W, C]
    H, W, C = x.shape
    if C != decoder.c_in:
        raise ValueError(f"the latent has {C} channels, the decoder takes {decoder.c_in}")
    decoder._check_input(x)
    if masks.dim() != 3 or tuple(masks.shape[1:]) != (H, W):
        raise ValueError(f"masks must be [K, H, W] = [K, {H}, {W}], got {tuple(masks.shape)}")
    if masks.dtype.is_floating_point or masks.dtype.is_complex:
        raise ValueError(f"masks must be bool or integer, got {masks.dtype}")
    if masks.device != x.device:
        raise ValueError(f"masks is on {masks.device} but the latent is on {x.device}")
    K = masks.shape[0]
    if queries.dim() != 2 or queries.shape[0] != K:
        raise ValueError(f"queries must be [K, d_out] = [{K}, {decoder.d_out}], got {tuple(queries.shape)}")
    if queries.device != x.device:
        raise ValueError(f"queries must be on the latent's device ({x.device})")
    qn = _unit_queries(queries, decoder.d_out)
    inside = masks.detach() == 1
    counts = inside.reshape(K, -1).sum(dim=1)
    if not _takes_native(x, decoder, queries):
        sims = torch.full((K,), float("nan"), dtype=x.dtype, device=x.device)
        q = qn.to(x.dtype)
        for k in range(K):
            rows = x[inside[k]]
            if rows.shape[0]:
                sims[k] = _cosine_torch(rows, decoder, q[k:k + 1])[0].double().mean().to(x.dtype)
        return sims, counts
    sims = torch.full((K,), float("nan"), dtype=torch.float32, device=x.device)
    n = counts.tolist()
    if K == 0 or sum(n) == 0:
        return sims, counts                                    # nothing is launched
    # the distinct queries of the call, in order of first appearance; masks are taken in runs whose
    # queries fit one launch
    q32 = qn.float().contiguous()
    keys = [r.tobytes() for r in q32.cpu().numpy()]
    lib = _lib.load()
    k0 = 0
    while k0 < K:
        slot, seg_q, k1 = {}, [], k0
        while k1 < K and (keys[k1] in slot or len(slot) < _lib.VIDEO_MAX_QUERIES):
            seg_q.append(slot.setdefault(keys[k1], len(slot)))
            k1 += 1
        first = sorted(slot.values())
        pick = [k0 + seg_q.index(s) for s in first]
        rows = torch.cat([x[inside[k]] for k in range(k0, k1)])          # [n_rows, C], gathered per mask
        total = rows.shape[0]
        if total:
            cos = _cosine_native(rows, decoder, q32[pick].contiguous(), int(chunk_rows))
            offs = torch.tensor(np.concatenate([[0], np.cumsum(n[k0:k1])]), dtype=torch.int64, device=x.device)
            sq = torch.tensor(seg_q, dtype=torch.int32, device=x.device)
            B = _lib.Boundary(x.device)
            with torch.cuda.device(x.device):
                _lib.check(lib.lsr_video_segment_mean(total, len(pick), B.ptr(cos, "cosines"), k1 - k0,
                                                      B.ptr(offs, "offsets", torch.int64),
                                                      B.ptr(sq, "query slots", torch.int32),
                                                      B.ptr(sims[k0:k1], "sims"), B.stream()),
                           "lsr_video_segment_mean")
        k0 = k1
    return sims, counts


def smooth_similarity(values, coeffs):
    """The reference's smoothing of a frame-ordered list (eval/eval.py:726-735): an odd-length window of
    coefficients; a frame whose window leaves the sequence keeps its raw value (no partial window)."""
    v = [float(a) for a in values]
    c = [float(a) for a in coeffs]
    if len(c) % 2 != 1:
        raise ValueError(f"coeffs must have an odd length, got {len(c)}")
    if abs(sum(c) - 1) >= 1e-9:
        raise ValueError(f"coeffs must sum to 1, got {sum(c)}")
    half = len(c) // 2
    out = []
    for i in range(len(v)):
        if i - half < 0 or i + half >= len(v):
            out.append(v[i])
            continue
        res = 0
        for j in range(-half, half + 1):
            res += v[i + j] * c[j + half]
        out.append(res)
    return out


def _labelled(idx, gt_intervals):
    return any(lo <= idx <= hi for lo, hi in gt_intervals)


def evaluate_frames(frame_ids, sims, ious, gt_intervals, thresh):
    """evaluate_video_feature (eval/eval.py:355-402): a frame is labelled if its id lies in one of the
    ground-truth intervals (both ends inclusive) and predicted if its similarity >= thresh.  vIoU is the
    mean, over the frames labelled or predicted, of the frame's IoU where both and 0 otherwise; 0 if
    there are no such frames.  Returns accuracy, precision, recall, viou, labels, predictions."""
    ids, s, u = list(frame_ids), [float(a) for a in sims], [float(a) for a in ious]
    if not (len(ids) == len(s) == len(u)):
        raise ValueError(f"frame_ids, sims and ious must have one entry per frame, got {len(ids)}, {len(s)}, {len(u)}")
    if not ids:
        raise ValueError("no frames to evaluate")
    labels = [_labelled(i, gt_intervals) for i in ids]
    preds = [a >= thresh for a in s]
    tp = sum(1 for p, l in zip(preds, labels) if p and l)
    fp = sum(1 for p, l in zip(preds, labels) if p and not l)
    fn = sum(1 for p, l in zip(preds, labels) if not p and l)
    vals = [(u[i] if labels[i] and preds[i] else 0) for i in range(len(ids)) if labels[i] or preds[i]]
    return {"accuracy": sum(1 for p, l in zip(preds, labels) if p == l) / len(preds),
            "precision": tp / (tp + fp) if tp + fp > 0 else 0,
            "recall": tp / (tp + fn) if tp + fn > 0 else 0,
            "viou": sum(vals) / len(vals) if vals else 0,
            "labels": labels, "predictions": preds}


def evaluate_sequence(frame_ids, sims, ious, gt_intervals, coeffs=None, clip_scores=None):
    """The host-side part of one phrase (eval/eval.py:712-790) on per-frame numbers: sort by frame id,
    optionally smooth, threshold and evaluate.  The video similarities are thresholded at the mean of the
    UNSMOOTHED list (:740), the CLIP scores at the mean of the SMOOTHED list (:760).  Returns what
    time_sensitive_query returns, without counts."""
    ids, sims, ious = [int(i) for i in frame_ids], [float(a) for a in sims], [float(a) for a in ious]
    n = len(ids)
    if not n:
        raise ValueError("no frames given")
    if not (len(sims) == len(ious) == n) or (clip_scores is not None and len(clip_scores) != n):
        raise ValueError("frame_ids, sims, ious and clip_scores must have one entry per frame")
    video_thresh = sum(sims) / n                               # of the unsmoothed list, in the order given
    order = sorted(range(n), key=lambda i: ids[i])
    sid = [ids[i] for i in order]
    raw = [sims[i] for i in order]
    siou = [ious[i] for i in order]
    smoothed = smooth_similarity(raw, coeffs) if coeffs is not None else list(raw)
    out = {"frame_ids": sid, "similarity": raw, "smoothed": smoothed, "iou": siou, "video_thresh": video_thresh,
           "video": evaluate_frames(sid, smoothed, siou, gt_intervals, video_thresh),
           "table": list(zip(sid, smoothed, siou))}
    if clip_scores is not None:
        clip = [float(clip_scores[i]) for i in order]
        clip = smooth_similarity(clip, coeffs) if coeffs is not None else clip
        clip_thresh = sum(clip) / n                            # of the smoothed list: the reference's asymmetry
        out.update(clip_smoothed=clip, clip_thresh=clip_thresh,
                   clip=evaluate_frames(sid, clip, siou, gt_intervals, clip_thresh))
    return out


def _load_frame(f, device):
    if isinstance(f, torch.Tensor):
        return f.detach().to(device)
    x = torch.from_numpy(np.load(f)).float().to(device)
    if x.min() > 0:                                            # eval/eval.py:604-605, as query_frames
        x = x * 2.0 - 1
    return x


def time_sensitive_query(frames, masks, ious, decoder, query, gt_intervals, coeffs=None, clip_scores=None,
                         frame_ids=None, layout="hwc", chunk_rows=8192):
    """One video phrase over its frames (eval/eval.py:652-653, 712-790).

    frames: per frame the video latent, a tensor ([H, W, C], or [C, H, W] with layout "chw"; used as it
    is) or the path of a renders_npy file ([H, W, C]; a file whose minimum is > 0 was saved in (0, 1) and
    is mapped back by x * 2 - 1).  masks: per frame the phrase's chosen raw mask [H, W] (segment()'s
    mask_raw at the chosen level; only == 1 counts).  ious: per frame the chosen mask's IoU.  query:
    [d_out], the phrase's embedding.  gt_intervals: [(first, last), ...] frame ids, inclusive.  coeffs:
    None, or the odd-length smoothing window ([0.1, 0.8, 0.1], [0.1, 0.2, 0.4, 0.2, 0.1]).
    clip_scores: None, or per frame the chosen level's CLIP score, evaluated beside the video feature.
    frame_ids default to 0, 1, ...; frames are sorted by them.

    The reference's threshold rules are kept: the video similarities are thresholded at the mean of the
    UNSMOOTHED list, the CLIP scores at the mean of the SMOOTHED list.

    Returns a dict: frame_ids, similarity (unsmoothed), smoothed, iou, counts, video_thresh, video (the
    evaluate_frames dict), table [(frame id, smoothed similarity, iou)], and with clip_scores also
    clip_smoothed, clip_thresh, clip."""
    frames, masks = list(frames), list(masks)
    n = len(frames)
    ids = list(range(n)) if frame_ids is None else [int(i) for i in frame_ids]
    if not n:
        raise ValueError("no frames given")
    if not (len(masks) == len(ious) == len(ids) == n):
        raise ValueError("frames, masks, ious and frame_ids must have one entry per frame")
    dev = decoder.device
    q = torch.as_tensor(query).reshape(1, -1).to(dev)
    sims, counts = [], []
    for f, m in zip(frames, masks):
        x = _load_frame(f, dev)
        s, c = masked_similarity(x, torch.as_tensor(m).to(dev)[None], decoder, q.to(x.dtype), layout=layout,
                                 chunk_rows=chunk_rows)
        sims.append(s)
        counts.append(c)
    sims = [float(a) for a in torch.cat(sims).cpu()]
    counts = [int(a) for a in torch.cat(counts).cpu()]
    out = evaluate_sequence(ids, sims, ious, gt_intervals, coeffs=coeffs, clip_scores=clip_scores)
    by_id = sorted(range(n), key=lambda i: ids[i])
    out["counts"] = [counts[i] for i in by_id]
    return out
