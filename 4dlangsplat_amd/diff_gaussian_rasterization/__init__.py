"""diff_gaussian_rasterization -- drop-in Python surface of the 4D-LangSplat rasterizer, backed by
the MI355X-native liblsr.so (HIP, gfx950) through its C ABI (include/lsr.h).

Mirrors what the reference imports and calls (the submodule zrporz/4d-langsplat-rasterization is
un-vendored, so the surface is taken from its call sites):
  from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
      gaussian_renderer/__init__.py:15, scene/dataset_readers.py:492
  GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier,
      viewmatrix, projmatrix, sh_degree, campos, prefiltered, debug, include_feature)
      gaussian_renderer/__init__.py:49-63 (include_feature defaults to True because
      scene/dataset_readers.py:502-515 builds the settings without it)
  rasterizer(means3D=, means2D=, shs=, colors_precomp=, language_feature_precomp=, opacities=,
      scales=, rotations=, cov3D_precomp=) -> (color [3,H,W], language_feature [C,H,W],
      radii int32 [P], depth [1,H,W])            gaussian_renderer/__init__.py:219-228
  rasterizer.markVisible(positions) -> bool [P]
Errors follow upstream: exactly one of shs / colors_precomp, exactly one of (scales, rotations) /
cov3D_precomp, else an Exception with the upstream message; native failures raise RuntimeError.
means2D's values are ignored; its .grad receives the screen-space gradient (NDC units).
"""
from __future__ import annotations

import ctypes
import functools
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _lib

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "RasterizerState",
           "forward_native", "backward_native", "backward_views_native", "backward_composite_native",
           "backward_preprocess_views_native", "preprocess_views_native", "binning_views_native",
           "render_views_native", "backward_composite_views_native", "language_split_native", "rasterize_views",
           "radii_max_native"]

_lib.load()   # fail loudly at import if the native library is missing
_BINNING_DELAY_CYCLES = 0   # tests only: GPU cycles slept on the stream before a side-stream binning


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    include_feature: bool = True


def _opt(t):
    """upstream passes torch.Tensor([]) for 'not provided'"""
    if t is None or t.numel() == 0:
        return None
    return t


def _f32(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _struct_array(cls, structs):
    """cls* const* over ctypes structures (the per-view arrays of the *_views entry points)"""
    return (ctypes.POINTER(cls) * len(structs))(*[ctypes.pointer(x) for x in structs])


def _settings_array(settings):
    return _struct_array(_lib.Settings, [s.c for s in settings])     # of _NativeSettings


def _int64_array(values):
    return (ctypes.c_int64 * len(values))(*values)


class _NativeSettings:
    """Keeps the device copies of the small settings tensors alive for the duration of a call."""

    def __init__(self, rs: GaussianRasterizationSettings, device):
        self.bg = _f32(rs.bg, device).reshape(-1)
        self.view = _f32(rs.viewmatrix, device).reshape(-1)
        self.proj = _f32(rs.projmatrix, device).reshape(-1)
        self.campos = _f32(rs.campos, device).reshape(-1)
        if self.bg.numel() != 3 or self.view.numel() != 16 or self.proj.numel() != 16 or self.campos.numel() != 3:
            raise ValueError("bg/campos must have 3 elements and view/proj matrices 16")
        B = _lib.Boundary(device)
        s = _lib.Settings()
        s.image_height, s.image_width = int(rs.image_height), int(rs.image_width)
        s.tanfovx, s.tanfovy = float(rs.tanfovx), float(rs.tanfovy)
        s.bg, s.scale_modifier = B.ptr(self.bg, "bg"), float(rs.scale_modifier)
        s.viewmatrix, s.projmatrix = B.ptr(self.view, "viewmatrix"), B.ptr(self.proj, "projmatrix")
        s.sh_degree, s.campos = int(rs.sh_degree), B.ptr(self.campos, "campos")
        s.prefiltered, s.debug = int(bool(rs.prefiltered)), int(bool(rs.debug))
        s.include_feature = int(bool(rs.include_feature))
        self.c = s


class RasterizerState:
    """What the forward leaves for the backward (upstream: num_rendered + geom/binning/img buffers)."""

    def __init__(self, settings, inputs, fin, geom, binning, img, num_rendered, radii):
        self.settings, self.inputs, self.fin = settings, inputs, fin
        self.geom, self.binning, self.img = geom, binning, img
        self.num_rendered, self.radii = num_rendered, radii
        self.composited = False           # backward_composite_native ran (it may run once)


class PendingForward:
    """Phase 1 of a forward (preprocess, depth order, instance count) done; render_native finishes
    it.  Holds the inputs, the geom workspace and num_rendered (K)."""

    def __init__(self, raster_settings, settings, fin, inputs, geom, radii, K, device, H, W):
        self.raster_settings, self.settings, self.fin, self.inputs = raster_settings, settings, fin, inputs
        self.geom, self.radii, self.num_rendered, self.device, self.H, self.W = geom, radii, K, device, H, W
        self.binning = self.img = None     # set when the binning already ran (preprocess_native(binning=True))
        self.ready = None                  # event recorded after that binning
        self.ready_stream = None           # the stream `ready` was recorded on
        self.count_host = None             # deferred count (preprocess_native(defer_count=True)): pinned
        self.counted = None                # [K, reserved], valid once `counted` (an event) has passed
        self.stream = None
        self.count_batch = None            # (pinned [n, 2] counts of a batch, this view's row)
        self.tile_bucket = False           # phase 1 prepared the tile-bucket binning (id-order counts)

    def resolve(self, binning=False):
        """Deferred-count forwards: wait for the instance count (host waits on the event only, not
        the stream), then optionally enqueue the binning on the preprocess stream.  No-op otherwise."""
        if self.counted is None:
            return self
        self.counted.synchronize()
        self.counted = None
        self.num_rendered = int(self.count_host[0])
        if binning:
            _run_binning(self, self.stream)
        return self


def _dump_forward(raster_settings, inputs):
    if raster_settings.debug:
        torch.save({k: (None if v is None else v.cpu()) for k, v in inputs.items()
                    if k in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations")},
                   "snapshot_fw.dump")
        print("\nAn error occured in forward. Writing snapshot_fw.dump for debugging.")


def _check_forward(rc, what, raster_settings, inputs):
    """_lib.check of a forward entry point's return code; on failure the inputs are dumped (debug mode)."""
    try:
        _lib.check(rc, what)
    except RuntimeError:
        _dump_forward(raster_settings, inputs)
        raise


def _check_device(t):
    if t.device.type != "cuda":
        raise RuntimeError("the rasterizer runs on the GPU only (no CPU fallback); got tensors on " + str(t.device))
    return t.device


def _fwd_inputs(means3D, opacities, shs, colors_precomp, language_feature, scales, rotations, cov3D_precomp):
    """fp32 contiguous device inputs and their lsr_fwd_in; returns (fin, inputs, P)."""
    device = _check_device(means3D)
    P = means3D.shape[0]
    means3D = _f32(means3D, device)
    opacities = _f32(opacities, device)
    shs = _opt(shs)
    colors_precomp = _opt(colors_precomp)
    language_feature = _opt(language_feature)
    scales, rotations, cov3D_precomp = _opt(scales), _opt(rotations), _opt(cov3D_precomp)
    shs = _f32(shs, device) if shs is not None else None
    colors_precomp = _f32(colors_precomp, device) if colors_precomp is not None else None
    language_feature = _f32(language_feature, device).reshape(P, -1) if language_feature is not None else None
    scales = _f32(scales, device) if scales is not None else None
    rotations = _f32(rotations, device) if rotations is not None else None
    cov3D_precomp = _f32(cov3D_precomp, device) if cov3D_precomp is not None else None
    M = shs.reshape(P, -1, 3).shape[1] if shs is not None else 0
    C = language_feature.shape[1] if language_feature is not None else 0
    fin = _lib.FwdIn()
    fin.P, fin.M, fin.C = P, M, C
    inputs = dict(means3D=means3D, opacities=opacities, shs=shs, colors_precomp=colors_precomp,
                  language_feature=language_feature, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
    B = _lib.Boundary(device)
    fin.means3D, fin.opacities = B.ptr(means3D, "means3D"), B.ptr(opacities, "opacities")
    for name in ("shs", "colors_precomp", "language_feature", "scales", "rotations", "cov3D_precomp"):
        setattr(fin, name, B.opt(inputs[name], name))
    return fin, inputs, P


def preprocess_native(raster_settings, means3D, opacities, shs=None, colors_precomp=None, language_feature=None,
                      scales=None, rotations=None, cov3D_precomp=None, stream=None, binning=False,
                      defer_count=False):
    """Forward phase 1 through liblsr.so (lsr_forward_preprocess) on `stream` (a torch stream,
    default: the current one).  Synchronises that stream once to read num_rendered (as upstream).
    binning=True also runs the tile binning there (lsr_forward_binning), so that render_native
    only composites.  Workspaces are allocated on `stream`; render_native may run on another
    stream.

    defer_count=True (lsr_forward_preprocess_async) does not synchronise: the count lands in pinned
    host memory and PendingForward.resolve(binning) reads it later (render_native resolves too),
    so a caller can enqueue this view's preprocess ahead of another view's work on the same stream."""
    device = _check_device(means3D)
    L, B = _lib.load(), _lib.Boundary(device)
    stream = stream or torch.cuda.current_stream(device)
    st = _NativeSettings(raster_settings, device)
    fin, inputs, P = _fwd_inputs(means3D, opacities, shs, colors_precomp, language_feature, scales, rotations,
                                 cov3D_precomp)
    H, W = int(raster_settings.image_height), int(raster_settings.image_width)
    with torch.cuda.stream(stream):
        radii = torch.empty(P, dtype=torch.int32, device=device)
        geom = torch.empty(int(L.lsr_geom_bytes(P)), dtype=torch.uint8, device=device)
    fout = _lib.FwdOut()
    fout.radii = B.ptr(radii, "radii", torch.int32)
    if defer_count:
        count = torch.zeros(2, dtype=torch.int32, pin_memory=True)
        _check_forward(L.lsr_forward_preprocess_async(ctypes.byref(st.c), ctypes.byref(fin), ctypes.byref(fout),
                                                      B.ptr(geom, "geom", torch.uint8),
                                                      _lib.HOST.ptr(count, "count", torch.int32), B.stream(stream)),
                       "lsr_forward_preprocess_async", raster_settings, inputs)
        pf = PendingForward(raster_settings, st, fin, inputs, geom, radii, None, device, H, W)
        pf.count_host, pf.stream = count, stream
        pf.counted = torch.cuda.Event()
        pf.counted.record(stream)
        return pf
    K = ctypes.c_int64(0)
    _check_forward(L.lsr_forward_preprocess(ctypes.byref(st.c), ctypes.byref(fin), ctypes.byref(fout),
                                            B.ptr(geom, "geom", torch.uint8), ctypes.byref(K), B.stream(stream)),
                   "lsr_forward_preprocess", raster_settings, inputs)
    pf = PendingForward(raster_settings, st, fin, inputs, geom, radii, K.value, device, H, W)
    if binning:
        _run_binning(pf, stream)
    return pf


def _run_binning(pf, stream):
    """lsr_forward_binning of a preprocessed view on `stream`; render_native's stream waits for it."""
    L, B = _lib.load(), _lib.Boundary(pf.device)
    device, H, W, K = pf.device, pf.H, pf.W, pf.num_rendered
    if _BINNING_DELAY_CYCLES:             # test hook: holds the binning back to expose missing waits
        with torch.cuda.stream(stream):
            torch.cuda._sleep(_BINNING_DELAY_CYCLES)
    with torch.cuda.stream(stream):
        pf.binning = torch.empty(int(L.lsr_binning_bytes(K)), dtype=torch.uint8, device=device)
        pf.img = torch.empty(int(L.lsr_img_bytes(W, H)), dtype=torch.uint8, device=device)
    _check_forward(L.lsr_forward_binning(ctypes.byref(pf.settings.c), ctypes.byref(pf.fin),
                                         B.ptr(pf.geom, "geom", torch.uint8),
                                         B.ptr(pf.binning, "binning", torch.uint8),
                                         B.ptr(pf.img, "img", torch.uint8), ctypes.c_int64(K), B.stream(stream)),
                   "lsr_forward_binning", pf.raster_settings, pf.inputs)
    pf.ready = torch.cuda.Event()
    pf.ready.record(stream)               # render_native's stream waits for the binning
    pf.ready_stream = stream


def language_split_native(language_feature, stream=None, out=None):
    """lsr_language_split: [P,32] fp32 -> [P,64] int16 holding the bf16 bit patterns (hi channels,
    then lo) that the compositors' matrix-core operands use; lsr_fwd_in.language_feature_split.
    `out` may be a preallocated [P,64] int16 tensor."""
    device = _check_device(language_feature)
    L, B = _lib.load(), _lib.Boundary(device)
    P, C = language_feature.shape
    stream = stream or torch.cuda.current_stream(device)
    lang = language_feature.detach().to(torch.float32).contiguous()
    if out is None:
        with torch.cuda.stream(stream):
            out = torch.empty(P, 2 * C, dtype=torch.int16, device=device)
    elif out.shape != (P, 2 * C) or out.dtype != torch.int16 or not out.is_contiguous():
        raise ValueError("language_split_native: out must be a contiguous [P, 2C] int16 tensor")
    _lib.check(L.lsr_language_split(P, C, B.ptr(lang, "language_feature"), B.ptr(out, "out", torch.int16),
                                    B.stream(stream)), "lsr_language_split")
    return out


def preprocess_views_native(raster_settings_list, means3D, opacities, shs=None, colors_precomp=None,
                            language_feature=None, scales=None, rotations=None, cov3D_precomp=None, stream=None,
                            split_language=True, split_behind_counts=True, split_stream=None, order_first=None,
                            order_stream=None, row_chunks=None, tile_bucket=False):
    """Forward phase 1 of several views of the same Gaussians as one batch
    (lsr_forward_preprocess_views_async: one preprocess launch per 8 views reads each Gaussian once,
    the views' depth sorts and instance scans share their launches) on `stream`.  No host
    synchronisation: returns one deferred-count PendingForward per view; binning_views_native
    resolves them all with one wait.  Same results as preprocess_native per view.

    split_language (C == 32): the language rows' bf16 hi / lo operands are made once here for all
    the batch's views (lsr_language_split) instead of per entry in every compositor wave (same
    bits, same results).  split_behind_counts: enqueue that split behind the batch's count event, so
    it runs while the host waits for the counts (False: ahead of the preprocess; an A/B switch).
    split_stream: enqueue the split there instead (after that stream waits for `stream`); the caller
    orders the compositors after it.

    order_first = k < n with order_stream: only the first k views are depth-ordered and counted on
    `stream` (lsr_forward_preprocess_views_split_async); the other views' depth orders and counts run
    on order_stream behind the preprocess (lsr_forward_depth_order_views_async), so the first views'
    binning and compositing start before the later views' sorts.  Those views carry their own count
    batch (binning_views_native waits for it on their first binning); same results.

    row_chunks = [(r0, r1, before), ...] covering [0, P) in order (r0 multiples of 256): the
    preprocess runs one launch per row chunk (lsr_forward_preprocess_views_rows_async), each after
    before() (which makes `stream` wait for that chunk's rows, e.g. the sharded optimizer's
    all-gather of them), and the depth orders follow once every chunk is in; same results.

    tile_bucket: prepare the tile-bucket binning instead (lsr_forward_preprocess_views_tb_async +
    lsr_forward_instance_scan_views_async: no depth sort; binning_views_native then buckets the
    instances by tile and sorts each bucket in LDS, lsr_forward_binning_views_tb).  Same lists, same
    results; the split into first views and order_stream views applies to the instance scans."""
    device = _check_device(means3D)
    L, B = _lib.load(), _lib.Boundary(device)
    stream = stream or torch.cuda.current_stream(device)
    fin, inputs, P = _fwd_inputs(means3D, opacities, shs, colors_precomp, language_feature, scales, rotations,
                                 cov3D_precomp)
    if row_chunks:   # validated before anything is enqueued (both binning paths)
        covered = 0
        for r0, r1, _ in row_chunks:
            if r0 != covered or r1 < r0 or r0 % 256:
                raise ValueError("row_chunks must cover [0, P) in order, each r0 a multiple of 256")
            covered = r1
        if covered != P:
            raise ValueError("row_chunks must cover [0, P) in order, each r0 a multiple of 256")
    split = split_language and fin.C == 32 and P > 0
    if split:   # allocated now (fin carries the pointer), written behind the batch's count event
        with torch.cuda.stream(stream):
            inputs["language_feature_split"] = torch.empty(P, 64, dtype=torch.int16, device=device)
        fin.language_feature_split = B.ptr(inputs["language_feature_split"], "language_feature_split", torch.int16)
        # with row_chunks the language rows may still be arriving (each chunk's before() waits for
        # them): the split is then always enqueued behind the chunk loop
        if not split_behind_counts and not row_chunks:
            language_split_native(inputs["language_feature"], stream=stream, out=inputs["language_feature_split"])
            split = False
    n = len(raster_settings_list)
    sts = [_NativeSettings(rs, device) for rs in raster_settings_list]
    with torch.cuda.stream(stream):
        radii = [torch.empty(P, dtype=torch.int32, device=device) for _ in range(n)]
        geoms = [torch.empty(int(L.lsr_geom_bytes(P)), dtype=torch.uint8, device=device) for _ in range(n)]
    fouts = [_lib.FwdOut() for _ in range(n)]
    for fo, r in zip(fouts, radii):
        fo.radii = B.ptr(r, "radii", torch.int32)
    k = n if (order_first is None or order_stream is None) else max(0, min(int(order_first), n))
    counts = torch.zeros(k, 2, dtype=torch.int32, pin_memory=True) if k > 0 else None
    s_arr, o_arr, g_arr = _settings_array(sts), _struct_array(_lib.FwdOut, fouts), B.array(geoms, "geom", torch.uint8)
    fi, stp = ctypes.byref(fin), B.stream(stream)

    def check(rc, what):
        _check_forward(rc, what, raster_settings_list[0], inputs)

    count_fn, count_what = ((L.lsr_forward_instance_scan_views_async, "lsr_forward_instance_scan_views_async")
                            if tile_bucket else
                            (L.lsr_forward_depth_order_views_async, "lsr_forward_depth_order_views_async"))
    if tile_bucket or row_chunks:
        rows_fn, rows_what = ((L.lsr_forward_preprocess_views_tb_async, "lsr_forward_preprocess_views_tb_async")
                              if tile_bucket else
                              (L.lsr_forward_preprocess_views_rows_async, "lsr_forward_preprocess_views_rows_async"))
        for r0, r1, before in (row_chunks or [(0, P, None)]):
            if before is not None:
                before()
            check(rows_fn(n, int(r0), int(r1), s_arr, fi, o_arr, g_arr, stp), rows_what)
        if k > 0:
            check(count_fn(k, s_arr, fi, g_arr, _lib.HOST.ptr(counts, "counts", torch.int32), stp), count_what)
    else:
        check(L.lsr_forward_preprocess_views_split_async(n, k, s_arr, fi, o_arr, g_arr,
                                                         _lib.HOST.opt(counts, "counts", torch.int32), stp),
              "lsr_forward_preprocess_views_split_async")
    ev = torch.cuda.Event()
    ev.record(stream)
    late = None
    if k < n:   # the later views' depth orders and counts on order_stream, behind the preprocess
        order_stream.wait_event(ev)
        for g in geoms[k:]:
            g.record_stream(order_stream)
        counts_b = torch.zeros(n - k, 2, dtype=torch.int32, pin_memory=True)
        check(count_fn(n - k, _settings_array(sts[k:]), fi, B.array(geoms[k:], "geom", torch.uint8),
                       _lib.HOST.ptr(counts_b, "counts", torch.int32), B.stream(order_stream)), count_what)
        ev_b = torch.cuda.Event()
        ev_b.record(order_stream)
        late = (counts_b, ev_b)
    if split and split_stream is not None:   # on the caller's side stream, beside the binning
        split_stream.wait_stream(stream)
        inputs["language_feature_split"].record_stream(split_stream)
        language_split_native(inputs["language_feature"], stream=split_stream, out=inputs["language_feature_split"])
    elif split:   # only the compositors read it: it runs while the host waits for the counts
        language_split_native(inputs["language_feature"], stream=stream, out=inputs["language_feature_split"])
    out = []
    for v, rs in enumerate(raster_settings_list):
        H, W = int(rs.image_height), int(rs.image_width)
        pf = PendingForward(rs, sts[v], fin, inputs, geoms[v], radii[v], None, device, H, W)
        pf.tile_bucket = bool(tile_bucket)
        if v < k:
            pf.count_host, pf.stream, pf.counted = counts[v], stream, ev
            pf.count_batch = (counts, v)      # binning_views_native reads the whole batch at once
        else:
            pf.count_host, pf.stream, pf.counted = late[0][v - k], order_stream, late[1]
            pf.count_batch = (late[0], v - k)
        out.append(pf)
    return out


def _align(nbytes, a=256):
    return (nbytes + a - 1) // a * a


@functools.lru_cache(maxsize=4096)
def _binning_bytes(K):   # pure size queries, asked on the device's critical path (the count wait)
    return _align(int(_lib.load().lsr_binning_bytes(K)))


@functools.lru_cache(maxsize=4096)
def _binning_bytes_tb(K, P, W, H):
    return _align(int(_lib.load().lsr_binning_bytes_tb(K, P, W, H)))


@functools.lru_cache(maxsize=64)
def _img_bytes(W, H):
    return _align(int(_lib.load().lsr_img_bytes(W, H)))


def _view_arrays(views, *between):
    """(settings array, &fin, *between, geom, binning, img and num_rendered arrays) of binned views
    (PendingForward or RasterizerState) of the same Gaussians: the *_views entry points' argument run."""
    B = _lib.Boundary(views[0].geom.device)
    return (_settings_array([v.settings for v in views]), ctypes.byref(views[0].fin), *between,
            B.array([v.geom for v in views], "geom", torch.uint8),
            B.array([v.binning for v in views], "binning", torch.uint8),
            B.array([v.img for v in views], "img", torch.uint8), _int64_array([v.num_rendered for v in views]))


def _forward_outputs(pf):
    """A view's colour, language and depth images on the current stream, and their lsr_fwd_out."""
    H, W, C = pf.H, pf.W, pf.fin.C
    color = torch.empty(3, H, W, dtype=torch.float32, device=pf.device)
    lang_out = torch.empty(C, H, W, dtype=torch.float32, device=pf.device)
    depth = torch.empty(1, H, W, dtype=torch.float32, device=pf.device)
    B = _lib.Boundary(pf.device)
    fout = _lib.FwdOut()
    fout.out_color = B.ptr(color, "out_color")
    fout.out_language_feature = B.ptr(lang_out, "out_language_feature") if C > 0 else None
    fout.radii, fout.out_depth = B.ptr(pf.radii, "radii", torch.int32), B.ptr(depth, "out_depth")
    return color, lang_out, depth, fout


def _wait_for_binning(pf, stream, waited=None):
    """`stream` waits for pf's binning event, once: not when the binning ran on `stream` (already
    ordered; a wait idles the device) and not when `waited` has the (event, stream) pair (views
    binned together share one event).  waited: the caller's set for one batch; None: a set kept on
    the event itself, across calls."""
    if pf.ready_stream is None or pf.ready_stream == stream:
        return
    if waited is None:
        waited = getattr(pf.ready, "_lsr_waited_by", None)
        if waited is None:
            waited = set()
            try:
                pf.ready._lsr_waited_by = waited
            except AttributeError:
                pass
    key = (id(pf.ready), stream.cuda_stream)
    if key not in waited:
        stream.wait_event(pf.ready)
        waited.add(key)


def binning_views_native(pendings, stream=None):
    """Resolve the deferred counts of preprocess_views_native's views (one host wait) and run their
    tile binning as one batch (lsr_forward_binning_views) on `stream` (default: theirs), so that
    render_native only composites each view."""
    if not pendings:
        return
    L = _lib.load()
    stream = stream or pendings[0].stream
    # the device idles from the counts' arrival to the emission launch, so this stretch is kept
    # short: one wait and one read for a batch's counts, one allocation for all workspaces
    batch = pendings[0].count_batch
    if batch is not None and all(pf.count_batch is not None and pf.count_batch[0] is batch[0] for pf in pendings):
        pendings[0].counted.synchronize()
        rows = batch[0].tolist()
        for pf in pendings:
            pf.num_rendered, pf.counted = rows[pf.count_batch[1]][0], None
    else:
        for pf in pendings:
            pf.resolve()
    n = len(pendings)
    device = pendings[0].device
    tb = pendings[0].tile_bucket
    if any(pf.tile_bucket != tb for pf in pendings):
        raise ValueError("binning_views_native: a batch mixes tile-bucket and sort-path views")
    sizes = []
    for pf in pendings:
        sizes += [_binning_bytes_tb(pf.num_rendered, pf.fin.P, pf.W, pf.H) if tb else _binning_bytes(pf.num_rendered),
                  _img_bytes(pf.W, pf.H)]
    with torch.cuda.stream(stream):
        ws = torch.empty(sum(sizes), dtype=torch.uint8, device=device)
    off = 0
    for i, pf in enumerate(pendings):
        pf.binning = ws[off:off + sizes[2 * i]]
        off += sizes[2 * i]
        pf.img = ws[off:off + sizes[2 * i + 1]]
        off += sizes[2 * i + 1]
    fn, what = ((L.lsr_forward_binning_views_tb, "lsr_forward_binning_views_tb") if tb
                else (L.lsr_forward_binning_views, "lsr_forward_binning_views"))
    _check_forward(fn(n, *_view_arrays(pendings), _lib.Boundary(device).stream(stream)), what,
                   pendings[0].raster_settings, pendings[0].inputs)
    ev = torch.cuda.Event()
    ev.record(stream)
    for pf in pendings:
        pf.ready, pf.ready_stream = ev, stream


def render_native(pending: PendingForward):
    """Forward phase 2 (binning unless preprocess_native already did it, then compositing) on the
    current stream.  Returns (color, language_feature, radii, depth, state)."""
    L = _lib.load()
    if pending.tile_bucket and pending.binning is None:   # lsr_forward_render bins the sort path's way
        binning_views_native([pending], stream=torch.cuda.current_stream(pending.device))
    pending.resolve()
    device, H, W = pending.device, pending.H, pending.W
    B = _lib.Boundary(device)
    stream = torch.cuda.current_stream(device)
    pending.geom.record_stream(stream)    # allocated on the preprocess stream, used from here on
    pending.radii.record_stream(stream)
    color, lang_out, depth, fout = _forward_outputs(pending)
    K = pending.num_rendered
    binned = pending.binning is not None
    if binned:
        binning, img = pending.binning, pending.img
        _wait_for_binning(pending, stream)
        binning.record_stream(stream)
        img.record_stream(stream)
    else:
        binning = torch.empty(int(L.lsr_binning_bytes(K)), dtype=torch.uint8, device=device)
        img = torch.empty(int(L.lsr_img_bytes(W, H)), dtype=torch.uint8, device=device)
    fn, what = (L.lsr_forward_composite, "lsr_forward_composite") if binned else (L.lsr_forward_render,
                                                                                   "lsr_forward_render")
    _check_forward(fn(ctypes.byref(pending.settings.c), ctypes.byref(pending.fin), ctypes.byref(fout),
                      B.ptr(pending.geom, "geom", torch.uint8), B.ptr(binning, "binning", torch.uint8),
                      B.ptr(img, "img", torch.uint8), ctypes.c_int64(K), B.stream(stream)), what,
                   pending.raster_settings, pending.inputs)
    state = RasterizerState(pending.settings, pending.inputs, pending.fin, pending.geom, binning, img, K, pending.radii)
    return color, lang_out, pending.radii, depth, state


def radii_max_native(radii, out, accumulate=False, stream=None):
    """lsr_radii_max: out = max(out if accumulate, radii[0], ..., radii[n-1]) elementwise, int32 [P]
    device tensors, one launch per 8 views on `stream` (default: current): the radii MAX over a
    batch's views (train.py:270) without a stack copy or one launch per view."""
    if not radii:
        return out
    L = _lib.load()
    P = out.shape[0]
    rs = [r.contiguous() for r in radii]
    for r in rs:
        if r.dtype != torch.int32 or r.shape != (P,) or r.device != out.device:
            raise ValueError("radii_max_native: int32 [P] tensors on out's device")
    if out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError("radii_max_native: out must be a contiguous int32 tensor")
    B = _lib.Boundary(_check_device(out))
    _lib.check(L.lsr_radii_max(P, len(rs), B.array(rs, "radii", torch.int32), B.ptr(out, "out", torch.int32),
                               1 if accumulate else 0, B.stream(stream)), "lsr_radii_max")
    return out


def render_views_native(pendings):
    """render_native for several views of the same Gaussians and image size, their compositing as
    ONE launch per 8 views (lsr_forward_composite_views: a view's last waves run beside the next
    view's first ones).  Views not binned yet are binned first, as one batch.  Same results as
    render_native per view.  Returns a list of (color, language_feature, radii, depth, state)."""
    if not pendings:
        return []
    L = _lib.load()
    unbinned = [pf for pf in pendings if pf.binning is None]
    if unbinned:
        binning_views_native(unbinned, stream=torch.cuda.current_stream(unbinned[0].device))
    device = pendings[0].device
    stream = torch.cuda.current_stream(device)
    waited = set()
    outs, fouts = [], []
    for pf in pendings:
        if pf.device != device or (pf.H, pf.W) != (pendings[0].H, pendings[0].W):
            raise ValueError("render_views_native: the views must share the device and image size")
        _wait_for_binning(pf, stream, waited)   # one wait per binning batch
        for t in (pf.geom, pf.radii, pf.binning, pf.img):
            t.record_stream(stream)
        color, lang_out, depth, fout = _forward_outputs(pf)
        outs.append((color, lang_out, depth))
        fouts.append(fout)
    _check_forward(L.lsr_forward_composite_views(len(pendings),
                                                 *_view_arrays(pendings, _struct_array(_lib.FwdOut, fouts)),
                                                 _lib.Boundary(device).stream(stream)),
                   "lsr_forward_composite_views", pendings[0].raster_settings, pendings[0].inputs)
    res = []
    for pf, (color, lang_out, depth) in zip(pendings, outs):
        state = RasterizerState(pf.settings, pf.inputs, pf.fin, pf.geom, pf.binning, pf.img, pf.num_rendered, pf.radii)
        res.append((color, lang_out, pf.radii, depth, state))
    return res


def forward_native(raster_settings, means3D, opacities, shs=None, colors_precomp=None, language_feature=None,
                   scales=None, rotations=None, cov3D_precomp=None):
    """Forward through liblsr.so on the current stream.  Returns (color, language_feature, radii,
    depth, state)."""
    return render_native(preprocess_native(raster_settings, means3D, opacities, shs=shs, colors_precomp=colors_precomp,
                                           language_feature=language_feature, scales=scales, rotations=rotations,
                                           cov3D_precomp=cov3D_precomp))


def backward_native(state: RasterizerState, grad_color, grad_lang=None, grad_depth=None, out=None,
                    accumulate=False, need=None, deterministic=False):
    """Backward through liblsr.so.  `out` may hold preallocated gradient buffers (dict); with
    accumulate=True they are added to.  deterministic=True selects the fixed-order reduction
    (bitwise reproducible gradients).  Returns the dict of gradient tensors."""
    L = _lib.load()
    device = state.inputs["means3D"].device
    B = _lib.Boundary(device)
    P, C = state.fin.P, state.fin.C
    g = _grad_buffers(state, out, accumulate, need or {})
    keep, gin = _bwd_in(state, grad_color, grad_lang, grad_depth, deterministic)   # keep: alive until enqueued
    gout = _bwd_out(g, B)
    scratch = torch.empty(int(L.lsr_backward_bytes(P, state.num_rendered, C, 1 if deterministic else 0)),
                          dtype=torch.uint8, device=device)
    rc = L.lsr_backward(ctypes.byref(state.settings.c), ctypes.byref(state.fin), ctypes.byref(gin), ctypes.byref(gout),
                        B.ptr(state.geom, "geom", torch.uint8), B.ptr(state.binning, "binning", torch.uint8),
                        B.ptr(state.img, "img", torch.uint8), B.ptr(scratch, "scratch", torch.uint8),
                        ctypes.c_int64(state.num_rendered), ctypes.c_int32(1 if accumulate else 0), B.stream())
    if rc != 0 and state.settings.c.debug:
        print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.")
        torch.save(dict(grad_color=keep[0].cpu()), "snapshot_bw.dump")
    _lib.check(rc, "lsr_backward")
    return g


def backward_views_native(states, grad_colors, grad_langs=None, grad_depths=None, out=None, accumulate=False,
                          need=None):
    """Backward of several views of the SAME Gaussians through liblsr.so (lsr_backward_views):
    the gradients of every view are summed, as train.py's loss.backward() sums its per-view renders
    (train.py:242-268,339).  Each view's compositor backward runs, then one preprocess backward
    per 8 views reads the Gaussian rows and writes the gradient rows once.  Float-atomic reduction
    (for bitwise-reproducible gradients use backward_native(deterministic=True) per view).
    `states` are the RasterizerState of the views' forwards; grad_* are per-view lists (entries may
    be None).  Returns the dict of gradient tensors (out's buffers when given)."""
    L = _lib.load()
    n = len(states)
    if n == 0:
        raise ValueError("backward_views_native needs at least one view")
    for s in states:
        if s.composited:
            raise RuntimeError("a view's forward was already backpropagated through its workspace accumulators "
                               "(backward_composite_native / backward_views_native run once per forward)")
    st0 = states[0]
    inp = st0.inputs
    for s in states[1:]:
        if s.inputs["means3D"].data_ptr() != inp["means3D"].data_ptr():
            raise ValueError("all views must render the same Gaussians")
    B = _lib.Boundary(inp["means3D"].device)
    g = _grad_buffers(st0, out, accumulate, need or {})
    keeps, gins = _bwd_in_views(states, grad_colors, grad_langs, grad_depths)   # keeps: alive until enqueued
    gout = _bwd_out(g, B)
    _lib.check(L.lsr_backward_views(n, *_view_arrays(states, _struct_array(_lib.BwdIn, gins), ctypes.byref(gout)),
                                    1 if accumulate else 0, B.stream()), "lsr_backward_views")
    for s in states:
        s.composited = True
    return g


class CompositeGrad:
    """A view whose compositor backward ran (backward_composite_native): its forward state and the
    upstream gradients; the per-Gaussian screen-space sums that backward_preprocess_views_native
    consumes live in the state's geom buffer."""

    def __init__(self, state, keep):
        self.state, self._keep = state, keep


def backward_composite_native(state: RasterizerState, grad_color, grad_lang=None, grad_depth=None,
                              dL_dlanguage=None) -> CompositeGrad:
    """First half of backward_views_native for ONE view (lsr_backward_composite), on the current
    stream: the compositor backward; the language gradient is ADDED to dL_dlanguage [P,C] (the
    caller zeroes it once per batch).  Finish a batch with backward_preprocess_views_native."""
    L = _lib.load()
    if state.composited:
        raise RuntimeError("backward_composite_native already ran on this forward: its screen-space sums are "
                           "accumulated in the forward's workspace, so a second run would double them")
    B = _lib.Boundary(state.inputs["means3D"].device)
    P, C = state.fin.P, state.fin.C
    keep, gi = _bwd_in(state, grad_color, grad_lang, grad_depth)
    if dL_dlanguage is not None and (dL_dlanguage.shape != (P, C) or not dL_dlanguage.is_contiguous()):
        raise ValueError("dL_dlanguage must be a contiguous [P, C] tensor")
    _lib.check(L.lsr_backward_composite(ctypes.byref(state.settings.c), ctypes.byref(state.fin), ctypes.byref(gi),
                                        B.opt(dL_dlanguage if C > 0 else None, "dL_dlanguage"),
                                        B.ptr(state.geom, "geom", torch.uint8),
                                        B.ptr(state.binning, "binning", torch.uint8),
                                        B.ptr(state.img, "img", torch.uint8),
                                        ctypes.c_int64(state.num_rendered), B.stream()), "lsr_backward_composite")
    state.composited = True
    return CompositeGrad(state, keep)


def backward_composite_views_native(states, grad_colors, grad_langs=None, grad_depths=None,
                                    dL_dlanguage=None):
    """backward_composite_native for several views of the same Gaussians and image size, their
    compositor backward as ONE launch per 8 views (lsr_backward_composite_views; one launch for
    their tile orders too).  grad_* are per-view lists (entries may be None).  Returns a list of
    CompositeGrad for backward_preprocess_views_native."""
    if not states:
        return []
    L = _lib.load()
    for s in states:
        if s.composited:
            raise RuntimeError("backward_composite_native already ran on this forward: its screen-space sums are "
                               "accumulated in the forward's workspace, so a second run would double them")
    st0 = states[0]
    B = _lib.Boundary(st0.inputs["means3D"].device)
    P, C = st0.fin.P, st0.fin.C
    if dL_dlanguage is not None and (dL_dlanguage.shape != (P, C) or not dL_dlanguage.is_contiguous()):
        raise ValueError("dL_dlanguage must be a contiguous [P, C] tensor")
    for s in states:
        if s.inputs["means3D"].data_ptr() != st0.inputs["means3D"].data_ptr():
            raise ValueError("all views must render the same Gaussians")
    keeps, gins = _bwd_in_views(states, grad_colors, grad_langs, grad_depths)
    _lib.check(L.lsr_backward_composite_views(len(states),
                                              *_view_arrays(states, _struct_array(_lib.BwdIn, gins),
                                                            B.opt(dL_dlanguage if C > 0 else None, "dL_dlanguage")),
                                              B.stream()), "lsr_backward_composite_views")
    for s in states:
        s.composited = True
    return [CompositeGrad(s, k) for s, k in zip(states, keeps)]


def backward_preprocess_views_native(parts, out=None, accumulate=False, need=None, row_chunks=None, on_rows=None):
    """Second half of backward_views_native (lsr_backward_preprocess_views): the preprocess backward
    of every view in `parts` (CompositeGrad), summed into one set of gradient rows.  The language
    gradient is not touched here (the composite halves added it).  Returns the dict of gradients.

    row_chunks: [(r0, r1), ...] covering [0, P) in order (r0 multiples of 256): one launch per chunk
    (lsr_backward_preprocess_views_rows), and on_rows(r0, r1) is called right after each chunk's
    launch is enqueued, so a data-parallel caller can start that chunk's all-reduce while the next
    chunk computes."""
    L = _lib.load()
    n = len(parts)
    if n == 0:
        raise ValueError("backward_preprocess_views_native needs at least one view")
    st0 = parts[0].state
    inp = st0.inputs
    for p_ in parts[1:]:
        if p_.state.inputs["means3D"].data_ptr() != inp["means3D"].data_ptr():
            raise ValueError("all views must render the same Gaussians")
    B = _lib.Boundary(inp["means3D"].device)
    need = dict(need or {})
    need["language_feature"] = False
    g = _grad_buffers(st0, out, accumulate, need)
    gout = _bwd_out(g, B)
    s_arr = _settings_array([p_.state.settings for p_ in parts])
    geoms = B.array([p_.state.geom for p_ in parts], "geom", torch.uint8)
    if row_chunks is None:
        _lib.check(L.lsr_backward_preprocess_views(n, s_arr, ctypes.byref(st0.fin), ctypes.byref(gout), geoms,
                                                   1 if accumulate else 0, B.stream()),
                   "lsr_backward_preprocess_views")
    else:
        P = st0.fin.P
        expect = 0
        for r0, r1 in row_chunks:
            if r0 != expect or r1 < r0 or r1 > P:
                raise ValueError(f"row_chunks must tile [0, {P}) in order, got {list(row_chunks)}")
            expect = r1
            part = {k: (v[r0:r1] if v is not None else None) for k, v in g.items()}
            gc = _bwd_out(part, B)
            _lib.check(L.lsr_backward_preprocess_views_rows(n, s_arr, ctypes.byref(st0.fin), ctypes.byref(gc), geoms,
                                                            1 if accumulate else 0, r0, r1 - r0, B.stream()),
                       "lsr_backward_preprocess_views_rows")
            if on_rows is not None:
                on_rows(r0, r1)
        if expect != P:
            raise ValueError(f"row_chunks must tile [0, {P}) in order, got {list(row_chunks)}")
    return g


def _grad_buffers(state, out, accumulate, need):
    inp = state.inputs
    device = inp["means3D"].device
    P, M, C = state.fin.P, state.fin.M, state.fin.C

    def buf(name, shape, wanted=True):
        if not wanted:
            return None
        if out is not None and name in out and out[name] is not None:
            return out[name]
        return torch.zeros(shape, dtype=torch.float32, device=device) if accumulate else \
            torch.empty(shape, dtype=torch.float32, device=device)

    return dict(
        means3D=buf("means3D", (P, 3), need.get("means3D", True)),
        means2D=buf("means2D", (P, 3), need.get("means2D", True)),
        colors=buf("colors", (P, 3), need.get("colors", True)),
        language_feature=buf("language_feature", (P, C), need.get("language_feature", True) and C > 0),
        opacities=buf("opacities", (P, 1), need.get("opacities", True)),
        cov3D=buf("cov3D", (P, 6), need.get("cov3D", True) and inp["cov3D_precomp"] is not None),
        sh=buf("sh", (P, max(M, 1), 3), need.get("sh", True) and M > 0),
        scales=buf("scales", (P, 3), need.get("scales", True) and inp["scales"] is not None),
        rotations=buf("rotations", (P, 4), need.get("rotations", True) and inp["rotations"] is not None),
    )


def _bwd_in(state, grad_color, grad_lang, grad_depth, deterministic=False):
    """A view's upstream gradients as fp32 contiguous tensors (zeros for a missing colour gradient;
    the language gradient only when C > 0) and the lsr_bwd_in over them: ((gc, gl, gd), gin).  The
    caller keeps the tensors alive until the backward is enqueued."""
    device = state.inputs["means3D"].device
    H, W = state.settings.c.image_height, state.settings.c.image_width
    gc = grad_color.detach().to(torch.float32).contiguous() if grad_color is not None else \
        torch.zeros(3, H, W, dtype=torch.float32, device=device)
    gl = grad_lang.detach().to(torch.float32).contiguous() if (grad_lang is not None and state.fin.C > 0) else None
    gd = grad_depth.detach().to(torch.float32).contiguous() if grad_depth is not None else None
    B = _lib.Boundary(device)
    gin = _lib.BwdIn()
    gin.dL_dout_color, gin.dL_dout_language_feature = B.ptr(gc, "grad_color"), B.opt(gl, "grad_lang")
    gin.dL_dout_depth = B.opt(gd, "grad_depth")
    gin.deterministic = 1 if deterministic else 0
    return (gc, gl, gd), gin


def _bwd_in_views(states, grad_colors, grad_langs, grad_depths):
    """_bwd_in per view (grad_langs / grad_depths may be None): ([kept tensors], [lsr_bwd_in])."""
    n = len(states)
    grad_langs, grad_depths = grad_langs or [None] * n, grad_depths or [None] * n
    pairs = [_bwd_in(s, grad_colors[v], grad_langs[v], grad_depths[v]) for v, s in enumerate(states)]
    return [k for k, _ in pairs], [gi for _, gi in pairs]


def _bwd_out(g, B):
    gout = _lib.BwdOut()
    for field, name in (("dL_dmeans3D", "means3D"), ("dL_dmeans2D", "means2D"), ("dL_dcolors", "colors"),
                        ("dL_dlanguage_feature", "language_feature"), ("dL_dopacity", "opacities"),
                        ("dL_dcov3D", "cov3D"), ("dL_dsh", "sh"), ("dL_dscales", "scales"),
                        ("dL_drotations", "rotations")):
        setattr(gout, field, B.opt(g[name], name))
    return gout


def _language_image_and_shapes(raster_settings, color, lang, lang_in, sh, opacities):
    """What both autograd functions keep of a view's forward: its language image (zeros when the
    language channels are off) and the input shapes the backward restores."""
    if not raster_settings.include_feature and lang_in is not None and lang_in.numel() > 0:
        # base stages: the caller passes zeros [P, hiddendim] and discards the output
        lang = torch.zeros((lang_in.shape[-1],) + tuple(color.shape[1:]), dtype=color.dtype, device=color.device)
    return lang, dict(sh=None if sh is None else sh.shape, opacities=opacities.shape,
                      lang=None if lang_in is None else lang_in.shape)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, language_feature_precomp, opacities, scales, rotations,
                cov3Ds_precomp, raster_settings):
        color, lang, radii, depth, state = forward_native(
            raster_settings, means3D, opacities, shs=sh, colors_precomp=colors_precomp,
            language_feature=language_feature_precomp if raster_settings.include_feature else None,
            scales=scales, rotations=rotations, cov3D_precomp=cov3Ds_precomp)
        lang, ctx.shapes = _language_image_and_shapes(raster_settings, color, lang, language_feature_precomp, sh,
                                                      opacities)
        ctx.state = state
        ctx.include_feature = raster_settings.include_feature
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        return color, lang, radii, depth

    @staticmethod
    def backward(ctx, grad_color, grad_lang, grad_radii, grad_depth):
        return _raster_backward(ctx.state, ctx.shapes, ctx.include_feature, ctx.needs_input_grad[:9], grad_color,
                                grad_lang, grad_depth) + (None,)


def _raster_backward(st, shp, include_feature, ng, grad_color, grad_lang, grad_depth):
    """The 9 input gradients of one view's rasterization (means3D, means2D, sh, colors_precomp,
    language_feature_precomp, opacities, scales, rotations, cov3D_precomp); ng: which are needed."""
    need = dict(means3D=ng[0], means2D=ng[1], sh=ng[2], colors=True, language_feature=ng[4], opacities=ng[5],
                scales=ng[6], rotations=ng[7], cov3D=ng[8])
    # torch.use_deterministic_algorithms(True) selects the fixed-order reduction (bitwise
    # reproducible gradients, lsr_backward's deterministic mode) instead of float atomics
    g = backward_native(st, grad_color, grad_lang if include_feature else None, grad_depth, need=need,
                        deterministic=torch.are_deterministic_algorithms_enabled())

    def like(t, shape):
        return None if (t is None or shape is None) else t.reshape(shape)

    grad_lang_in = None
    if ng[4] and shp["lang"] is not None and len(shp["lang"]) > 0:
        if g["language_feature"] is not None:
            grad_lang_in = g["language_feature"].reshape(shp["lang"])
        else:
            grad_lang_in = torch.zeros(shp["lang"], dtype=torch.float32, device=st.inputs["means3D"].device)
    return (g["means3D"] if ng[0] else None,
            g["means2D"] if ng[1] else None,
            like(g["sh"], shp["sh"]) if ng[2] else None,
            g["colors"] if ng[3] else None,
            grad_lang_in,
            like(g["opacities"], shp["opacities"]) if ng[5] else None,
            g["scales"] if ng[6] else None,
            g["rotations"] if ng[7] else None,
            g["cov3D"] if ng[8] else None)


class _RasterizeViews(torch.autograd.Function):
    """_RasterizeGaussians for several views with their own Gaussians (a batch's deformed copies,
    gaussian_scene.render_views): every view's preprocess is enqueued first with its instance count
    deferred, then each view is binned and composited, so the host waits on view v's count while the
    device runs the later views' preprocesses (one stream synchronisation per view in a row before:
    the device idled through each).  Same kernels per view, same results; per-view backward."""

    @staticmethod
    def forward(ctx, settings_list, *flat):
        pfs = []
        for v, rs in enumerate(settings_list):
            m3, _, sh, cp, lang, op, sc, rot, cov = flat[9 * v:9 * v + 9]
            pfs.append(preprocess_native(rs, m3, op, shs=sh, colors_precomp=cp,
                                         language_feature=lang if rs.include_feature else None, scales=sc,
                                         rotations=rot, cov3D_precomp=cov, defer_count=True))
        outs, radii_all = [], []
        ctx.views = []
        for v, (rs, pf) in enumerate(zip(settings_list, pfs)):
            color, lang, radii, depth, state = render_native(pf)
            lang, shapes = _language_image_and_shapes(rs, color, lang, flat[9 * v + 4], flat[9 * v + 2],
                                                      flat[9 * v + 5])
            ctx.views.append((state, shapes, rs.include_feature))
            outs += [color, lang, radii, depth]
            radii_all.append(radii)
        ctx.mark_non_differentiable(*radii_all)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        res = []
        for v, (state, shapes, include_feature) in enumerate(ctx.views):
            gc, gl, _, gd = grads[4 * v:4 * v + 4]
            res.extend(_raster_backward(state, shapes, include_feature, ctx.needs_input_grad[1 + 9 * v:10 + 9 * v],
                                        gc, gl, gd))
        return (None,) + tuple(res)


def rasterize_views(settings_list, views):
    """GaussianRasterizer forward for several views, each with its own inputs: views[v] =
    dict(means3D=, means2D=, shs=, colors_precomp=, language_feature_precomp=, opacities=, scales=,
    rotations=, cov3D_precomp=).  Returns [(color, language_feature, radii, depth)] per view
    (_RasterizeViews: the views' preprocesses enqueued ahead of their count waits)."""
    flat = []
    for rs, kw in zip(settings_list, views):
        if (kw.get("shs") is None) == (kw.get("colors_precomp") is None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((kw.get("scales") is None or kw.get("rotations") is None) == (kw.get("cov3D_precomp") is None)):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        flat += [kw["means3D"], kw["means2D"], kw.get("shs"), kw.get("colors_precomp"),
                 kw.get("language_feature_precomp"), kw["opacities"], kw.get("scales"), kw.get("rotations"),
                 kw.get("cov3D_precomp")]
    out = _RasterizeViews.apply(list(settings_list), *flat)
    return [tuple(out[4 * v:4 * v + 4]) for v in range(len(settings_list))]


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, language_feature_precomp, opacities, scales, rotations,
                        cov3Ds_precomp, raster_settings):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, language_feature_precomp, opacities,
                                     scales, rotations, cov3Ds_precomp, raster_settings)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            rs = self.raster_settings
            pos = _f32(positions, positions.device)
            view = _f32(rs.viewmatrix, positions.device).reshape(-1)
            proj = _f32(rs.projmatrix, positions.device).reshape(-1)
            out = torch.empty(pos.shape[0], dtype=torch.uint8, device=positions.device)
            L = _lib.load()
            B = _lib.Boundary(_check_device(positions))
            _lib.check(L.lsr_mark_visible(pos.shape[0], B.ptr(pos, "positions"), B.ptr(view, "viewmatrix"),
                                          B.ptr(proj, "projmatrix"), B.ptr(out, "out", torch.uint8), B.stream()),
                       "lsr_mark_visible")
            return out.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, language_feature_precomp=None,
                scales=None, rotations=None, cov3D_precomp=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        empty = torch.Tensor([])
        return rasterize_gaussians(means3D, means2D, shs if shs is not None else empty,
                                   colors_precomp if colors_precomp is not None else empty,
                                   language_feature_precomp if language_feature_precomp is not None else empty,
                                   opacities, scales if scales is not None else empty,
                                   rotations if rotations is not None else empty,
                                   cov3D_precomp if cov3D_precomp is not None else empty, rs)
