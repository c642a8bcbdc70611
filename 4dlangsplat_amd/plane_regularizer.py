"""The HexPlane regularisers of the training loop with their gradient (include/lsr_plane_reg.h,
csrc/plane_reg.hip).

  compute_plane_smoothness(t)                                    scene/regulation.py:22-28
  GaussianModel._plane_regulation / _time_regulation / _l1_regulation,
  compute_regulation(time_smoothness_weight, l1_time_planes_weight, plane_tv_weight)
                                                                 scene/gaussian_model.py:763-802
  the gate `hyper.time_smoothness_weight != 0`                   train.py:331-333

Per plane t [1, C, H, W] (grid.grids.{s}.{ci}; pairs xy, xz, xt, yz, yt, zt, so ci 0, 1, 3 are the spatial
planes and ci 2, 4, 5 the time planes):
  d2[c, i, w] = t[c, i+2, w] - 2 t[c, i+1, w] + t[c, i, w]      i in [0, H - 2)
  smooth = sum d2^2 / (C (H - 2) W)         d smooth / d t[c, j, w] = 2 / (C (H - 2) W) (d2[j-2] - 2 d2[j-1] + d2[j])
  l1     = sum |1 - t| / (C H W)            d l1 / d t = -sign(1 - t) / (C H W), sign(0) = 0
  total  = plane_tv_weight sum_{spatial} smooth + time_smoothness_weight sum_{time} smooth
           + l1_time_planes_weight sum_{time} l1

One fused call (two launches) takes every plane of the field, returns the terms and the total and writes or
accumulates the gradient; float32 contiguous CUDA planes take it.  Anything else (CPU, float64) evaluates
the same formulas as torch ops in the input's dtype with the gradient from the closed form, which is also
what the tests hold against the reference's results.
"""
from __future__ import annotations

from typing import Mapping, Optional, Sequence, Tuple

import torch

SPATIAL_PLANES = (0, 1, 3)
TIME_PLANES = (2, 4, 5)
MAX_NATIVE_PLANES = 24
# arguments/__init__.py:93-95 (ModelHiddenParams)
DEFAULT_TIME_SMOOTHNESS_WEIGHT = 0.01
DEFAULT_L1_TIME_PLANES = 0.0001
DEFAULT_PLANE_TV_WEIGHT = 0.0001


class PlaneReg:
    """The result of one call: total (the weighted sum, a device scalar in the planes' dtype), terms
    [n_planes, 2] (the unweighted {smooth, l1} of every plane, scale-major; float64 from the kernel) and the
    three unweighted sums the reference logs, taken from terms when first read: plane_smooth (spatial planes'
    smooth), time_smooth (time planes' smooth), time_l1 (time planes' l1)."""

    def __init__(self, total: torch.Tensor, terms: torch.Tensor, total64: Optional[torch.Tensor] = None):
        self.total, self.terms = total, terms
        self._total64 = total64
        self._sums = None

    @property
    def total64(self) -> torch.Tensor:
        """The total in float64: the kernel's before its rounding to float32, else total cast up."""
        return self.total.double() if self._total64 is None else self._total64

    def _named(self, i: int) -> torch.Tensor:
        if self._sums is None:
            t = self.terms.view(-1, 6, 2)
            sel = lambda cis, k: sum(t[:, ci, k].sum() for ci in cis) if t.shape[0] else t.new_zeros(())  # noqa: E731
            self._sums = (sel(SPATIAL_PLANES, 0), sel(TIME_PLANES, 0), sel(TIME_PLANES, 1))
        return self._sums[i]

    plane_smooth = property(lambda self: self._named(0))
    time_smooth = property(lambda self: self._named(1))
    time_l1 = property(lambda self: self._named(2))

    def __iter__(self):
        return iter((self.total, self.plane_smooth, self.time_smooth, self.time_l1, self.terms))

    def __repr__(self):
        return f"PlaneReg(total={self.total!r}, terms={tuple(self.terms.shape)})"


def plane_weights(weights: Sequence[float], ci: int) -> Tuple[float, float]:
    """(w_smooth, w_l1) of plane ci under weights = (time_smoothness_weight, l1_time_planes_weight,
    plane_tv_weight)."""
    tsw, l1w, tvw = (float(w) for w in weights)
    return (tvw, 0.0) if ci in SPATIAL_PLANES else (tsw, l1w)


def _flatten(planes, what: str = "planes"):
    scales = [list(s) for s in planes]
    if any(len(s) != 6 for s in scales):
        raise ValueError(f"plane regularisers: {what} must be six planes (xy, xz, xt, yz, yt, zt) per scale")
    return [p for s in scales for p in s]


def _check(flat, weights, gflat):
    if len(tuple(weights)) != 3:
        raise ValueError("plane regularisers: weights = (time_smoothness_weight, l1_time_planes_weight, "
                         "plane_tv_weight)")
    for i, t in enumerate(flat):
        if t.dim() != 4 or t.shape[0] != 1 or t.numel() == 0:
            raise ValueError(f"plane regularisers: plane {i} must be [1, C, H, W], got {tuple(t.shape)}")
        if plane_weights(weights, i % 6)[0] != 0 and t.shape[2] < 3:
            raise ValueError(f"plane regularisers: plane {i} has H = {t.shape[2]}; a second difference needs H >= 3 "
                             "(the reference's mean over nothing is NaN)")
        if gflat is not None and (gflat[i].shape != t.shape or gflat[i].dtype != t.dtype
                                  or gflat[i].device != t.device):
            raise ValueError(f"plane regularisers: gradient {i} must match its plane's shape, dtype and device")


def native_eligible(flat, gflat=None) -> bool:
    """Whether the HIP path is taken: at most 24 float32 contiguous CUDA planes on one device (and gradient
    buffers of the same kind)."""
    if not flat or len(flat) > MAX_NATIVE_PLANES:
        return False
    if not flat[0].is_cuda:
        return False
    from diff_gaussian_rasterization import _lib
    B = _lib.Boundary(flat[0].device)
    return all(B.ok(t) for t in list(flat) + list(gflat or ())) and all(t.numel() <= 0x7fffffff for t in flat)


def plane_terms_torch(t: torch.Tensor, need_grad: bool = True):
    """(smooth, l1, d smooth / d t, d l1 / d t) of one plane as torch ops in t's dtype; the gradients from
    the closed form (None unless need_grad); smooth and its gradient are 0 where H < 3."""
    t = t.detach()
    _, C, H, W = t.shape
    one = 1 - t
    l1 = one.abs().sum() / (C * H * W)
    g_l1 = -torch.sign(one) / (C * H * W) if need_grad else None
    if H < 3:
        return t.new_zeros(()), l1, (torch.zeros_like(t) if need_grad else None), g_l1
    n_s = C * (H - 2) * W
    d2 = t[:, :, 2:] - 2 * t[:, :, 1:-1] + t[:, :, :-2]
    smooth = (d2 * d2).sum() / n_s
    g_s = None
    if need_grad:
        g_s = torch.zeros_like(t)
        g_s[:, :, 2:] += d2
        g_s[:, :, 1:-1] -= 2 * d2
        g_s[:, :, :-2] += d2
        g_s *= 2.0 / n_s
    return smooth, l1, g_s, g_l1


def regularize_planes_torch(planes, weights, grads=None, accumulate: bool = True) -> PlaneReg:
    """regularize_planes as torch ops on whatever device and dtype the planes have."""
    flat = _flatten(planes)
    gflat = _flatten(grads, "grads") if grads is not None else None
    _check(flat, weights, gflat)
    tsw, l1w, tvw = (float(w) for w in weights)
    rows, sums = [], [0, 0, 0]
    with torch.no_grad():
        for i, t in enumerate(flat):
            smooth, l1, g_s, g_l1 = plane_terms_torch(t, gflat is not None)
            rows.append(torch.stack([smooth, l1]))
            w_s, w_l1 = plane_weights(weights, i % 6)
            if i % 6 in SPATIAL_PLANES:
                sums[0] = sums[0] + smooth
            else:
                sums[1], sums[2] = sums[1] + smooth, sums[2] + l1
            if gflat is not None:
                g = w_s * g_s + w_l1 * g_l1
                if accumulate:
                    gflat[i] += g
                else:
                    gflat[i].copy_(g)
        if not flat:
            z = torch.zeros(())
            return PlaneReg(z, torch.zeros(0, 2))
        total = tvw * sums[0] + tsw * sums[1] + l1w * sums[2]
        return PlaneReg(total, torch.stack(rows))


def _native(flat, weights, gflat, accumulate: bool) -> PlaneReg:
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    n, dev = len(flat), flat[0].device
    B = _lib.Boundary(dev)
    desc = (_lib.PlaneDesc * n)()
    for i, t in enumerate(flat):
        d = desc[i]
        d.t = B.ptr(t, f"plane {i}")
        d.grad = B.ptr(gflat[i], f"gradient {i}") if gflat is not None else None
        _, d.C, d.H, d.W = t.shape
        d.w_smooth, d.w_l1 = plane_weights(weights, i % 6)
    nbytes = int(L.lsr_plane_reg_workspace_bytes(n, desc))
    if nbytes < 0:
        raise ValueError(L.lsr_last_error().decode())
    nbytes = (nbytes + 15) // 16 * 16
    # one allocation: the workspace, then terms [n, 2] float64, total64, total
    buf = torch.empty(nbytes + 16 * n + 16, dtype=torch.uint8, device=dev)
    terms = buf[nbytes:nbytes + 16 * n].view(torch.float64).view(n, 2)
    total64 = buf[nbytes + 16 * n:nbytes + 16 * n + 8].view(torch.float64)
    total = buf[nbytes + 16 * n + 8:nbytes + 16 * n + 12].view(torch.float32)
    with torch.cuda.device(dev):
        _lib.check(L.lsr_plane_reg(n, desc, int(bool(accumulate)), B.ptr(buf, "workspace", torch.uint8),
                                   B.ptr(terms, "terms", torch.float64), B.ptr(total, "total"),
                                   B.ptr(total64, "total64", torch.float64), B.stream()), "lsr_plane_reg")
    return PlaneReg(total.view(()), terms, total64.view(()))


def regularize_planes(planes, weights, grads=None, accumulate: bool = True) -> PlaneReg:
    """The regularisers of a field's planes and, with grads, their gradient.
    planes: one sequence of six planes [1, C, H, W] per scale; weights = (time_smoothness_weight,
    l1_time_planes_weight, plane_tv_weight), compute_regulation's argument order; grads: buffers of the
    planes' layout that receive weights . gradient, added to what they hold (accumulate) or overwritten; None:
    the loss only.  Returns PlaneReg; total is a device scalar and nothing synchronises with the host."""
    flat = _flatten(planes)
    gflat = _flatten(grads, "grads") if grads is not None else None
    _check(flat, weights, gflat)
    if native_eligible(flat, gflat):
        return _native([t.detach() for t in flat], weights, gflat, accumulate)
    return regularize_planes_torch(planes, weights, grads, accumulate)


def _planes_of(planes_or_field):
    """The planes of a DeformationField (its grid.grids.{s}.{ci}) or the nested sequence itself (a list of
    lists, or a reference checkout's deformation_net.grid.grids: a ModuleList of ParameterLists)."""
    p = getattr(planes_or_field, "p", None)
    if isinstance(p, Mapping):
        return [[p[f"grid.grids.{s}.{ci}"] for ci in range(6)] for s in range(len(planes_or_field.multires))]
    return [list(s) for s in planes_or_field]


class _ComputeRegulation(torch.autograd.Function):
    """Forward: the one fused call, which also leaves the gradient in a saved buffer; backward: grad_output
    times that buffer, per plane."""

    @staticmethod
    def forward(ctx, weights, *flat):
        planes = [list(flat[i:i + 6]) for i in range(0, len(flat), 6)]
        det = [t.detach() for t in flat]
        if native_eligible(det):
            # the gradients as views of one buffer, each 256-byte aligned
            offs, o = [], 0
            for t in det:
                offs.append(o)
                o += (t.numel() + 63) // 64 * 64
            gbuf = torch.empty(o, dtype=torch.float32, device=det[0].device)
            grads = [gbuf[a:a + t.numel()].view(t.shape) for a, t in zip(offs, det)]
        else:
            grads = [torch.empty_like(t) for t in det]
        res = regularize_planes(planes, weights, [grads[i:i + 6] for i in range(0, len(grads), 6)], accumulate=False)
        ctx.save_for_backward(*grads)
        return res.total

    @staticmethod
    def backward(ctx, g):
        return (None,) + tuple(g * x for x in ctx.saved_tensors)


def compute_regulation(planes_or_field, time_smoothness_weight: float, l1_time_planes_weight: float,
                       plane_tv_weight: float) -> torch.Tensor:
    """GaussianModel.compute_regulation (scene/gaussian_model.py:801-802) on a field's planes: the scalar
    total inside autograd, its gradient towards every plane that requires one."""
    planes = _planes_of(planes_or_field)
    flat = _flatten(planes)
    weights = (float(time_smoothness_weight), float(l1_time_planes_weight), float(plane_tv_weight))
    _check(flat, weights, None)
    return _ComputeRegulation.apply(weights, *flat)


def plane_reg_from_hidden(hidden) -> Optional[Tuple[float, float, float]]:
    """(time_smoothness_weight, l1_time_planes_weight, plane_tv_weight) of a ModelHiddenParams dict or
    object (its l1_time_planes is the second), the reference's defaults where absent
    (arguments/__init__.py:93-95); None when time_smoothness_weight == 0, the gate of train.py:331."""
    h = hidden if isinstance(hidden, Mapping) else vars(hidden)
    tsw = float(h.get("time_smoothness_weight", DEFAULT_TIME_SMOOTHNESS_WEIGHT))
    l1w = float(h.get("l1_time_planes", DEFAULT_L1_TIME_PLANES))
    tvw = float(h.get("plane_tv_weight", DEFAULT_PLANE_TV_WEIGHT))
    if tsw == 0:
        return None
    return tsw, l1w, tvw
