"""The photometric loss of the training loop with its D-SSIM term, and the image metrics that share its
kernel (include/lsr_train.h: lsr_image_loss_views / _backward, csrc/image_loss.hip).

  ssim(img1, img2, window_size=11, size_average=True)     utils/loss_utils.py:39-69
  psnr(img1, img2, mask=None)                             utils/image_utils.py:17-38
  image_loss_views(images, gts, lambda_dssim)             train.py:284,335-337:
      loss = l1_loss(images, gts[:, :3]) + lambda_dssim * (1 - ssim(images, gts[:, :3]))

One fused forward reads every view's render and ground truth once and returns the L1, the SSIM and the
squared error (per view and over all views); one fused backward takes both upstream gradients.  The
native path runs when native_eligible(); anything else (CPU, float64, more than 8 views, another window
size, a ground truth that wants a gradient) evaluates the same formulas as torch ops in the input's
dtype, which is also what the tests hold against the reference's results.

The window: w[i] = exp(-(i - n // 2)^2 / (2 sigma^2)) / sum, sigma = 1.5, evaluated in float32; the 2-D
window is its float32 outer product (so the float64 evaluation uses float32 window values cast up, as
the reference's does).  Zero padding of n // 2; channels are independent planes; C1 = 0.01^2, C2 = 0.03^2.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

MAX_NATIVE_VIEWS = 8
NATIVE_WINDOW = 11
SIGMA = 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2
# window_1d(11) as float32 arithmetic gives it; csrc/image_loss.hip holds the same 11 values
WINDOW_11 = (0.001028380123898387, 0.0075987582094967365, 0.036000773310661316, 0.10936068743467331,
             0.21300552785396576, 0.26601171493530273, 0.21300552785396576, 0.10936068743467331,
             0.036000773310661316, 0.0075987582094967365, 0.001028380123898387)


def window_1d(window_size: int = NATIVE_WINDOW) -> torch.Tensor:
    """The normalised Gaussian taps, float32 [window_size]."""
    if window_size == NATIVE_WINDOW:
        return torch.tensor(WINDOW_11, dtype=torch.float32)
    half = window_size // 2
    g = torch.tensor([math.exp(-((i - half) ** 2) / (2.0 * SIGMA ** 2)) for i in range(window_size)],
                     dtype=torch.float32)
    return g / g.sum()


def _window_2d(window_size: int, channels: int, like: torch.Tensor) -> torch.Tensor:
    w = window_1d(window_size)
    w2 = torch.outer(w, w)                                    # float32 products, then cast
    return w2.to(device=like.device, dtype=like.dtype).expand(channels, 1, window_size, window_size).contiguous()


def ssim_map(x: torch.Tensor, y: torch.Tensor, window_size: int = NATIVE_WINDOW) -> torch.Tensor:
    """The per-pixel SSIM of [B, C, H, W] (or [C, H, W]) images as torch ops in x's dtype."""
    channels = x.shape[-3]
    win = _window_2d(window_size, channels, x)
    blur = lambda t: torch.nn.functional.conv2d(t, win, padding=window_size // 2, groups=channels)  # noqa: E731
    mu_x, mu_y = blur(x), blur(y)
    mu_xx, mu_yy, mu_xy = mu_x * mu_x, mu_y * mu_y, mu_x * mu_y
    var_x, var_y, cov = blur(x * x) - mu_xx, blur(y * y) - mu_yy, blur(x * y) - mu_xy
    return ((2 * mu_xy + C1) * (2 * cov + C2)) / ((mu_xx + mu_yy + C1) * (var_x + var_y + C2))


def _psnr_of_mse(mse: torch.Tensor) -> torch.Tensor:
    return 20 * torch.log10(1.0 / torch.sqrt(mse.float()))   # the reference evaluates this in float32


def _fallback(images: Sequence[torch.Tensor], gt: torch.Tensor, window_size: int):
    """(l1, ssim, stats [V, 3]) of the views against gt [V, C, H, W] as torch ops in the images' dtype."""
    x = torch.stack(list(images))
    y = gt.to(device=x.device, dtype=x.dtype)
    d = x - y
    m = ssim_map(x, y, window_size)
    with torch.no_grad():
        stats = torch.stack([d.abs().flatten(1).mean(1), m.flatten(1).mean(1), (d * d).flatten(1).mean(1)], dim=1)
    return d.abs().mean(), m.mean(), stats


def native_eligible(images: Sequence[torch.Tensor], gt: torch.Tensor, window_size: int = NATIVE_WINDOW) -> bool:
    """Whether the HIP path is taken: 1..8 float32 CUDA images of one [C, H, W] shape on one device, each
    contiguous; window_size 11; gt (the caller's gts[:, :3]) float32 [V, C, H, W] on that device, not requiring
    grad, each view's slice contiguous (the views may be any distance >= C H W apart)."""
    images = list(images)
    if window_size != NATIVE_WINDOW or not 1 <= len(images) <= MAX_NATIVE_VIEWS:
        return False
    x0 = images[0]
    if not (x0.is_cuda and x0.dim() == 3 and x0.numel() > 0):
        return False
    from diff_gaussian_rasterization import _lib
    B = _lib.Boundary(x0.device)   # the test _ImageLossViews' addresses are taken under
    if not all(B.ok(x) and x.shape == x0.shape for x in images):
        return False
    if gt.requires_grad or gt.dim() != 4 or gt.shape[0] != len(images) or gt.shape[1:] != x0.shape:
        return False
    if not all(B.ok(y) for y in gt):
        return False
    return len(images) == 1 or gt.stride(0) >= x0.numel()


class _ImageLossViews(torch.autograd.Function):
    """lsr_image_loss_views / _backward over the views' renders, unstacked: two launches forward, one
    backward that receives the gradients of both the L1 and the SSIM; between them the workspace (the
    forward's three per-pixel partial-derivative maps) is kept.  Returns (l1, ssim, stats [V, 3])."""

    @staticmethod
    def forward(ctx, gt, *images):
        from diff_gaussian_rasterization import _lib
        L = _lib.load()
        V, (C, H, W) = len(images), images[0].shape
        dev = images[0].device
        B = _lib.Boundary(dev)
        nbytes = int(L.lsr_image_loss_workspace_bytes(V, C, H, W))
        if nbytes < 0:
            raise ValueError(L.lsr_last_error().decode())
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        stats = torch.empty((V, 3), dtype=torch.float32, device=dev)
        totals = torch.empty(2, dtype=torch.float32, device=dev)
        stride = gt.stride(0) if V > 1 else C * H * W
        with torch.cuda.device(dev):
            _lib.check(L.lsr_image_loss_views(V, C, H, W, B.array(images, "images"), B.ptr(gt[0], "gt"), stride,
                                              B.ptr(stats, "stats"), B.ptr(totals, "totals"),
                                              B.ptr(ws, "workspace", torch.uint8), B.stream()), "lsr_image_loss_views")
        ctx.stride = stride
        ctx.set_materialize_grads(False)                 # an unused output's gradient arrives as None: NULL
        ctx.save_for_backward(gt, ws, *images)
        ctx.mark_non_differentiable(stats)
        l1, ss = totals.unbind(0)
        return l1, ss, stats

    @staticmethod
    def backward(ctx, g_l1, g_ssim, _g_stats):
        from diff_gaussian_rasterization import _lib
        gt, ws, *images = ctx.saved_tensors
        V, (C, H, W) = len(images), images[0].shape
        dev = images[0].device
        B = _lib.Boundary(dev)
        grads = [torch.empty_like(x) for x in images]
        keep = [None if g is None else g.to(device=dev, dtype=torch.float32).contiguous() for g in (g_l1, g_ssim)]
        with torch.cuda.device(dev):
            _lib.check(_lib.load().lsr_image_loss_views_backward(
                V, C, H, W, B.array(images, "images"), B.ptr(gt[0], "gt"), ctx.stride, B.opt(keep[0], "grad l1"),
                B.opt(keep[1], "grad ssim"), B.array(grads, "grads"), B.ptr(ws, "workspace", torch.uint8),
                B.stream()), "lsr_image_loss_views_backward")
        return (None,) + tuple(grads)


def loss_terms(images: Sequence[torch.Tensor], gt: torch.Tensor,
               window_size: int = NATIVE_WINDOW) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(l1, ssim, stats) of the views' [C, H, W] images against gt [V, C, H, W]: mean |x - y| and mean ssim_map
    over all views (both differentiable towards the images), and stats [V, 3] = per view mean |x - y|, mean
    ssim_map, mean (x - y)^2 (no gradient)."""
    images = list(images)
    if not images:
        raise ValueError("image loss: at least one view")
    shape = tuple(images[0].shape)
    if len(shape) != 3 or any(tuple(x.shape) != shape or x.dtype != images[0].dtype or x.device != images[0].device
                              for x in images):
        raise ValueError("image loss: the views' images must share one [C, H, W] shape, dtype and device")
    if gt.dim() != 4 or gt.shape[0] != len(images) or tuple(gt.shape[1:]) != shape:
        raise ValueError(f"image loss: ground truth {tuple(gt.shape)} for {len(images)} images of {shape}")
    if native_eligible(images, gt, window_size):
        return _ImageLossViews.apply(gt, *images)
    return _fallback(images, gt, window_size)


def image_loss_views(images: Sequence[torch.Tensor], gts: torch.Tensor, lambda_dssim: float):
    """(loss, l1, ssim) with loss = l1 + lambda_dssim * (1 - ssim) over the views' renders [3, H, W] against
    gts[:, :3] (gts [V, 3 or more, H, W]), without stacking the renders; the gradient reaches the renders."""
    l1, ss, _ = loss_terms(images, gts[:, :3])
    return l1 + lambda_dssim * (1.0 - ss), l1, ss


def _as_views(img1: torch.Tensor, img2: torch.Tensor):
    if img1.shape != img2.shape or img1.dim() not in (3, 4):
        raise ValueError(f"expected two [C, H, W] or [B, C, H, W] images of one shape, got {tuple(img1.shape)} "
                         f"and {tuple(img2.shape)}")
    if img1.dim() == 3:
        return [img1], img2[None]
    return list(img1.unbind(0)), img2


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """Mean SSIM of img1 against img2 ([C, H, W] or [B, C, H, W]), differentiable towards img1.
    size_average=False: the per-image means [B] (no gradient on the native path; a single [C, H, W] image
    gives a 0-dim tensor, where the reference's chain of means raises)."""
    views, gt = _as_views(img1, img2)
    if size_average:
        return loss_terms(views, gt, window_size)[1]
    if native_eligible(views, gt, window_size):
        per_image = loss_terms(views, gt, window_size)[2][:, 1]
    else:
        x = torch.stack(views)
        per_image = ssim_map(x, gt.to(device=x.device, dtype=x.dtype), window_size).flatten(1).mean(1)
    return per_image[0] if img1.dim() == 3 else per_image


@torch.no_grad()
def psnr(img1: torch.Tensor, img2: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """20 log10(1 / sqrt(mse)) per leading index of img1, [B, 1] float32 (for a [C, H, W] image: per channel,
    as the reference's view(shape[0], -1) has it).  Without a mask the squared error comes from the fused
    kernel's stats where native_eligible().  With a mask (for a [3, H, W] image: the mask's non-zero pixels of
    every channel) it is torch ops, and yields what the reference's indexing yields: one value per selected
    element, the infinite ones dropped."""
    if mask is not None:
        a, b = img1.flatten(1), img2.flatten(1)
        keep = mask.flatten(1).repeat(3, 1) != 0
        a, b = a[keep], b[keep]
        mse = ((a - b) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)
        out = _psnr_of_mse(mse)
        return out[~torch.isinf(out)] if bool(torch.isinf(out).any()) else out
    if img1.dim() in (3, 4) and img1.shape == img2.shape:
        # a [C, H, W] image counts as C one-plane images
        views = list(img1.unbind(0)) if img1.dim() == 4 else [p[None] for p in img1.unbind(0)]
        gt = img2 if img2.dim() == 4 else img2[:, None]
        views = [v.contiguous() for v in views]
        if native_eligible(views, gt):
            return _psnr_of_mse(loss_terms(views, gt)[2][:, 2:3])
    mse = ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdim=True)
    return _psnr_of_mse(mse)
