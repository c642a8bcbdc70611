"""Generate tests/golden/image_loss_golden.npz (and image_loss_golden_c.npz): the REFERENCE's image loss
terms on seeded inputs, run where a checkout of the reference is at hand (no test reads it).  The fixture
is data: the seed, a checksum of the regenerated inputs, the window's values and the reference's results.

What runs is the reference's own code, unchanged, on the CPU: utils.loss_utils.ssim and l1_loss
(utils/loss_utils.py:20-21,29-69; `lpips`, which the module imports and these never call, is registered as
an empty module) and utils.image_utils.psnr (utils/image_utils.py:17-38), on the views stacked to
[V, C, H, W] with the ground truth gt[:, :C], with autograd's gradients of l1_loss and of ssim towards the
images.  Everything runs in float64 (the stored results; the reference's window keeps its float32 values,
cast up) and again in float32: the float32 run's max abs error against float64 is stored beside each
result, and the tests bound the native gradient's error by a multiple of it.

Inputs: tests/image_loss_cases.py, shared with the tests; what it asserts of them (no |x - gt| < 1e-3
outside the x == gt patch) holds here too, so no test needs an exclusion list.  The ssim gradient of case c
(972 KB of float64) goes to a file of its own, each file staying under the repository's 1 MiB limit.

    python tests/golden/make_image_loss_golden.py <path of the reference checkout>
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "image_loss_golden.npz")

sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_loss_cases as ic  # noqa: E402


def reference_modules(ref):
    sys.modules.setdefault("lpips", types.ModuleType("lpips"))
    sys.path.insert(0, ref)
    from utils import image_utils, loss_utils
    return loss_utils, image_utils


def run(loss_utils, image_utils, x, gt, dtype):
    out = {}
    gt = torch.from_numpy(gt).to(dtype)
    for name, fn in (("l1", loss_utils.l1_loss), ("ssim", loss_utils.ssim)):
        xx = torch.from_numpy(x).to(dtype).requires_grad_(True)
        value = fn(xx, gt)
        value.backward()
        out[name] = value.detach().numpy()
        out[name + "_grad"] = xx.grad.numpy()
    xx = torch.from_numpy(x).to(dtype)
    out["ssim_view"] = loss_utils.ssim(xx, gt, size_average=False).numpy()
    out["psnr_view"] = image_utils.psnr(xx, gt).numpy()
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    loss_utils, image_utils = reference_modules(sys.argv[1])
    window = loss_utils.gaussian(11, 1.5)
    assert window.dtype == torch.float32 and window.shape == (11,)
    store = {"seed": np.int64(ic.FIXTURE_SEED), "window": window.numpy()}
    extra = {f: {} for f in ic.GRAD_FILE_OF.values()}
    for name, (V, C, H, W, Cg) in ic.CASES.items():
        x, gt_full = ic.inputs(name)
        gt = np.ascontiguousarray(gt_full[:, :C])
        r64 = run(loss_utils, image_utils, x, gt, torch.float64)
        r32 = run(loss_utils, image_utils, x, gt, torch.float32)
        p = name + "_"
        store[p + "inputs_sha256"] = np.array(ic.checksum([x, gt_full]))
        for k, v64 in r64.items():
            assert v64.dtype == (np.float32 if k == "psnr_view" else np.float64), (k, v64.dtype)
            assert r32[k].dtype == np.float32
            dest = extra[ic.GRAD_FILE_OF[name]] if (k == "ssim_grad" and name in ic.GRAD_FILE_OF) else store
            dest[p + k] = v64
            store[p + k + "_f32_err"] = np.float64(np.abs(r32[k].astype(np.float64) - v64.astype(np.float64)).max())
        assert r64["ssim_view"].shape == (V,) and r64["psnr_view"].shape == (V, 1)
        print(f"case {name}: l1 {float(r64['l1']):.9g} ssim {float(r64['ssim']):.9g}; float32 reference errors: "
              f"l1 {float(store[p + 'l1_f32_err']):.3g} ssim {float(store[p + 'ssim_f32_err']):.3g} "
              f"ssim gradient {float(store[p + 'ssim_grad_f32_err']):.3g} "
              f"(max |gradient| {np.abs(r64['ssim_grad']).max():.3g})")
    np.savez_compressed(OUT, **store)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    for f, arrays in extra.items():
        path = os.path.join(HERE, f)
        np.savez_compressed(path, **arrays)
        print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
