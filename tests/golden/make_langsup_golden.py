"""Generate tests/golden/langsup_golden.npz: the REFERENCE's language supervision and 'lang' stage
loss on seeded inputs, run where a checkout of the reference is at hand (the GPU tests never read
it).  The fixture is data: the seeded files' contents, a checksum of the regenerated images, and
the reference's results.

What runs is the reference's own code, unchanged, on the CPU:
  * scene.cameras.Camera.get_language_feature (scene/cameras.py:69-118).  scene/cameras.py is loaded
    by file path (scene/__init__.py pulls in torchvision, absent here); the camera is made with
    Camera.__new__ and nn.Module.__init__, and colmap_id, image_height, image_width and cam_name are
    set by hand.  Its `.cuda()` on the results is the identity in this process, and its np.load is
    served from memory, which also records the file names it asks for.
  * utils.loss_utils.l1_loss and cos_loss (utils/loss_utils.py:20-27; `lpips`, which the module
    imports and these two never call, is registered as an empty module), combined as train.py:287-292
    does: lam * l1_loss(x * mask, gt * mask) (+ beta * cos_loss(x * mask, gt * mask)), over the views
    stacked to [V, C, H, W] and [V, 1, H, W], with autograd's gradient towards x.
Both losses run in float64 (the stored results) and again in float32: the float32 run's max abs error
against float64 is stored beside each result, and the tests bound the native error by a multiple of it.

Inputs (tests/langsup_cases.py, shared with the tests): (V = 2, C = 32, 19 x 37, S = 11) named by
the nerfies and the dynerf scheme, and (V = 1, C = 3, 5 x 300, S = 4).  Asserted here, so that no
test needs an exclusion list: no labelled element has |x - t| < 1e-3; no partly labelled row has
|a| or |b| below 1e-3; every map has -1 pixels, a fully unlabelled row, a constant row and S - 1.

    python tests/golden/make_langsup_golden.py <path of the reference checkout>
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "langsup_golden.npz")

sys.path.insert(0, os.path.join(ROOT, "tests"))
import langsup_cases as lc  # noqa: E402


def reference_modules(ref):
    sys.modules.setdefault("lpips", types.ModuleType("lpips"))
    sys.path.insert(0, ref)
    spec = importlib.util.spec_from_file_location("reference_cameras", os.path.join(ref, "scene", "cameras.py"))
    cameras = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cameras)
    from utils import loss_utils
    torch.Tensor.cuda = lambda self, *a, **k: self          # this process only: the reference calls .cuda()
    return cameras, loss_utils


class Files:
    """np.load for the reference: serves `contents` by suffix and records the stems asked for."""

    def __init__(self, cameras):
        self.contents, self.asked = {}, []
        cameras.np = types.SimpleNamespace(load=self.load)

    def load(self, path):
        stem, kind = path[:-6], path[-6:]
        if kind == "_s.npy":
            self.asked.append(stem)
        return self.contents[kind]


def camera(cameras, colmap_id, cam_name, H, W):
    cam = cameras.Camera.__new__(cameras.Camera)
    nn.Module.__init__(cam)
    cam.colmap_id, cam.cam_name, cam.image_height, cam.image_width = colmap_id, cam_name, H, W
    return cam


def losses(loss_utils, x, gt, mask, dtype):
    """{name: (loss, gradient [V, C, H, W])} of train.py:287-292 in `dtype`."""
    out = {}
    for name, with_cos in (("l1", False), ("cos", True)):
        xx = x.detach().clone().to(dtype).requires_grad_(True)
        a, b = xx * mask, gt.to(dtype) * mask
        loss = lc.LAM * loss_utils.l1_loss(a, b)
        if with_cos:
            loss = loss + lc.BETA * loss_utils.cos_loss(a, b)
        loss.backward()
        out[name] = (loss.detach().numpy(), xx.grad.numpy())
    return out


def check_maps(segs, S):
    for seg in segs.reshape(-1, *segs.shape[-2:]):
        rows_unlabelled = (seg == -1).all(axis=1)
        rows_constant = (seg == seg[:, :1]).all(axis=1) & (seg[:, 0] >= 0)
        assert (seg == -1).any() and rows_unlabelled.any() and rows_constant.any() and (seg == S - 1).any()
        assert seg.min() >= -1 and seg.max() < S


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    cameras, loss_utils = reference_modules(sys.argv[1])
    files = Files(cameras)
    store = dict(seed=np.int64(lc.FIXTURE_SEED), lam=np.float64(lc.LAM), beta=np.float64(lc.BETA))

    # the names the reference asks for
    files.contents = {"_s.npy": np.full((4, 2, 2), -1, np.int32), "_f.npy": np.zeros((1, 3), np.float32)}
    names = []
    for colmap_id, data_type, split, cam_name in lc.STEM_QUERIES:
        n = len(files.asked)
        got = camera(cameras, colmap_id, cam_name, 2, 2).get_language_feature("", 0, split=split, data_type=data_type)
        names.append(files.asked[n] if len(files.asked) > n else "")
        assert (got[0] is None) == (names[-1] == "")
    store["stems"] = np.array(names)

    for k, (V, C, H, W, S, level) in enumerate(lc.FIXTURE_CASES):
        inp = lc.fixture_inputs(k)
        check_maps(inp["segs"], S)
        gts, masks, stems = [], [], []
        for v, (colmap_id, data_type, split, cam_name) in enumerate(lc.FIXTURE_VIEWS[k]):
            files.contents = {"_s.npy": inp["segs"][v], "_f.npy": inp["tables"][v]}
            cam = camera(cameras, colmap_id, cam_name, H, W)
            per_level = [cam.get_language_feature("", lv, split=split, data_type=data_type) for lv in range(4)]
            stems.append(files.asked[-1])
            gts.append(torch.stack([g for g, _ in per_level]))
            masks.append(torch.stack([m for _, m in per_level]))
        gt_all, mask_all = torch.stack(gts), torch.stack(masks)          # [V, 4, C, H, W], [V, 4, 1, H, W]
        assert gt_all.dtype == torch.float32 and mask_all.dtype == torch.bool
        x = torch.from_numpy(inp["images"])
        gt, mask = gt_all[:, level], mask_all[:, level]
        a, b = (x * mask).double(), (gt * mask).double()
        assert not bool(((a - b).abs()[mask.expand_as(a)] < 1e-3).any()), "ambiguous sign"
        partly = mask.any(dim=-1)                                         # [V, 1, H]
        na, nb = a.norm(dim=-1)[partly.expand(V, C, H)], b.norm(dim=-1)[partly.expand(V, C, H)]
        assert float(na.min()) >= 1e-3 and float(nb.min()) >= 1e-3, "a nearly empty row"
        r64 = losses(loss_utils, x, gt, mask, torch.float64)
        r32 = losses(loss_utils, x, gt, mask, torch.float32)
        p = f"c{k}_"
        store.update({p + "segs": inp["segs"], p + "tables": inp["tables"], p + "level": np.int64(level),
                      p + "stems": np.array(stems), p + "images_sha256": np.array(lc.checksum([inp["images"]])),
                      # [V, 4, H, W, C]: the layout the reference gathers in (its result is the permuted view), which
                      # also compresses best
                      p + "gt_hwc": np.ascontiguousarray(gt_all.permute(0, 1, 3, 4, 2).numpy()),
                      p + "mask": mask_all.numpy()})
        for name in ("l1", "cos"):
            (l64, g64), (l32, g32) = r64[name], r32[name]
            assert l64.dtype == np.float64 and g64.dtype == np.float64 and g32.dtype == np.float32
            store.update({p + name + "_loss": l64, p + name + "_grad": g64,
                          p + name + "_loss_f32_err": np.float64(abs(float(l32) - float(l64))),
                          p + name + "_grad_f32_err": np.float64(np.abs(g32.astype(np.float64) - g64).max())})
            print(f"case {k} {name}: loss {float(l64):.9g}, float32 reference error: loss "
                  f"{float(store[p + name + '_loss_f32_err']):.3g}, gradient {float(store[p + name + '_grad_f32_err']):.3g} "
                  f"(max |gradient| {np.abs(g64).max():.3g})")
    np.savez_compressed(OUT, **store)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; stems {names}")


if __name__ == "__main__":
    main()
