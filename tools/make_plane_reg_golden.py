#!/usr/bin/env python3
"""Writes tests/golden/plane_reg.npz: what the REFERENCE's regularisers give on a small seeded field.

  python tools/make_plane_reg_golden.py /path/to/reference

The reference's scene/regulation.py is loaded by file path (importing its `scene` package pulls in
dependencies the regularisers do not need).  compute_plane_smoothness comes from that file; the three sums
and their weighting are restated from GaussianModel._plane_regulation / _time_regulation / _l1_regulation /
compute_regulation (scene/gaussian_model.py:763-802), which cannot be imported without a whole model, around
the reference's function: spatial planes 0, 1, 3; time planes 2, 4, 5; torch.abs(1 - plane).mean().

Stored: the float32 planes of a field with resolution [4, 5, 6, 7], multires [1, 2], 16 channels (spatial
planes U(0.1, 0.5), time planes 1 with half the entries perturbed: tests/plane_reg_cases.plane_values), and
in float64 from the reference's functions: terms [12, 2] (smooth and l1 per plane), the total for the weights
(1e-3, 1e-4, 2e-4) and its autograd gradient towards every plane.  Data only.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_reg_cases as pc  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    path = os.path.join(sys.argv[1], "scene", "regulation.py")
    spec = importlib.util.spec_from_file_location("reference_regulation", path)
    reg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(reg)
    rng = np.random.default_rng(20240613)
    shapes = pc.plane_shapes(pc.GOLDEN_RES, pc.GOLDEN_MULTIRES)
    planes32 = [[pc.plane_values(sh, "time" if ci in pc.TIME else "spatial", rng) for ci, sh in enumerate(scale)]
                for scale in shapes]
    planes = [[torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in scale] for scale in planes32]
    tsw, l1w, tvw = pc.GOLDEN_WEIGHTS
    plane_total = sum(reg.compute_plane_smoothness(g[ci]) for g in planes for ci in (0, 1, 3))
    time_total = sum(reg.compute_plane_smoothness(g[ci]) for g in planes for ci in (2, 4, 5))
    l1_total = sum(torch.abs(1 - g[ci]).mean() for g in planes for ci in (2, 4, 5))
    total = tvw * plane_total + tsw * time_total + l1w * l1_total
    total.backward()
    out = {"weights": np.array(pc.GOLDEN_WEIGHTS, np.float64), "total": np.float64(total.item()),
           "plane_smooth": np.float64(plane_total.item()), "time_smooth": np.float64(time_total.item()),
           "time_l1": np.float64(l1_total.item())}
    terms = []
    for s, scale in enumerate(planes):
        for ci, p in enumerate(scale):
            with torch.no_grad():
                terms.append((reg.compute_plane_smoothness(p).item(), torch.abs(1 - p).mean().item()))
            out[f"plane/{s}/{ci}"] = planes32[s][ci]
            out[f"grad/{s}/{ci}"] = p.grad.numpy()
    out["terms"] = np.array(terms, np.float64)
    dst = os.path.join(ROOT, "tests", "golden", "plane_reg.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
