"""Writes pca_golden.npz: what scikit-learn's PCA gives on the small planted-spectrum cases of
tests/pca_cases.py, so that tests/test_pca.py can hold the float64 restatement against the real
library without importing it.

Per case NAME (inputs at most 48 x 40 x 32): NAME/x the float32 image [H, W, C], NAME/sk the
normalised output of gaussian_scene.pca_compress's lines (sklearn PCA(3).fit_transform on the
float32 pixels, one min-max) [H, W, 3], NAME/e_sk its largest deviation from the restatement.
A wrong sign rule or ordering is off by 0.1 or more; the generator asserts e_sk <= 1e-4.

    python tests/golden/make_pca_golden.py        (needs scikit-learn; written with 1.7.2)
"""
import os
import sys

import numpy as np
from sklearn.decomposition import PCA

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pca_cases  # noqa: E402

# The low-contrast case is not recorded: scikit-learn's own float32 path (an uncentred float32 Gram,
# corrected by N m m^T) is off by 9e-4 there, past what can tell a right restatement from a wrong one.
NAMES = ["5x7x4", "16x24x6", "17x23x32", "40x48x32"]


def main():
    out = {}
    for name in NAMES:
        img, ref = pca_cases.case(name)
        H, W, C = img.shape
        assert H * W <= 48 * 40 and C <= 32
        y = PCA(n_components=3).fit_transform(img.reshape(-1, C)).reshape(H, W, 3)
        sk = (y - y.min()) / (y.max() - y.min())
        e_sk = float(np.abs(sk.astype(np.float64) - ref["out"].reshape(H, W, 3)).max())
        print(f"{name}: e_sk = {e_sk:.3e}")
        assert e_sk <= 1e-4, (name, e_sk)
        out[f"{name}/x"] = np.array(img)
        out[f"{name}/sk"] = sk
        out[f"{name}/e_sk"] = np.float64(e_sk)
    path = os.path.join(HERE, "pca_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
