"""CPU checks of the PCA colouring (include/lsr_pca.h, language_query.pca_image / LanguagePCA): the
float64 restatement the GPU tests compare against agrees with real scikit-learn (recorded in
golden/pca_golden.npz by golden/make_pca_golden.py, so nothing here imports sklearn), every case meets
the conditions under which its answer is well defined, and the library and the Python surface refuse
what they cannot take before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pca_cases


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pca_golden.npz"))


def test_every_case_is_well_defined():
    for name in pca_cases.CASES:
        img, ref = pca_cases.case(name)                # the builder asserts the gap and the sign margin
        assert img.dtype == np.float32 and ref["out"].min() == 0.0 and ref["out"].max() == 1.0
        assert np.allclose(np.linalg.norm(ref["components"], axis=1), 1.0, atol=1e-12)
    frames, ref = pca_cases.sequence_case()
    assert len(frames) == 3 and ref["y"].shape == (3 * 17 * 23, 3)


def _header_constants():
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lsr_pca.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (LSR_PCA_\w+) (\d+)", txt, re.M)}


def test_kernel_constants_agree():
    """include/lsr_pca.h (which csrc/pca.hip takes its constants from), the ctypes binding and the case
    builder name the same numbers: the large cases mean what their comments say."""
    from diff_gaussian_rasterization import _lib
    h = _header_constants()
    assert h == {"LSR_PCA_MIN_CHANNELS": _lib.PCA_MIN_CHANNELS, "LSR_PCA_MAX_CHANNELS": _lib.PCA_MAX_CHANNELS,
                 "LSR_PCA_BLOCK_PIXELS": _lib.PCA_BLOCK_PIXELS, "LSR_PCA_TILE_PIXELS": _lib.PCA_TILE_PIXELS,
                 "LSR_PCA_FINISH_WAVES": _lib.PCA_FINISH_WAVES, "LSR_PCA_RANGE_THREADS": _lib.PCA_RANGE_THREADS}
    assert (pca_cases.BLOCK_PIXELS, pca_cases.TILE_PIXELS, pca_cases.FINISH_WAVES, pca_cases.RANGE_THREADS) == \
        (_lib.PCA_BLOCK_PIXELS, _lib.PCA_TILE_PIXELS, _lib.PCA_FINISH_WAVES, _lib.PCA_RANGE_THREADS)
    src = open(os.path.join(os.path.dirname(_lib._PKG), "4dlangsplat_amd", "csrc", "pca.hip")).read()
    for name in ("LSR_PCA_BLOCK_PIXELS", "LSR_PCA_TILE_PIXELS", "LSR_PCA_FINISH_WAVES", "LSR_PCA_RANGE_THREADS"):
        assert name in src, f"pca.hip no longer takes {name} from the header"


def test_the_blocks_case_spans_three_blocks_with_a_ragged_tail():
    from diff_gaussian_rasterization import _lib
    blocks = lambda name: divmod(pca_cases.CASES[name][0] * pca_cases.CASES[name][1], _lib.PCA_BLOCK_PIXELS)
    full, rest = blocks("blocks")
    assert full >= 2 and rest % _lib.PCA_TILE_PIXELS and rest > _lib.PCA_TILE_PIXELS


def test_the_large_cases_reach_every_level_of_the_cross_block_reductions():
    """k_pca_finish: every wave adds at least two partials, then the 16-way fold; k_pca_range: a thread
    folds more than one pair; both with a ragged last block, and on the 16-byte load path."""
    from diff_gaussian_rasterization import _lib
    blocks = lambda name: divmod(pca_cases.CASES[name][0] * pca_cases.CASES[name][1], _lib.PCA_BLOCK_PIXELS)
    full, rest = blocks("fan-in")
    assert full + 1 >= 2 * _lib.PCA_FINISH_WAVES + 1 and full >= 2 * _lib.PCA_FINISH_WAVES
    assert rest and rest % _lib.PCA_TILE_PIXELS
    full, rest = blocks("many-blocks")
    assert full + 1 > _lib.PCA_RANGE_THREADS and full // _lib.PCA_FINISH_WAVES >= 2 * 8
    assert rest and rest % _lib.PCA_TILE_PIXELS
    for name in ("fan-in", "many-blocks"):
        H, W, C = pca_cases.CASES[name][:3]
        assert H * W % 4 == 0 and C % 4 == 0


def test_restatement_matches_recorded_sklearn(golden):
    names = sorted({k.split("/")[0] for k in golden.files})
    assert names == sorted(["5x7x4", "16x24x6", "17x23x32", "40x48x32"])
    for name in names:
        x, sk, e_sk = golden[f"{name}/x"], golden[f"{name}/sk"], float(golden[f"{name}/e_sk"])
        img, ref = pca_cases.case(name)
        assert np.array_equal(x, img), f"{name}: the golden file was written for other inputs"
        assert e_sk <= 1e-4
        err = float(np.abs(sk.astype(np.float64) - ref["out"].reshape(sk.shape)).max())
        print(f"{name}: |restatement - sklearn| = {err:.3e}, recorded e_sk = {e_sk:.3e}")
        assert err <= 2 * e_sk                         # 2: BLAS builds that sum in another order


def test_library_refuses_bad_arguments():
    """LSR_EINVAL and a message, decided before the device is touched (this machine has none)."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    err = lambda: lib.lsr_last_error().decode()
    p = ctypes.c_void_p(64)                                    # never dereferenced: every call below returns early

    def refused(rc, text):
        assert rc == 1 and text in err(), (rc, err())          # LSR_EINVAL

    assert lib.lsr_pca_workspace_bytes(32, 0) > 0
    assert lib.lsr_pca_workspace_bytes(32, 1352 * 1014) >= (1352 * 1014 // _lib.PCA_BLOCK_PIXELS) * 3 * 256 * 4
    for C, n in ((3, 10), (33, 10), (8, -1)):
        assert lib.lsr_pca_workspace_bytes(C, n) == -1 and "C in [4, 32] and n_pix >= 0" in err()
    for C in (3, 33, 0, -4):
        refused(lib.lsr_pca_sums(C, 10, p, 1, 10, 1, p, p, None), "C must be in [4, 32]")
        refused(lib.lsr_pca_gram(C, 10, p, 1, 10, p, 10, 1, p, p, None), "C must be in [4, 32]")
        refused(lib.lsr_pca_basis(C, 10, p, p, p, p, p, None), "C must be in [4, 32]")
        refused(lib.lsr_pca_project(C, 10, p, 1, 10, p, p, 1, p, p, p, None), "C must be in [4, 32]")
    refused(lib.lsr_pca_sums(8, -1, p, 1, 10, 1, p, p, None), "n_pix must be >= 0")
    refused(lib.lsr_pca_gram(8, -1, p, 1, 10, p, 10, 1, p, p, None), "n_pix must be >= 0")
    refused(lib.lsr_pca_project(8, -1, p, 1, 10, p, p, 1, p, p, p, None), "n_pix must be >= 0")
    refused(lib.lsr_pca_colorize_f32(-1, p, p, p, None), "n_pix must be >= 0")
    refused(lib.lsr_pca_colorize_u8(-1, p, p, p, None), "n_pix must be >= 0")
    # NULL pointers, one at a time
    refused(lib.lsr_pca_sums(8, 10, None, 1, 10, 1, p, p, None), "frame and workspace are required")
    refused(lib.lsr_pca_sums(8, 10, p, 1, 10, 1, p, None, None), "frame and workspace are required")
    refused(lib.lsr_pca_sums(8, 10, p, 1, 10, 1, None, p, None), "sums is required")
    refused(lib.lsr_pca_gram(8, 10, None, 1, 10, p, 10, 1, p, p, None), "frame and workspace are required")
    refused(lib.lsr_pca_gram(8, 10, p, 1, 10, None, 10, 1, p, p, None), "sums and gram are required")
    refused(lib.lsr_pca_gram(8, 10, p, 1, 10, p, 10, 1, None, p, None), "sums and gram are required")
    refused(lib.lsr_pca_gram(8, 10, p, 1, 10, p, 9, 1, p, p, None), "n_total must be the pixel count of the sums")
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        refused(lib.lsr_pca_basis(8, 10, *args, None), "sums, gram, mean, components and eigenvalues are required")
    refused(lib.lsr_pca_basis(8, 1, p, p, p, p, p, None), "n_total >= 2")
    refused(lib.lsr_pca_basis(8, 0, p, p, p, p, p, None), "n_total >= 2")
    refused(lib.lsr_pca_project(8, 10, None, 1, 10, p, p, 1, p, p, p, None), "frame and workspace are required")
    refused(lib.lsr_pca_project(8, 10, p, 1, 10, None, p, 1, p, p, p, None), "mean and components are required")
    refused(lib.lsr_pca_project(8, 10, p, 1, 10, p, None, 1, p, p, p, None), "mean and components are required")
    refused(lib.lsr_pca_project(8, 10, p, 1, 10, p, p, 1, None, None, p, None), "y or range is required")
    refused(lib.lsr_pca_project(8, 10, p, 1, 10, p, p, 1, p, p, None, None), "frame and workspace are required")
    refused(lib.lsr_pca_project(8, 10, p, 1, 10, p, p, 1, None, p, None, None), "frame and workspace are required")
    # strides that cannot describe memory
    refused(lib.lsr_pca_sums(8, 10, p, -1, 10, 1, p, p, None), "pix_stride and chan_stride must be >= 0")
    refused(lib.lsr_pca_gram(8, 10, p, 1, -10, p, 10, 1, p, p, None), "pix_stride and chan_stride must be >= 0")
    refused(lib.lsr_pca_project(8, 10, p, -8, 1, p, p, 1, p, p, p, None), "pix_stride and chan_stride must be >= 0")
    refused(lib.lsr_pca_sums(8, 10, p, 1, 10, 1, p, ctypes.c_void_p(68), None), "8-byte aligned")
    for fn in (lib.lsr_pca_colorize_f32, lib.lsr_pca_colorize_u8):
        for hole in range(3):
            args = [p] * 3
            args[hole] = None
            refused(fn(10, *args, None), "y, range and out are required")
    # no pixels: nothing is launched
    assert lib.lsr_pca_sums(8, 0, p, 1, 0, 1, p, p, None) == 0
    assert lib.lsr_pca_gram(8, 0, p, 1, 0, p, 10, 0, p, p, None) == 0
    assert lib.lsr_pca_project(8, 0, p, 1, 0, p, p, 0, None, p, p, None) == 0
    assert lib.lsr_pca_project(8, 0, p, 1, 0, p, p, 0, p, None, None, None) == 0     # y alone needs no workspace
    assert lib.lsr_pca_colorize_f32(0, p, p, p, None) == 0 and lib.lsr_pca_colorize_u8(0, p, p, p, None) == 0


def test_python_surface_refuses_what_the_library_cannot_take():
    """ValueError with the reason, never a bad pointer to a kernel."""
    import language_query as lq
    good = torch.zeros(8, 5, 7)
    for call in (lq.pca_image, lambda f, **kw: lq.LanguagePCA().fit([f], **kw)):
        with pytest.raises(ValueError, match="CPU tensor"):
            call(good)
        with pytest.raises(ValueError, match="CPU tensor"):
            call(torch.zeros(5, 7, 8).permute(2, 0, 1))                                  # a view two strides describe
        with pytest.raises(ValueError, match='layout must be "hwc" or "chw"'):
            call(good, layout="nchw")
        with pytest.raises(ValueError, match="3-dimensional"):
            call(torch.zeros(2, 8, 5, 7))
        with pytest.raises(ValueError, match="3-dimensional"):
            call(np.zeros((8, 5, 7), np.float32))
        with pytest.raises(ValueError, match="float32 frames, got torch.float64"):
            call(torch.zeros(8, 5, 7, dtype=torch.float64))
        for C in (1, 3, 33):
            with pytest.raises(ValueError, match=f"4 ... 32 channels, the frame has C = {C}"):
                call(torch.zeros(C, 5, 7))
            with pytest.raises(ValueError, match=f"4 ... 32 channels, the frame has C = {C}"):
                call(torch.zeros(5, 7, C), layout="hwc")
        with pytest.raises(ValueError, match="two strides cannot describe"):
            call(torch.zeros(8, 5, 9)[:, :, :7])                                         # rows of 9, 7 used
        with pytest.raises(ValueError, match="two strides cannot describe"):
            call(torch.zeros(5, 9, 8)[:, :7], layout="hwc")
    with pytest.raises(ValueError, match='out must be "float" or "uint8"'):
        lq.pca_image(good, out="png")
    with pytest.raises(ValueError, match="at least one frame"):
        lq.LanguagePCA().fit([])
    with pytest.raises(ValueError, match="before fit"):
        lq.LanguagePCA().transform(good)
    import gaussian_scene as gs
    with pytest.raises(ValueError, match='pca must be "sklearn", "native" or "sequence"'):
        gs.render_set("unused", "test", 0, [], None, None, pca="torch")
