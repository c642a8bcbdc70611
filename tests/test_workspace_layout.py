"""Every workspace size query of the library but the deformation field's two (tests/test_deform_layout.py),
without a GPU: the queries are host-only.  Each is the same walk of the unit's layout that carves the
workspace in the call (csrc/lsr_host.h Carver), so a changed number is a changed layout.  The shapes sit
around the 256-byte alignment and the kernels' tile edges; every expected number below is what a build of
commit f714373 (the last before the units shared one Carver) returned, written down, not recomputed."""
import ctypes

import pytest

from diff_gaussian_rasterization import _lib

# query: its argument tuples (plane_reg: the planes' (C, H, W); video: (the decoder's dims, n_rows))
CASES = {
    "lsr_geom_bytes": [(P,) for P in (0, 1, 63, 64, 255, 256, 257, 1024, 1025, 100000)],
    "lsr_binning_bytes": [(K,) for K in (0, 1, 64, 65, 257, 1000000)],
    "lsr_binning_bytes_tb": [(1000000, 100000, 640, 480), (0, 0, 1, 1), (1, 1, 16, 16), (65, 257, 17, 9),
                             (1000, 5000, 1352, 1014)],
    "lsr_img_bytes": [(17, 9), (16, 16), (1, 1), (64, 64), (65, 63), (1352, 1014)],
    "lsr_backward_bytes": [(1000, 5000, C, det) for C in (0, 3, 32) for det in (0, 1)]
                          + [(0, 0, 0, 0), (0, 0, 64, 1), (257, 65, 16, 1), (257, 65, 16, 0)],
    "lsr_train_workspace_bytes": [(P,) for P in (0, 1, 64, 65, 257, 1024, 1025, 100000)],
    "lsr_l1_workspace_bytes": [(V,) for V in (0, 1, 3, 8)],
    "lsr_image_loss_workspace_bytes": [(1, 3, 1, 1), (2, 3, 17, 33), (8, 3, 64, 65), (1, 1, 16, 64), (1, 1, 17, 65),
                                       (3, 3, 32, 128)],
    "lsr_seg_loss_workspace_bytes": [(1, 1, 1, 1), (2, 3, 17, 33), (8, 32, 64, 65), (1, 3, 32, 7), (1, 3, 33, 7),
                                     (8, 1, 1, 4097)],
    "lsr_segment_workspace_bytes": [(0, 1, 1), (1, 1, 1), (3, 33, 65), (70000, 16, 16), (1, 16, 64), (1, 17, 65),
                                    (2, 32, 64), (2, 33, 128), (64, 512, 512)],
    "lsr_pca_workspace_bytes": [(4, 1), (32, 2049), (16, 100000), (4, 0), (32, 2048), (8, 4096), (8, 4097)],
    "lsr_knn_workspace_bytes": [(P,) for P in (0, 1, 64, 257, 1024, 1025, 100000)],
    "lsr_plane_reg_workspace_bytes": [((16, 5, 7), (16, 150, 64)), (), ((1, 3, 1),), ((16, 64, 64),), ((16, 64, 64), (1, 3, 1)),
                                      ((32, 150, 64),) * 3],
    "lsr_video_workspace_bytes": [((3, 16), 0), ((3, 16), 1), ((3, 64, 512), 127), ((3, 64, 512), 128),
                                  ((3, 64, 512), 129), ((6, 128, 256, 512, 1024), 1000), ((3, 16, 32, 16), 5)],
}

# query: the values at its CASES, in their order; from a build of commit f714373
EXPECTED = {
    "lsr_geom_bytes": (20992, 20992, 27136, 27136, 57088, 57088, 61184, 177664, 181760, 16111872),
    "lsr_binning_bytes": (17920, 17920, 17920, 18944, 22016, 20014592),
    "lsr_binning_bytes_tb": (28048384, 18432, 18432, 19968, 63232),
    "lsr_img_bytes": (2304, 2816, 1280, 33536, 33536, 11054592),
    "lsr_backward_bytes": (64000, 245248, 64000, 325120, 64000, 885248, 256, 768, 7680, 16640),
    "lsr_train_workspace_bytes": (1280, 1280, 1280, 2304, 5376, 16640, 17664, 1601280),
    "lsr_l1_workspace_bytes": (1024, 1024, 3072, 8192),
    "lsr_image_loss_workspace_bytes": (512, 40960, 1202688, 12544, 13568, 443392),
    "lsr_seg_loss_workspace_bytes": (512, 1792, 200704, 1536, 1792, 512),
    "lsr_segment_workspace_bytes": (0, 1536, 1536, 1960448, 1536, 1536, 1536, 1536, 229888),
    "lsr_pca_workspace_bytes": (3072, 6144, 150528, 3072, 3072, 6144, 9216),
    "lsr_knn_workspace_bytes": (30720, 30720, 31488, 38912, 62208, 63488, 3625472),
    "lsr_plane_reg_workspace_bytes": (2416, 16, 16, 1024, 1040, 14400),
    "lsr_video_workspace_bytes": (16, 80, 67056, 67584, 68112, 3616000, 1312),
}


def query(name, args):
    lib = _lib.load()
    if name == "lsr_plane_reg_workspace_bytes":
        planes = (_lib.PlaneDesc * max(len(args), 1))()
        for d, (C, H, W) in zip(planes, args):
            d.C, d.H, d.W, d.w_smooth, d.w_l1 = C, H, W, 1.0, 1.0   # the query reads no pointer
        return int(lib.lsr_plane_reg_workspace_bytes(len(args), planes))
    if name == "lsr_video_workspace_bytes":
        dims, n_rows = args
        dec = _lib.Decoder()
        dec.n_layers = len(dims) - 1
        dec.dims = (ctypes.c_int32 * 9)(*dims)
        return int(lib.lsr_video_workspace_bytes(ctypes.byref(dec), n_rows))
    return int(getattr(lib, name)(*args))


def test_every_query_has_its_numbers():
    assert set(EXPECTED) == set(CASES)
    assert all(len(EXPECTED[q]) == len(CASES[q]) and min(EXPECTED[q]) >= 0 for q in CASES)


def test_every_size_query_of_the_library_is_listed():
    """(the deformation field's two are pinned by tests/test_deform_layout.py)"""
    queries = {n for n in _lib.SIGNATURES if n.endswith(("_bytes", "_bytes_tb"))}
    assert queries == set(CASES) | {"lsr_deform_workspace_bytes", "lsr_deform_backward_scratch_bytes"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_bytes_are_the_recorded_ones(name):
    assert tuple(query(name, a) for a in CASES[name]) == EXPECTED[name]
