"""CPU checks of the C ABI: liblsr.so builds for gfx950, loads, and exports exactly what
include/*.h declare; the workspace size queries behave (no GPU compute is called here)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", h) for h in sorted(os.listdir(os.path.join(ROOT, "include"))) if h.endswith(".h")]


def declared():
    txt = "".join(open(h).read() for h in HEADERS)
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|const char \*)\s*(lsr_\w+)\s*\(", txt, re.M)))


def test_header_declares_the_boundary():
    names = declared()
    for n in ("lsr_forward_preprocess", "lsr_forward_render", "lsr_backward", "lsr_mark_visible",
              "lsr_geom_bytes", "lsr_binning_bytes", "lsr_img_bytes", "lsr_backward_bytes", "lsr_last_error",
              "lsr_version"):
        assert n in names


def test_library_exports_every_declared_symbol():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    for n in declared():
        assert hasattr(lib, n), n
    assert set(declared()) == set(_lib.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (lsr_\w+)", out))
    assert exported == set(declared())


def test_library_has_no_undefined_internal_symbols():
    """Every kernel launch stub the library references is defined in it (a template kernel whose
    host-side instantiation is dropped leaves an undefined __device_stub__ that only fails at
    load time on the GPU box)."""
    from diff_gaussian_rasterization import _lib
    out = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert not [l for l in out.splitlines() if "lsr" in l], out


def test_library_is_built_for_gfx950():
    from diff_gaussian_rasterization import _lib
    out = subprocess.run(["strings", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_size_queries():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.lsr_version() == _lib.API_VERSION == 4
    g1, g2 = lib.lsr_geom_bytes(1000), lib.lsr_geom_bytes(2_000_000)
    assert 0 < g1 < g2 and g2 >= 2_000_000 * 60
    assert lib.lsr_binning_bytes(8_600_000) >= 8_600_000 * 16
    assert lib.lsr_img_bytes(1352, 1014) >= 1352 * 1014 * 8
    assert lib.lsr_backward_bytes(2_000_000, 8_600_000, 32, 0) >= 2_000_000 * 48
    assert lib.lsr_backward_bytes(2_000_000, 8_600_000, 32, 1) >= 8_600_000 * 44 * 4
    # the tile-bucket binning: the sort path's layout (the compositors read its point list), then the
    # per-block tile count table and the long buckets' 8-byte merge workspace
    K, P, W, H = 8_600_000, 2_000_000, 1352, 1014
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    tb = lib.lsr_binning_bytes_tb(K, P, W, H)
    assert tb >= lib.lsr_binning_bytes(K) + 8 * K + 4 * tiles * (P // 16384)
    assert lib.lsr_binning_bytes_tb(K, 2 * P, W, H) > tb                  # more Gaussians: more table rows
    assert lib.lsr_binning_bytes_tb(K, P, 0, H) == -1                     # invalid image size


def test_train_glue_argument_checks():
    """The training-step glue (include/lsr_train.h: activations, view repeat / sum, the multi-view L1)
    refuses bad arguments with a message and accepts empty work, before anything touches a device."""
    import ctypes
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    err = lambda: lib.lsr_last_error().decode()
    assert lib.lsr_l1_workspace_bytes(1) == 256 * 4 and lib.lsr_l1_workspace_bytes(8) == 8 * 256 * 4
    assert lib.lsr_l1_workspace_bytes(0) == 256 * 4
    p = ctypes.c_void_p(64)                                    # never dereferenced: every call below fails early
    imgs = (ctypes.c_void_p * 9)(*([64] * 9))
    for V, n, stride in ((0, 4, 4), (9, 4, 4), (2, -1, 4), (2, 8, 4)):
        assert lib.lsr_l1_loss_views(V, n, imgs, p, stride, p, p, None) != 0
        assert "1 <= V <= 8" in err()
    assert lib.lsr_l1_loss_views(2, 4, imgs, p, 4, None, p, None) != 0 and "workspace required" in err()
    assert lib.lsr_l1_loss_views_backward(2, 4, imgs, p, 4, None, imgs, None) != 0 and "d_loss" in err()
    holes = (ctypes.c_void_p * 2)(64, None)
    assert lib.lsr_l1_loss_views(2, 4, holes, p, 4, p, p, None) != 0 and "null image" in err()
    assert lib.lsr_l1_loss_views_backward(2, 4, imgs, p, 4, p, holes, None) != 0 and "null gradient" in err()
    assert lib.lsr_activate(-1, None, None, None, None, None, None, None) != 0 and "P >= 0" in err()
    assert lib.lsr_activate(4, p, None, None, None, None, None, None) != 0 and "needs its output" in err()
    assert lib.lsr_activate(4, None, ctypes.c_void_p(72), None, None, ctypes.c_void_p(64), None, None) != 0
    assert "16-byte aligned" in err()
    assert lib.lsr_activate(0, p, p, p, p, p, p, None) == 0    # no rows: no launch
    rt = (_lib.RowTensor * 1)()
    assert lib.lsr_repeat_rows(1, rt, 4, 0, None) != 0 and "n_blocks >= 1" in err()
    assert lib.lsr_sum_row_blocks(1, rt, 4, 2, None) != 0 and "rows of whole floats" in err()
    assert lib.lsr_repeat_rows(0, None, 4, 2, None) == 0 and lib.lsr_sum_row_blocks(1, rt, 0, 2, None) == 0


def test_rasterizer_argument_checks():
    """The rasterizer's entry points (include/lsr.h) refuse bad batches with LSR_EINVAL and their
    message, every view validated before anything touches a device, and accept P = 0 as no work."""
    import ctypes
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    err = lambda: lib.lsr_last_error().decode()
    FAKE = 64                                                  # never dereferenced: every call returns early

    def settings(W=64, H=48, scale=1.0, feature=1):
        s = _lib.Settings()
        s.image_width, s.image_height, s.tanfovx, s.tanfovy = W, H, 0.5, 0.5
        s.bg = s.viewmatrix = s.projmatrix = s.campos = FAKE
        s.scale_modifier, s.sh_degree, s.include_feature = scale, 0, feature
        return s

    def views(*ss):
        return (ctypes.POINTER(_lib.Settings) * len(ss))(*[ctypes.pointer(s) for s in ss])

    def structs(cls, n, **fields):
        objs = [cls(**fields) for _ in range(n)]
        return (ctypes.POINTER(cls) * n)(*[ctypes.pointer(o) for o in objs]), objs

    def refused(rc, text):
        assert rc == 1 and text in err(), (rc, err())          # LSR_EINVAL

    fin = _lib.FwdIn()
    fin.P, fin.M, fin.C = 1000, 0, 0
    fin.means3D = fin.opacities = fin.colors_precomp = fin.scales = fin.rotations = FAKE
    fi = ctypes.byref(fin)
    same = views(settings(), settings())
    sizes = views(settings(), settings(W=80))
    scales = views(settings(), settings(scale=2.0))
    features = views(settings(), settings(feature=0))
    vp = (ctypes.c_void_p * 2)(FAKE, FAKE)
    K = (ctypes.c_int64 * 2)(10, 10)
    hc = ctypes.c_void_p(FAKE)
    outs, _o = structs(_lib.FwdOut, 2, out_color=FAKE, out_depth=FAKE, radii=FAKE)
    no_radii, _n = structs(_lib.FwdOut, 2, out_color=FAKE, out_depth=FAKE)
    gins, _g = structs(_lib.BwdIn, 2, dL_dout_color=FAKE)
    det, _d = structs(_lib.BwdIn, 2, dL_dout_color=FAKE, deterministic=1)
    gout = ctypes.byref(_lib.BwdOut())

    # every batched entry point as f(n_views, settings array): the other arguments valid
    batched = {
        "lsr_forward_preprocess_views_async":
            lambda n, s: lib.lsr_forward_preprocess_views_async(n, s, fi, outs, vp, hc, None),
        "lsr_forward_preprocess_views_split_async":
            lambda n, s: lib.lsr_forward_preprocess_views_split_async(n, n, s, fi, outs, vp, hc, None),
        "lsr_forward_preprocess_views_rows_async":
            lambda n, s: lib.lsr_forward_preprocess_views_rows_async(n, 0, 1000, s, fi, outs, vp, None),
        "lsr_forward_preprocess_views_tb_async":
            lambda n, s: lib.lsr_forward_preprocess_views_tb_async(n, 0, 1000, s, fi, outs, vp, None),
        "lsr_forward_depth_order_views_async":
            lambda n, s: lib.lsr_forward_depth_order_views_async(n, s, fi, vp, hc, None),
        "lsr_forward_instance_scan_views_async":
            lambda n, s: lib.lsr_forward_instance_scan_views_async(n, s, fi, vp, hc, None),
        "lsr_forward_binning_views": lambda n, s: lib.lsr_forward_binning_views(n, s, fi, vp, vp, vp, K, None),
        "lsr_forward_binning_views_tb": lambda n, s: lib.lsr_forward_binning_views_tb(n, s, fi, vp, vp, vp, K, None),
        "lsr_forward_composite_views":
            lambda n, s: lib.lsr_forward_composite_views(n, s, fi, outs, vp, vp, vp, K, None),
        "lsr_backward_composite_views":
            lambda n, s: lib.lsr_backward_composite_views(n, s, fi, gins, None, vp, vp, vp, K, None),
        "lsr_backward_preprocess_views": lambda n, s: lib.lsr_backward_preprocess_views(n, s, fi, gout, vp, 0, None),
        "lsr_backward_preprocess_views_rows":
            lambda n, s: lib.lsr_backward_preprocess_views_rows(n, s, fi, gout, vp, 0, 0, 1000, None),
        "lsr_backward_views": lambda n, s: lib.lsr_backward_views(n, s, fi, gins, gout, vp, vp, vp, K, 0, None),
    }
    own_words = ("lsr_backward_preprocess_views", "lsr_backward_preprocess_views_rows", "lsr_backward_views")
    for name, f in batched.items():
        refused(f(0, same), "n_views must be >= 1" if name in own_words else "n_views >= 1 and the per-view arrays")
        refused(f(2, None), "null argument" if name in own_words else "the per-view arrays are required")
    for name in ("lsr_forward_preprocess_views_async", "lsr_forward_preprocess_views_split_async",
                 "lsr_forward_preprocess_views_rows_async", "lsr_forward_preprocess_views_tb_async",
                 "lsr_forward_depth_order_views_async", "lsr_forward_instance_scan_views_async"):
        refused(batched[name](2, sizes), "share the image size, sh_degree and scale_modifier")
        refused(batched[name](2, scales), "share the image size, sh_degree and scale_modifier")
    for name in ("lsr_forward_binning_views", "lsr_forward_binning_views_tb"):
        refused(batched[name](2, sizes), "batched views must share the image size")
    for name in ("lsr_forward_composite_views", "lsr_backward_composite_views", "lsr_backward_views"):
        refused(batched[name](2, sizes), "share the image size and include_feature")
        refused(batched[name](2, features), "share the image size and include_feature")
    for name in ("lsr_backward_preprocess_views", "lsr_backward_preprocess_views_rows", "lsr_backward_views"):
        refused(batched[name](2, scales), "all views must share scale_modifier")
    null_view = (ctypes.c_void_p * 2)(FAKE, None)
    refused(lib.lsr_forward_depth_order_views_async(2, same, fi, null_view, hc, None), "geom workspaces are required")
    refused(lib.lsr_forward_binning_views(2, same, fi, vp, vp, null_view, K, None), "workspaces are required")
    refused(lib.lsr_forward_binning_views_tb(2, same, fi, vp, null_view, vp, K, None), "workspaces are required")
    refused(lib.lsr_backward_preprocess_views(2, same, fi, gout, null_view, 0, None),
            "geom workspace is required for every")

    # rows, ordered views, outputs and counts
    refused(lib.lsr_forward_preprocess_views_rows_async(2, 128, 1000, same, fi, outs, vp, None),
            "row0 a multiple of 256")
    refused(lib.lsr_forward_preprocess_views_tb_async(2, 128, 1000, same, fi, outs, vp, None), "row0 a multiple of 256")
    refused(lib.lsr_forward_preprocess_views_rows_async(2, 0, 1001, same, fi, outs, vp, None), "row0 <= row1 <= P")
    refused(lib.lsr_backward_preprocess_views_rows(2, same, fi, gout, vp, 0, 128, 100, None),
            "row_begin must be a multiple")
    refused(lib.lsr_backward_preprocess_views_rows(2, same, fi, gout, vp, 0, 768, 256, None), "must lie inside [0, P)")
    refused(lib.lsr_forward_preprocess_views_split_async(2, 3, same, fi, outs, vp, hc, None),
            "0 <= n_ordered <= n_views")
    refused(lib.lsr_forward_preprocess_views_split_async(2, 1, same, fi, outs, vp, None, None),
            "0 <= n_ordered <= n_views")
    refused(lib.lsr_forward_preprocess_views_split_async(2, 2, same, fi, no_radii, vp, hc, None),
            "radii output is required")
    refused(lib.lsr_forward_preprocess_views_rows_async(2, 0, 1000, same, fi, no_radii, vp, None),
            "radii output is required")
    refused(lib.lsr_forward_preprocess_async(same[0], fi, no_radii[0], hc, hc, None), "radii output is required")
    refused(lib.lsr_forward_preprocess_async(same[0], fi, outs[0], hc, None, None), "geom workspace and host_count are")
    refused(lib.lsr_forward_preprocess_async(same[0], fi, outs[0], None, hc, None), "geom workspace and host_count are")
    refused(lib.lsr_forward_preprocess(same[0], fi, outs[0], hc, None, None), "geom workspace and num_rendered are")
    refused(lib.lsr_forward_preprocess_views_async(2, same, fi, outs, vp, None, None), "host_counts is required")
    refused(lib.lsr_forward_depth_order_views_async(2, same, fi, vp, None, None), "host_counts is required")
    refused(lib.lsr_forward_instance_scan_views_async(2, same, fi, vp, None, None), "host_counts is required")
    refused(lib.lsr_forward_composite_views(2, same, fi, structs(_lib.FwdOut, 2, radii=FAKE)[0], vp, vp, vp, K, None),
            "color and depth outputs are required")
    refused(lib.lsr_backward_composite_views(2, same, fi, structs(_lib.BwdIn, 2)[0], None, vp, vp, vp, K, None),
            "dL_dout_color is required")
    refused(lib.lsr_backward_composite_views(2, same, fi, det, None, vp, vp, vp, K, None),
            "the split backward reduces with float atomics")
    refused(lib.lsr_backward_views(2, same, fi, det, gout, vp, vp, vp, K, 0, None),
            "lsr_backward_views reduces with float atomics")

    # P = 0: nothing to do, the counts are zeroed on the host
    fin.P = 0
    counts = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    cp = ctypes.c_void_p(ctypes.addressof(counts))

    def zeroed(rc, n=4):
        assert rc == 0 and list(counts) == [0] * n + [7] * (4 - n), (rc, err(), list(counts))
        counts[:] = [7, 7, 7, 7]

    zeroed(lib.lsr_forward_preprocess_async(same[0], fi, outs[0], hc, cp, None), 2)
    zeroed(lib.lsr_forward_preprocess_views_async(2, same, fi, outs, vp, cp, None))
    zeroed(lib.lsr_forward_preprocess_views_split_async(2, 1, same, fi, outs, vp, cp, None), 2)
    zeroed(lib.lsr_forward_depth_order_views_async(2, same, fi, vp, cp, None))
    zeroed(lib.lsr_forward_instance_scan_views_async(2, same, fi, vp, cp, None))
    assert lib.lsr_forward_preprocess_views_rows_async(2, 0, 0, same, fi, outs, vp, None) == 0
    assert lib.lsr_forward_preprocess_views_tb_async(2, 0, 0, same, fi, outs, vp, None) == 0
    assert lib.lsr_backward(same[0], fi, gins[0], gout, hc, hc, hc, hc, 0, 0, None) == 0
    assert lib.lsr_backward_composite(same[0], fi, gins[0], None, hc, hc, hc, 0, None) == 0
    assert lib.lsr_backward_composite_views(2, same, fi, gins, None, vp, vp, vp, K, None) == 0
    assert lib.lsr_backward_preprocess_views(2, same, fi, gout, vp, 0, None) == 0
    assert lib.lsr_backward_preprocess_views_rows(2, same, fi, gout, vp, 0, 0, 0, None) == 0
    assert lib.lsr_backward_views(2, same, fi, gins, gout, vp, vp, vp, K, 0, None) == 0


def test_settings_validation_messages():
    """Upstream's exactly-one-of errors are raised before anything touches a device."""
    import torch
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.ones(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                           torch.zeros(3), False, False)
    assert rs.include_feature is True       # dataset_readers.py:502-515 builds it without the field
    r = dgr.GaussianRasterizer(rs)
    m = torch.zeros(4, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=torch.ones(4, 1), scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        r(means3D=m, means2D=m, opacities=torch.ones(4, 1), shs=torch.zeros(4, 16, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        r(means3D=m, means2D=m, opacities=torch.ones(4, 1), shs=torch.zeros(4, 16, 3), scales=m,
          rotations=torch.zeros(4, 4))


def test_callers_of_another_header_version_are_refused():
    """lsr_require_api: until a caller has declared the lsr.h version it was built against, every
    entry point that reads the structs refuses (no misread trailing fields); a mismatched
    declaration is refused too.  Fresh process: the handshake is per process."""
    import sys
    from diff_gaussian_rasterization import _lib
    code = f"""
import ctypes
L = ctypes.CDLL({_lib.LIB_PATH!r})
L.lsr_last_error.restype = ctypes.c_char_p
k = ctypes.c_int64(0)
rc = L.lsr_forward_preprocess(None, None, None, None, ctypes.byref(k), None)
assert rc == 1 and b"lsr_require_api" in L.lsr_last_error(), (rc, L.lsr_last_error())
assert L.lsr_require_api(3) == 1 and b"mismatch" in L.lsr_last_error()
rc = L.lsr_forward_preprocess(None, None, None, None, ctypes.byref(k), None)
assert rc == 1 and b"lsr_require_api" in L.lsr_last_error()
assert L.lsr_require_api(4) == 0
rc = L.lsr_forward_preprocess(None, None, None, None, ctypes.byref(k), None)
assert rc == 1 and b"null settings" in L.lsr_last_error(), L.lsr_last_error()
# lsr_deform.h has its own handshake (its structs gained a trailing field in version 3)
L.lsr_deform_workspace_bytes.restype = ctypes.c_int64
assert L.lsr_deform_workspace_bytes(None) == -1 and b"lsr_deform_require_api" in L.lsr_last_error()
assert L.lsr_deform_require_api(2) == 1 and b"mismatch" in L.lsr_last_error()
assert L.lsr_deform_workspace_bytes(None) == -1 and b"lsr_deform_require_api" in L.lsr_last_error()
assert L.lsr_deform_require_api(3) == 0
assert L.lsr_deform_workspace_bytes(None) == -1 and b"null deformation net" in L.lsr_last_error()
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


STRUCTS = {"Settings": "lsr_settings", "FwdIn": "lsr_fwd_in", "FwdOut": "lsr_fwd_out", "BwdIn": "lsr_bwd_in",
           "BwdOut": "lsr_bwd_out", "DeformNet": "lsr_deform_net", "DeformGrads": "lsr_deform_grads",
           "AdamGroup": "lsr_adam_group", "RowTensor": "lsr_row_tensor"}


def test_ctypes_structs_match_the_headers(tmp_path):
    """Every ctypes mirror of an include/*.h struct has the C compiler's field offsets and size
    (a duplicated or misplaced field in a mirror hands the library NULL or shifted pointers)."""
    from diff_gaussian_rasterization import _lib
    lines = ["#include <stddef.h>", "#include <stdio.h>"] + [f'#include "{h}"' for h in HEADERS] + ["int main(void) {"]
    want = {}
    for py, c in STRUCTS.items():
        cls = getattr(_lib, py)
        names = [f[0] for f in cls._fields_]
        assert len(names) == len(set(names)), f"{py}: duplicate fields"
        lines.append(f'printf("{py} size %zu\\n", sizeof({c}));')
        want[(py, "size")] = ctypes_sizeof(cls)
        for n in names:
            lines.append(f'printf("{py} {n} %zu\\n", offsetof({c}, {n}));')
            want[(py, n)] = getattr(cls, n).offset
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        py, n, v = line.split()
        got[(py, n)] = int(v)
    assert got == want


def ctypes_sizeof(cls):
    import ctypes
    return ctypes.sizeof(cls)
