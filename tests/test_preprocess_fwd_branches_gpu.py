"""Every instantiation of the forward preprocess (preprocess.hip, k_preprocess<MS, MULTI>) per
Gaussian against the float oracle: what the kernel writes into a view's geom workspace, not what
the compositor later makes of it.

Phase 1 alone (lsr_forward_preprocess; lsr_forward_preprocess_views_async for several views;
lsr_forward_preprocess_views_rows_async + lsr_forward_depth_order_views_async for row chunks) runs
into workspaces the test owns and has filled with the byte 0xA5, radii included, so a row the kernel
forgets to reset shows whatever the allocator would have returned.  The workspace is decoded
(lsr_testutil.decode_geom) and held to lsr_testutil.preprocess_check: radii; xy, conic and opacity,
colour and depth bit for bit; the clamped bits; culled rows reset; the binning rectangle inside
upstream's, tiles == rect_count(rect) <= upstream's, sum(tiles) == num_rendered; faint Gaussians
(opacity <= 0.003) with a radius and no tiles; accumulator rows zeroed under a rectangle and
untouched elsewhere.  One-view cases are also finished with the public forward_native, whose
workspace must hold the same records and whose point list must carry each Gaussian at most tiles
times, exactly tiles times for rectangles of at most 2 x 2 tiles.

The scenes are those of bwd_cases (PP_CASES and PP_EXTRA: 700 Gaussians on 83 x 61, three 256-row
blocks, the last one partial, 40 culled rows in the first; tests/test_backward_check.py and
tests/test_preprocess_fwd_check.py assert their preconditions on the oracle).

    case        inputs                                        kernel path
    M1          SH, 1 coefficient, degree 0                   MS = 1 (load_sh: scalar, 3 floats per row)
    M4          SH, 4 coefficients, degree 1                  MS = 4 (load_sh: float4)
    M9          SH, 9 coefficients, degree 2                  MS = 9 (load_sh: scalar, 27 floats per row)
    M16         SH, 16 coefficients, degree 3                 MS = 16 (load_sh: float4)
    M16_deg0/1/2  the same rows at sh_degree 0, 1, 2          MS = 16, degree below the stored one
    M25         SH, 25 coefficients, degree 3                 MS = 0, rows read from global memory
    COL         colors_precomp                                MS = 0, no SH
    COV         SH 16, cov3D_precomp                          MS = 16, no cov3d()
    M16_sm0.7   scale_modifier 0.7                            cov3d() with the modifier
    M16_off1    SH block one float past 16-byte alignment     MS = 16, load_sh's scalar branch
    M4_off1     the same for 4 coefficients                   MS = 4, load_sh's scalar branch
    M16_off4    SH block 16 bytes into a 256-byte line        MS = 16, load_sh's float4 branch off the line
    M4_off4     the same for 4 coefficients                   MS = 4, the same
    CLAMP       rows outside 1.3 tan(fov); faint opacities    the frustum clamp; radius without tiles
    NEAR        CLAMP + rows at z = 0.2f and beside it        the near cull at exactly z == 0.2f
    each of the above, 3 views of camera_batch(3, seed=31)    k_preprocess<MS, true>
    M16, 9 views                                              a launch of 8 views and one of 1
    M16, rows (0, 256), (256, 512), (512, 700)                row0 > 0

The misaligned runs must also equal the aligned ones bit for bit in every record, the row-chunked
run the plain one.  Batched views are each checked against the oracle of their own camera; that
the views differ is asserted on the oracle's radii.

Measured on an MI355X (recorded, not used to set any bound).  Every float field -- xy, conic and
opacity, colour, depth -- equals the float oracle's bit for bit in every case, view and visible
row: 0 differing elements, 0 ulps; no field needed a tolerance or the fallback to the float
oracle's distance from the double one.  Rows per view: visible / outside the 1.3 tan(fov) clamp /
visible without tiles (of these, with opacity <= 0.003), and the listed tiles against upstream's:

    one view, origin camera   M1 .. COV, M16_deg*, M*_off*   632 /  0 /  31 (0)    956 of 1245 tiles
                              M16_sm0.7                      629 /  0 /  38 (0)    862 of 1114
                              CLAMP                          631 / 46 /  59 (19)  1160 of 1570
                              NEAR                           628 / 46 /  59 (19)  1191 of 1616
    3 views, view 0 / 1 / 2   M16 and the cases on its scene 527, 610, 607 / 2, 22, 0 / 17, 103, 18
                              CLAMP                          530, 607, 606 / 32, 49, 44 / 41, 118, 48
                              NEAR                           528, 602, 607 / 32, 49, 44 / 41, 117, 48
    9 views                   M16                            525 .. 654 / 0 .. 30 / 8 .. 106

The yawed cameras of the batches put rows of the plain scenes outside the clamp too.  A visible row
without tiles is a faint one, or one whose tightened rectangle is empty or reaches no quadrant.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # CPU container: the driver only runs these on the MI355X box
    pytest.skip("needs a GPU", allow_module_level=True)

import diff_gaussian_rasterization as dgr  # noqa: E402
import bwd_cases  # noqa: E402
import oracle  # noqa: E402
import synthetic  # noqa: E402
from lsr_testutil import (decode_geom, decode_img, decode_point_list, preprocess_check, raster_settings,  # noqa: E402
                          run_native, run_oracle)

PREFILL = 0xA5
W, H = bwd_cases.BASE_W, bwd_cases.BASE_H
RECORDS = ("xy", "conic_o", "rgbd", "clamped", "tiles", "radius", "rect", "acc")   # what the preprocess writes per row

VARIANTS = {
    "M1": dict(case="M1"), "M4": dict(case="M4"), "M9": dict(case="M9"), "M16": dict(case="M16"),
    "M16_deg0": dict(case="M16", sh_degree=0), "M16_deg1": dict(case="M16", sh_degree=1),
    "M16_deg2": dict(case="M16", sh_degree=2),
    "M25": dict(case="M25"), "COL": dict(case="COL"), "COV": dict(case="COV"),
    "M16_sm0.7": dict(case="M16", scale_modifier=0.7),
    "M16_off1": dict(case="M16", sh_offset=1, aligned="M16"), "M4_off1": dict(case="M4", sh_offset=1, aligned="M4"),
    "M16_off4": dict(case="M16", sh_offset=4, aligned="M16"), "M4_off4": dict(case="M4", sh_offset=4, aligned="M4"),
    "CLAMP": dict(case="CLAMP"), "NEAR": dict(case="NEAR"),
}


def _cams(nv):
    """0: the scene's origin camera alone (one-view entry point); n: a camera batch."""
    return None if nv == 0 else synthetic.camera_batch(nv, W, H, seed=31)


def _run_kw(variant):
    v = VARIANTS[variant]
    kw = bwd_cases.case(v["case"]).run_kw()
    kw.update({k: v[k] for k in ("sh_degree", "scale_modifier") if k in v})
    return kw


@functools.lru_cache(maxsize=None)
def _oracle(variant, nv, view):
    """The float oracle's forward of one view; computed once, shared, never modified."""
    v = VARIANTS[variant]
    c = bwd_cases.case(v["case"])
    if nv == 0 and set(v) <= {"case", "sh_offset", "aligned"}:
        return bwd_cases.reference(v["case"]).views[0]
    cam = c.cams[0] if nv == 0 else _cams(nv)[view]
    return run_oracle(c.scene, cam, **_run_kw(variant))


def _inputs(variant):
    """The device tensors of a variant, as run_native passes them."""
    v = VARIANTS[variant]
    c = bwd_cases.case(v["case"])
    sc = c.scene
    kw = dict(means3D=sc.means3D.cuda(), opacities=sc.opacities.cuda(), language_feature=sc.lang.cuda())
    if c.cov3D:
        kw["cov3D_precomp"] = torch.tensor(oracle.cov3d(sc.scales.numpy(), sc.rotations.numpy())).cuda()
    else:
        kw["scales"], kw["rotations"] = sc.scales.cuda(), sc.rotations.cuda()
    if c.colors is not None:
        kw["colors_precomp"] = torch.as_tensor(c.colors).cuda()
    else:
        off = v.get("sh_offset", 0)
        buf = torch.zeros(sc.shs.numel() + 8, device="cuda")      # allocations are 256-byte aligned
        shs = buf[off:off + sc.shs.numel()].view(sc.shs.shape)
        shs.copy_(sc.shs)
        assert shs.is_contiguous() and shs.data_ptr() % 256 == 4 * off
        kw["shs"] = shs
    return kw


def _filled(nbytes):
    return torch.full((nbytes,), PREFILL, dtype=torch.uint8, device="cuda")


@functools.lru_cache(maxsize=None)
def _phase1(variant, nv, chunks=None):
    """Phase 1 of a variant into prefilled workspaces: a list of (decoded geom, radii, num_rendered)
    per view.  nv == 0: lsr_forward_preprocess on the origin camera; nv > 0:
    lsr_forward_preprocess_views_async on a camera batch; chunks (nv == 0): the rows in chunks."""
    L = dgr._lib.load()
    c = bwd_cases.case(VARIANTS[variant]["case"])
    cams = [c.cams[0]] if nv == 0 else _cams(nv)
    kw = _run_kw(variant)
    rss = [raster_settings(cam, bg=kw["bg"], sh_degree=kw["sh_degree"], scale_modifier=kw["scale_modifier"])
           for cam in cams]
    sts = [dgr._NativeSettings(rs, torch.device("cuda")) for rs in rss]
    inp = _inputs(variant)
    fin, inputs, P = dgr._fwd_inputs(inp["means3D"], inp["opacities"], inp.get("shs"), inp.get("colors_precomp"),
                                     inp["language_feature"], inp.get("scales"), inp.get("rotations"),
                                     inp.get("cov3D_precomp"))
    if "shs" in inp:
        assert fin.shs == inp["shs"].data_ptr()          # the wrapper passed the (mis)aligned view itself
    nbytes = int(L.lsr_geom_bytes(P))
    geoms = [_filled(nbytes) for _ in cams]
    radii = [_filled(4 * P).view(torch.int32) for _ in cams]
    fouts = [dgr._lib.FwdOut() for _ in cams]
    for fo, r in zip(fouts, radii):
        fo.radii = r.data_ptr()
    stream = torch.cuda.current_stream()
    stp = ctypes.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize()
    if nv == 0 and chunks is None:
        K = ctypes.c_int64(-1)
        dgr._lib.check(L.lsr_forward_preprocess(ctypes.byref(sts[0].c), ctypes.byref(fin), ctypes.byref(fouts[0]),
                                                ctypes.c_void_p(geoms[0].data_ptr()), ctypes.byref(K), stp),
                       "lsr_forward_preprocess")
        counts = [K.value]
    else:
        n = len(cams)
        host = torch.zeros(n, 2, dtype=torch.int32, pin_memory=True)
        s_arr, o_arr = dgr._settings_array(sts), dgr._struct_array(dgr._lib.FwdOut, fouts)
        g_arr = dgr._lib.Boundary(geoms[0].device).array(geoms, "geom", torch.uint8)
        if chunks is None:
            dgr._lib.check(L.lsr_forward_preprocess_views_async(n, s_arr, ctypes.byref(fin), o_arr, g_arr,
                                                                ctypes.c_void_p(host.data_ptr()), stp),
                           "lsr_forward_preprocess_views_async")
        else:
            for r0, r1 in chunks:
                dgr._lib.check(L.lsr_forward_preprocess_views_rows_async(n, r0, r1, s_arr, ctypes.byref(fin), o_arr,
                                                                         g_arr, stp),
                               "lsr_forward_preprocess_views_rows_async")
            dgr._lib.check(L.lsr_forward_depth_order_views_async(n, s_arr, ctypes.byref(fin), g_arr,
                                                                 ctypes.c_void_p(host.data_ptr()), stp),
                           "lsr_forward_depth_order_views_async")
        stream.synchronize()
        counts = [int(k) for k in host[:, 0]]
    torch.cuda.synchronize()
    return [(decode_geom(g.cpu().numpy(), P), r.cpu().numpy(), k) for g, r, k in zip(geoms, radii, counts)]


def _same_records(a, b, what):
    for k in RECORDS:
        x, y = (np.ascontiguousarray(d[k]).view(np.uint8) for d in (a[0], b[0]))
        assert np.array_equal(x, y), (what, k)
    assert np.array_equal(a[1], b[1]) and a[2] == b[2], (what, "radii or num_rendered")


def _check_view(variant, nv, view, got, point_list=None):
    ref = _oracle(variant, nv, view)
    c = bwd_cases.case(VARIANTS[variant]["case"])
    decoded, radii, K = got
    bad, stats = preprocess_check(decoded, radii, ref, W, H, point_list=point_list, num_rendered=K, prefill=PREFILL)
    cam = c.cams[0] if nv == 0 else _cams(nv)[view]
    vis = ref.radii > 0
    fig = dict(visible=stats["visible"], frustum_clamped=int((bwd_cases.frustum_clamped(c.scene, cam) & vis).sum()),
               unlisted_visible=stats["unlisted_visible"], faint_visible=stats["faint_visible"], tiles=stats["tiles"], upstream_tiles=stats["upstream_tiles"],
               ulps={k: stats[k]["max_ulps"] for k in ("xy", "conic_o", "rgb", "depth")})
    print("FIGURES", variant, f"views={nv}", f"view={view}", fig)
    assert not bad, (variant, nv, view, bad, stats)
    # not vacuous: visible and culled rows, rectangles with and without a quadrant map, dropped tiles
    assert stats["visible"] >= 300 and (~vis).sum() >= 20, (variant, stats)
    assert stats["small_rects"] >= 100 and stats["rect_rows"] - stats["small_rects"] >= 1, (variant, stats)
    assert 0 < stats["tiles"] < stats["upstream_tiles"], (variant, stats)
    if VARIANTS[variant]["case"] in bwd_cases.PP_EXTRA and nv == 0:
        assert fig["frustum_clamped"] >= 20 and fig["unlisted_visible"] >= 16, (variant, fig)
    return stats


def _preconditions(variant):
    name = VARIANTS[variant]["case"]
    bwd_cases.check_preprocess_preconditions(name, bwd_cases.reference(name))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_view(variant):
    _preconditions(variant)
    got = _phase1(variant, 0)[0]
    # the same view finished by the public entry point: its own workspace, its point list
    c = bwd_cases.case(VARIANTS[variant]["case"])
    state = run_native(c.scene, c.cams[0], **_run_kw(variant))[4]
    torch.cuda.synchronize()
    kept = int(decode_img(state)[0][:, 1].max(initial=0))
    assert 0 < kept <= state.num_rendered
    _check_view(variant, 0, 0, got, point_list=decode_point_list(state)[:kept])
    public = (decode_geom(state.geom.cpu().numpy(), c.scene.P), state.radii.cpu().numpy(), state.num_rendered)
    # the rows the kernel writes: a culled row's xy, conic_o and rgbd and an accumulator row without a
    # rectangle are the allocator's there and the prefill here
    every = np.ones(c.scene.P, bool)
    rows = dict(xy=got[1] > 0, conic_o=got[1] > 0, rgbd=got[1] > 0, acc=got[0]["rect_fields"]["area"] > 0)
    for k in RECORDS:
        x, y = (np.ascontiguousarray(d[k][rows.get(k, every)]).view(np.uint8) for d in (got[0], public[0]))
        assert np.array_equal(x, y), (variant, k)
    assert np.array_equal(got[1], public[1]) and got[2] == public[2], variant
    if "aligned" in VARIANTS[variant]:
        _same_records(got, _phase1(VARIANTS[variant]["aligned"], 0)[0], variant)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_three_views(variant):
    _preconditions(variant)
    got = _phase1(variant, 3)
    refs = [_oracle(variant, 3, v) for v in range(3)]
    assert not np.array_equal(refs[0].radii, refs[1].radii) and not np.array_equal(refs[1].radii, refs[2].radii)
    for v in range(3):
        _check_view(variant, 3, v, got[v])
    if "aligned" in VARIANTS[variant]:
        for v, (a, b) in enumerate(zip(got, _phase1(VARIANTS[variant]["aligned"], 3))):
            _same_records(a, b, (variant, v))


def test_nine_views():
    """LSR_MAX_VIEWS = 8: nine views are one launch of eight and one of one."""
    _preconditions("M16")
    got = _phase1("M16", 9)
    refs = [_oracle("M16", 9, v) for v in range(9)]
    assert len({r.radii.tobytes() for r in refs}) == 9
    for v in range(9):
        _check_view("M16", 9, v, got[v])


def test_row_chunks():
    """The rows in three launches (row0 = 0, 256, 512; the last one partial), then the depth order."""
    _preconditions("M16")
    P = bwd_cases.PP_P
    got = _phase1("M16", 0, chunks=((0, 256), (256, 512), (512, P)))[0]
    _check_view("M16", 0, 0, got)
    _same_records(got, _phase1("M16", 0)[0], "row chunks")
