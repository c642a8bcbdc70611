"""The per-Gaussian forward check (lsr_testutil.preprocess_check, decode_geom) and the scenes CLAMP
and NEAR of tests/test_preprocess_fwd_branches_gpu.py (bwd_cases.PP_EXTRA), on the oracle alone.

(a) the float oracle's own state, laid out as a decoded geom workspace -- upstream's full rectangle
    per visible Gaussian, a full quadrant map where it is at most 2 x 2 tiles and none otherwise,
    nothing for an opacity below 1 / 255, accumulator rows zeroed under a rectangle and the prefill
    elsewhere -- passes preprocess_check whole, the point-list rules included: the check asks
    nothing the reference's state does not have.
(b) the check has teeth: each single corruption of that state fails it, under the rule meant --
    one xy component, one opacity, one colour channel or one depth moved by one ulp, one clamped bit
    flipped, a culled row left with tiles or with a rect, tiles != rect_count(rect), a rectangle one
    tile outside upstream's, a nonzero accumulator word under a rectangle, a visible row of opacity
    0.001 listed with one tile.
(c) CLAMP and NEAR hold their preconditions (bwd_cases.check_preprocess_preconditions: at least 20
    visible frustum-clamped rows, 16 visible rows of opacity <= 0.003, 20 frustum-clamped rows with a
    means3D gradient; NEAR culls z <= 0.2f and keeps the rows just past it), and on CLAMP the float
    oracle passes grad_check against the double oracle with the same radii, so the backward test's
    bound is one the reference meets without any kernel.  Measured: 46 frustum-clamped visible rows,
    39 of them with a gradient (largest |means3D gradient| 117), 19 faint visible rows; float
    against double grad_err <= 5.7e-6 in every field, err / A language 2.3e-5, means2D 1.5e-5,
    opacity 1.4e-5 (bound 1e-4).
(d) decode_geom reads back a byte buffer packed on the host by the stated layout, P = 700 (no
    multiple of 64), with the sort / scan workspaces and every alignment gap filled with another byte.
"""
import numpy as np
import pytest

import bwd_cases
import diff_gaussian_rasterization as dgr
from lsr_testutil import ACC_PITCH, decode_geom, grad_check, preprocess_check, rect_pack, rect_unpack, upstream_rect

PREFILL = 0xA5
W, H = bwd_cases.BASE_W, bwd_cases.BASE_H


def oracle_as_geom(ref):
    """(decoded, radii, point_list, num_rendered): the float oracle's state in the place of a decoded
    geom workspace (module docstring (a)); every array is a fresh copy."""
    st = ref.state()
    P = len(ref.radii)
    vis = ref.radii > 0
    listed = vis & (st["conic_o"][:, 3] >= np.float32(1.0 / 255.0))
    x0, y0, x1, y1 = (np.where(listed, a, 0) for a in upstream_rect(st["xy"], ref.radii, W, H))
    small = (x1 - x0 <= 2) & (y1 - y0 <= 2)
    qmap = np.zeros(P, np.int64)
    for dy in range(2):
        for dx in range(2):
            inside = listed & small & (x0 + dx < x1) & (y0 + dy < y1)
            qmap |= np.where(inside, (0x03 << (2 * dx) | 0x30 << (2 * dx)) << (8 * dy), 0)
    rect = rect_pack(x0, y0, x1, y1, qmap)
    f = rect_unpack(rect)
    assert np.array_equal(f["count"][listed], st["tiles"][listed])       # full maps: upstream's counts
    acc = np.full((P, ACC_PITCH), PREFILL * 0x01010101, np.uint32)
    acc[f["area"] > 0] = 0
    decoded = dict(xy=st["xy"].copy(), conic_o=st["conic_o"].copy(),
                   rgbd=np.concatenate([st["rgb"], st["depth"][:, None]], axis=1),
                   clamped=(st["clamped"] * np.array([1, 2, 4], np.uint8)).sum(axis=1).astype(np.uint8),
                   tiles=f["count"].astype(np.uint32), radius=ref.radii.astype(np.int32), rect=rect,
                   acc=acc.view(np.float32), rect_fields=f)
    pl = st["point_list"].astype(np.int64)
    return decoded, ref.radii.copy(), pl[listed[pl]], int(f["count"].sum())


def _ref(name):
    return bwd_cases.reference(name).views[0]


@pytest.mark.parametrize("name", ["M16", "CLAMP", "NEAR"])
def test_oracle_state_passes(name):
    ref = _ref(name)
    d, radii, pl, K = oracle_as_geom(ref)
    bad, stats = preprocess_check(d, radii, ref, W, H, point_list=pl, num_rendered=K, prefill=PREFILL)
    print(name, stats)
    assert not bad, (name, bad)
    assert stats["visible"] > 500 and stats["small_rects"] > 100 and stats["rect_rows"] > stats["small_rects"]
    assert all(stats[k] == dict(differing=0, max_ulps=0) for k in ("xy", "conic_o", "rgb", "depth"))
    assert (stats["unlisted_visible"] >= 16) == (name != "M16")


def _bump(a, idx):
    a[idx] = np.nextafter(a[idx], np.float32(np.inf))


CORRUPTIONS = {
    "xy": {"xy"}, "opacity": {"conic_o"}, "colour": {"rgb"}, "depth": {"depth"}, "clamped_bit": {"clamped"},
    "culled_tiles": {"culled_tiles", "tiles_vs_rect_count", "tiles_above_upstream"},
    "culled_rect": {"culled_rect", "tiles_vs_rect_count", "rect_outside_upstream", "acc_not_zeroed"},
    "tiles_count": {"tiles_vs_rect_count"}, "rect_outside": {"rect_outside_upstream"},
    "acc_word": {"acc_not_zeroed"}, "faint_listed": {"faint_listed", "tiles_vs_rect_count"},
}
# the rule each corruption is meant for (the other names above follow from the same edit)
MEANT = dict(xy="xy", opacity="conic_o", colour="rgb", depth="depth", clamped_bit="clamped", culled_tiles="culled_tiles",
             culled_rect="culled_rect", tiles_count="tiles_vs_rect_count", rect_outside="rect_outside_upstream",
             acc_word="acc_not_zeroed", faint_listed="faint_listed")


@pytest.mark.parametrize("what", list(CORRUPTIONS))
def test_single_corruption_is_rejected(what):
    ref = _ref("CLAMP")
    d, radii, _, _ = oracle_as_geom(ref)
    st, f = ref.state(), d["rect_fields"]
    vis = ref.radii > 0
    row = int(np.nonzero(vis & (d["tiles"] > 0) & ~f["small"])[0][3])       # visible, listed, no map
    culled = int(np.nonzero(~vis)[0][5])
    if what == "xy":
        _bump(d["xy"], (row, 1))
    elif what == "opacity":
        _bump(d["conic_o"], (row, 3))
    elif what == "colour":
        ch = int(np.argmax(st["rgb"][row] > 0))
        _bump(d["rgbd"], (row, ch))
    elif what == "depth":
        _bump(d["rgbd"], (row, 3))
    elif what == "clamped_bit":
        d["clamped"][row] ^= 2
    elif what == "culled_tiles":
        d["tiles"][culled] = 1
    elif what == "culled_rect":
        d["rect"][culled] = rect_pack(1, 1, 2, 2, 0)
    elif what == "tiles_count":
        d["tiles"][row] -= 1
    elif what == "rect_outside":
        ux0 = upstream_rect(st["xy"], ref.radii, W, H)[0]
        row = int(np.nonzero(vis & (d["tiles"] > 0) & ~f["small"] & (ux0 > 0))[0][0])
        d["rect"][row] = rect_pack(f["x0"][row] - 1, f["y0"][row], f["x1"][row] - 1, f["y1"][row], 0)
    elif what == "acc_word":
        d["acc"].view(np.uint32)[row, ACC_PITCH - 1] = 1                    # the last, unused float: a denormal
    else:
        row = int(np.nonzero(vis & (st["conic_o"][:, 3] == np.float32(0.001)))[0][0])
        d["tiles"][row] = 1
    bad, _ = preprocess_check(d, radii, ref, W, H, prefill=PREFILL)
    assert MEANT[what] in bad and set(bad) <= CORRUPTIONS[what], (what, bad)


@pytest.mark.parametrize("what", ["dropped", "extra"])
def test_point_list_rules_reject(what):
    ref = _ref("CLAMP")
    d, radii, pl, K = oracle_as_geom(ref)
    small = np.nonzero(d["rect_fields"]["small"] & (d["tiles"] > 0))[0]
    if what == "dropped":       # a small rectangle must be listed on every tile it counts
        pl = np.delete(pl, np.nonzero(pl == small[0])[0][0])
    else:                       # nothing is listed more often than its count
        pl = np.append(pl, small[0])
    bad, _ = preprocess_check(d, radii, ref, W, H, point_list=pl, num_rendered=K, prefill=PREFILL)
    assert set(bad) == {"list_counts"}, bad
    bad, _ = preprocess_check(d, radii, ref, W, H, point_list=pl, num_rendered=K + 1, prefill=PREFILL)
    assert set(bad) == {"list_counts", "num_rendered"}, bad


@pytest.mark.parametrize("name", list(bwd_cases.PP_EXTRA))
def test_scene_preconditions(name):
    print(name, bwd_cases.check_preprocess_preconditions(name, bwd_cases.reference(name)))


def test_clamp_f32_oracle_passes_against_f64():
    r32, r64 = bwd_cases.reference("CLAMP"), bwd_cases.reference("CLAMP", True)
    np.testing.assert_array_equal(r32.views[0].radii, r64.views[0].radii)
    bad, stats = grad_check(r32.grads, r64.grads, r64.abs)
    print(stats)
    assert not bad, (bad, stats)
    assert set(stats) >= {"means3D", "means2D", "opacity", "colors", "lang", "sh", "scales", "rotations"}


def test_decode_geom_round_trip():
    P = bwd_cases.PP_P
    assert P % 64 != 0
    total = int(dgr._lib.load().lsr_geom_bytes(P))
    rng = np.random.default_rng(3)
    # the stated layout, written out: (name, bytes per Gaussian), every array on a 256-byte boundary
    layout = [("xy", 8), ("conic_o", 16), ("rgbd", 16), ("clamped", 1), ("tiles", 4), ("key_a", 4), ("key_b", 4),
              ("val_a", 4), ("val_b", 4), ("counts", 4), ("offsets", 4), ("inst_off", 4), ("radius", 4), ("rect", 8),
              ("rect_sorted", 8)]
    buf = np.full(total, 0xEE, np.uint8)
    want, off = {}, 0
    for name, nb in layout:
        want[name] = rng.integers(0, 256, P * nb, dtype=np.uint8)
        buf[off:off + P * nb] = want[name]
        off += (P * nb + 255) // 256 * 256
    want["total"] = rng.integers(0, 256, 16, dtype=np.uint8)
    buf[off:off + 16] = want["total"]
    want["acc"] = rng.integers(0, 256, P * 64, dtype=np.uint8)
    acc_off = total - (P * 64 + 255) // 256 * 256
    assert acc_off >= off + 256
    buf[acc_off:acc_off + P * 64] = want["acc"]
    d = decode_geom(buf, P)
    for name, w in want.items():
        assert np.array_equal(np.ascontiguousarray(d[name]).view(np.uint8).reshape(-1), w), name
    assert d["xy"].shape == (P, 2) and d["conic_o"].shape == d["rgbd"].shape == (P, 4) and d["rect"].shape == (P, 2)
    assert d["acc"].shape == (P, ACC_PITCH) and d["radius"].dtype == np.int32 and d["clamped"].dtype == np.uint8
    assert d["tmp_bytes"] == acc_off - off - 256
    f = d["rect_fields"]
    r = d["rect"].astype(np.int64)
    assert np.array_equal(rect_pack(f["x0"], f["y0"], f["x1"], f["y1"], f["qmap"]), d["rect"])
    assert np.array_equal(f["qmap"], (r[:, 0] >> 24) + 256 * (r[:, 1] >> 24))
    with pytest.raises(AssertionError):
        decode_geom(buf[:-256], P)


def test_rect_count_follows_the_header():
    """rect_count on the cases of lsr_internal.h: a large rectangle counts its tiles, a small one its
    tiles with a reachable quadrant, an empty one nothing."""
    rect = rect_pack([0, 1, 1, 1, 3], [0, 2, 2, 2, 3], [3, 3, 3, 2, 3], [2, 4, 4, 3, 5], [0, 0x0304, 0xFFFF, 0, 0])
    f = rect_unpack(rect)
    assert f["count"].tolist() == [6, 2, 4, 0, 0] and f["small"].tolist() == [False, True, True, True, True]
    assert f["mask"].tolist() == [0, 6, 15, 0, 0]
