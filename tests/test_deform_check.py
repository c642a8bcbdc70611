"""The measure of tests/test_deform_branches_gpu.py judged on the CPU: the oracle's term scales, its
float32 coordinate mode and its box gradient; the bf16x3 emulation under deform_check at the
coefficient the GPU module uses (and under half of it: the condition of lsr_testutil.DEFORM_COEF);
the case table's tile counts; and the teeth -- doctored gradients that the tensor-wide
max|a - b| / max|b| < 1e-4 of test_deform_gpu.py passes and deform_check refuses, and, on the
references the GPU module itself compares with, wrong boxes, zeroed plane gradients and outputs and
gradients a few per cent off that deform_check refuses."""
import numpy as np
import pytest

import deform_cases as dc
from deform_oracle import DeformOracle
from lsr_testutil import DEFORM_COEF, deform_check

KEYS = dc.KEYS


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _oracle(x, **kw):
    return DeformOracle(x["params"], x["aabb"], cfg=x["cfg"], train_aabb=True, **kw)


def _fwd(o, x, rows=slice(None), **kw):
    return o.forward(*[x["inp"][k][rows] for k in KEYS], None if x["lang"] is None else x["lang"][rows], x["times"][rows],
                     **kw)


# ---- the case table ---------------------------------------------------------------------------------
def test_case_table_states_the_launchers_tile_counts():
    """T of k_head_wgrad3 and k_head_wgrad2 and k_atb's rows per block of every case, recomputed from
    the launchers' formulas (deform_cases' docstring quotes them); the regimes the issue names are
    all there, and every window of a tile case has rows."""
    seen3, seen2, seen_atb = set(), set(), set()
    for name, c in dc.CASES.items():
        cfg = dc.inputs(name)["cfg"] if c["variant"] else None
        heads = cfg.heads if cfg else c["heads"]
        ns = sum(heads[:4]) + int(bool(cfg) and cfg.lang_mode == "discrete")
        t3, t2, atb = dc.tiles(c["P"], ns, int(heads[4]))
        if ns:
            assert t3 == c["T3"], name
            seen3.add(t3)
        if heads[4]:
            assert t2 == c["T2"], name
            seen2.add(t2)
        assert atb == c["atb"], name
        seen_atb.add(atb)
    assert {1, 2, 3, 4} <= seen3 and {1, 3} <= seen2 and seen_atb == {64, 128}
    c = dc.CASES["tiles_T2"]
    assert c["P"] - (c["P"] - 1) // (64 * c["T3"]) * (64 * c["T3"]) == 1          # a last block of one row
    for name in dc.TILE_CASES:
        P = dc.CASES[name]["P"]
        first, last = dc.window_rows(name, "first_tile"), dc.window_rows(name, "last_tile")
        assert len(first) and len(last) and last[-1] == P - 1 and first[0] == 0
        assert list(dc.window_rows(name, "last_row")) == [P - 1]
        if dc.CASES[name]["T3"] > 1:
            assert not set(first[:64]) & set(last)


@pytest.mark.parametrize("name", list(dc.CASES))
def test_kink_mask_stays_under_the_cap(name):
    """The Gaussians whose upstream is zeroed (a ReLU input within 1e-4 of zero) stay under the share
    the existing tests assert; a window of a single row keeps that row."""
    for w in dc.windows(name):
        amb = dc.kink_rows(name, w)
        assert (amb.mean() < dc.KINK_CAP) if len(amb) >= 10 else not amb.all(), (name, w)


def test_cases_put_points_on_lines_faces_and_outside():
    """Every case has points whose float32 pixel coordinate is an integer (on a line), points on a
    face of the box (|n| = 1 to an ulp) and, from P = 64 on, points outside; times +-1 and beyond."""
    for name, c in dc.CASES.items():
        x = dc.inputs(name)
        q = _oracle(x, coords="float32").normalised(x["inp"]["means3D"], x["times"])
        r = (q[:, 0] + np.float32(1)) * np.float32(0.5) * np.float32(x["res"][0] * x["multires"][0] - 1)
        assert (r == np.floor(r)).any() or c["P"] == 1, name
        assert (np.abs(np.abs(q[:, :3]) - 1) < 1e-6).any(), name
        if c["P"] >= 64:
            assert (np.abs(q[:, :3]) > 1.01).any() and (np.abs(q[:, 3]) > 1).any() and (q[:, 3] == 1).any() \
                and (q[:, 3] == -1).any(), name


# ---- the oracle's term scales -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("S2_P300", "apply_rotation", "depth3_S1", "variant_lang", "variant_noresnet",
                                  "variant_discrete", "narrow_on_lines"))
def test_term_scale_bounds_the_value(name):
    r = dc.reference(name)
    for val, A in ((r["out"], r["A_out"]), (r["g_in"], r["A_in"]), (r["g"], r["A_g"])):
        assert set(A) == set(val)
        for k, v in dc.offsets(name, val, r["rows"]).items() if val is r["out"] else val.items():
            a = np.asarray(A[k]).reshape(np.shape(v))
            assert (a >= np.abs(v) * (1 - 1e-12)).all(), (name, k)


def test_term_scale_equals_the_value_without_cancellation():
    """Planes, weights, biases and upstreams non-negative, every point inside the box: no product
    changes sign and no mask cuts, so A is the value itself to rounding -- for the output offsets and
    the plane, weight and bias gradients.  (The coordinate gradient and the box take tap differences
    and n -+ 1, which cancel whatever the signs: there A only bounds.)"""
    x = dict(dc.inputs("S2_P300"))
    x["params"] = {k: np.abs(v) for k, v in x["params"].items()}
    rng = np.random.default_rng(5)
    x["inp"] = dict(x["inp"], means3D=rng.uniform(x["aabb"][1] + 0.05, x["aabb"][0] - 0.05, size=(300, 3)))
    x["times"] = rng.uniform(-0.9, 0.9, size=(300, 1))
    o = _oracle(x)
    out, A_out = _fwd(o, x, abs_terms=True)
    g_in, g, A_in, A_g = o.backward(*[np.abs(x["ups"][k]) for k in KEYS], abs_terms=True)
    for k in ("means3D", "scales", "rotations", "opacity", "shs"):
        np.testing.assert_allclose(A_out[k], out[k] - x["inp"][k], rtol=1e-9, atol=0)
    for k, v in g.items():
        if k != "grid.aabb":
            np.testing.assert_allclose(A_g[k], v, rtol=1e-9, atol=0, err_msg=k)
    assert (A_in["means3D"] >= np.abs(g_in["means3D"])).all() and (A_g["grid.aabb"] >= np.abs(g["grid.aabb"])).all()


def _off_lines(x, n=200, seed=3):
    """The case's inputs with n fresh points kept 1e-3 cells from every grid line (the existing tests'
    exclusion)."""
    rng = np.random.default_rng(seed)
    a0, a1 = x["aabb"]
    pts = np.asarray(rng.uniform(a1 - 0.1, a0 + 0.1, size=(8 * n, 3)), np.float32).astype(np.float64)
    crd = (pts - a0) * (2.0 / (a1 - a0)) - 1.0
    keep = np.ones(len(pts), bool)
    for m in x["multires"]:
        u = (crd + 1.0) * 0.5 * (np.array(x["res"][:3]) * m - 1)
        keep &= (np.abs(u - np.round(u)) > 1e-3).all(1)
    y = dict(x)
    y["inp"] = {k: v[:n] for k, v in x["inp"].items()}
    y["inp"]["means3D"] = pts[keep][:n]
    t = np.asarray(rng.uniform(-1.2, 1.2, size=(n, 1)), np.float32).astype(np.float64)
    t[::5] = 1.0
    y["times"], y["ups"] = t, {k: v[:n] for k, v in x["ups"].items()}
    assert len(y["inp"]["means3D"]) == n
    return y


def test_box_gradient_agrees_with_central_differences():
    """grid.aabb of the oracle against fp64 central differences of its own forward (float64
    coordinates, points off the lines, kink-ambiguous Gaussians without upstream)."""
    x = _off_lines(dc.inputs("S2_P64"), n=48)
    o = _oracle(x)
    _fwd(o, x)
    amb = np.zeros(48, bool)
    for z in o.preactivations():
        amb |= (np.abs(z) < 1e-4).any(1)
    ups = {k: np.where(amb.reshape((-1,) + (1,) * (v.ndim - 1)), 0.0, v) for k, v in x["ups"].items()}
    g = o.backward(*[ups[k] for k in KEYS])[1]["grid.aabb"]

    def loss(aabb):
        out = _fwd(DeformOracle(x["params"], aabb, cfg=x["cfg"]), x)
        return sum((out[k] * ups[k]).sum() for k in KEYS)
    fd = np.zeros((2, 3))
    for i in range(2):
        for j in range(3):
            d = np.zeros((2, 3))
            d[i, j] = 1e-6
            fd[i, j] = (loss(x["aabb"] + d) - loss(x["aabb"] - d)) / 2e-6
    assert _rel(g, fd) < 1e-6, (g, fd)


# ---- coords="float32" ---------------------------------------------------------------------------------
def test_float32_coordinates_off_the_lines_match_float64():
    """Off the lines both modes take the same cells and masks, and every output and gradient
    agrees within the existing tensor-wide 1e-4 (the fractions differ by float32 rounding)."""
    x = _off_lines(dc.inputs("S2_P300"))
    res = {}
    for mode in ("float64", "float32"):
        o = _oracle(x, coords=mode)
        out = _fwd(o, x)
        res[mode] = (out, o._cache[1]) + o.backward(*[x["ups"][k] for k in KEYS])
    for (v64, t64), (v32, t32) in zip(res["float64"][1], res["float32"][1]):
        for a, b in zip(t64, t32):
            for i in (0, 1, 2, 3, 10, 11):                                       # cells and masks
                assert np.array_equal(a[i], b[i])
    for k in KEYS:
        assert _rel(res["float32"][0][k] - x["inp"][k], res["float64"][0][k] - x["inp"][k]) < 1e-4, k
    assert _rel(res["float32"][2]["means3D"], res["float64"][2]["means3D"]) < 1e-4
    for k, v in res["float64"][3].items():
        assert _rel(res["float32"][3][k], v) < 1e-4, k


def test_float32_coordinates_decide_differently_on_the_lines():
    """On a case's own points (a quarter on grid lines, some on faces) float32 and float64 pick
    different cells or masks for some Gaussians, and the plane gradients differ by far more than
    1e-4: the mode matters."""
    x = dc.inputs("S2_P300")
    taps, grads = {}, {}
    for mode in ("float64", "float32"):
        o = _oracle(x, coords=mode)
        _fwd(o, x)
        taps[mode] = o._cache[1]
        grads[mode] = o.backward(*[x["ups"][k] for k in KEYS])[1]
    cells = masks = 0
    for (_, t64), (_, t32) in zip(taps["float64"], taps["float32"]):
        for a, b in zip(t64, t32):
            cells += int(((a[0] != b[0]) | (a[2] != b[2])).sum())
            masks += int(((a[10] != b[10]) | (a[11] != b[11])).sum())
    assert cells > 0 and masks > 0, (cells, masks)
    assert max(_rel(grads["float32"][k], v) for k, v in grads["float64"].items()) > 1e-4


# ---- the emulation under the check ----------------------------------------------------------------------
def _check_all(name, got, ref):
    bad, stats = {}, {}
    for what, g, r, A in (("forward", dc.offsets(name, got["out"], ref["rows"]), dc.offsets(name, ref["out"], ref["rows"]),
                           ref["A_out"]), ("inputs", got["g_in"], ref["g_in"], ref["A_in"]),
                          ("param", got["g"], ref["g"], ref["A_g"])):
        b, s = deform_check(g, r, A, DEFORM_COEF)
        bad.update(b)
        stats.update({(what, k): v["max_err_over_A"] for k, v in s.items()})
    return bad, stats


@pytest.mark.parametrize("name", dc.CPU_CASES)
def test_emulation_passes_the_check_at_half_the_coefficient(name):
    """products="bf16x3" against the float64 oracle, both on the float32 coordinates: passes
    deform_check at DEFORM_COEF, and its largest err / A stays under half of it -- the condition
    under which DEFORM_COEF is grad_check's 1e-4 (largest over the cases: 2.3e-5)."""
    worst = 0.0
    for w in dc.windows(name):
        bad, stats = _check_all(name, dc.reference(name, w, products="bf16x3"), dc.reference(name, w))
        assert not bad, (name, w, bad)
        k = max(stats, key=stats.get)
        worst = max(worst, stats[k])
        print(f"\nEMULATION_ERR_OVER_A {name} {w} {stats[k]:.2e} at {k}")
    assert worst < DEFORM_COEF / 2


# ---- teeth ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teeth():
    """S2_P300's inputs with what a rendered frame has: most Gaussians count little.  The upstream of
    the Gaussians at |t| >= 1 or outside 0.8 of the box is scaled by 3e-6 and that of one SH channel
    by 1e-5, so that the border cells, the clamped time rows and one row of shs_deform.3.weight are
    small beside their tensors' largest elements."""
    x = dc.inputs("S2_P300")
    q = _oracle(x, coords="float32").normalised(x["inp"]["means3D"], x["times"]).astype(np.float64)
    far = (np.abs(q[:, :3]) > 0.8).any(1) | (np.abs(q[:, 3]) >= 1)
    amb = dc.kink_rows("S2_P300")
    assert 0.05 < (~far).mean() < 0.5
    ups = {k: v.copy() for k, v in x["ups"].items()}
    for v in ups.values():
        v[amb] = 0.0
        v[far] *= 3e-6
    ups["shs"][:, 5, 1] *= 1e-5

    def run(ups, **kw):
        o = _oracle(x, coords="float32", **kw)
        _fwd(o, x, abs_terms=True)
        return o.backward(*[ups[k] for k in KEYS], abs_terms=True)
    g_in, g, A_in, A_g = run(ups)
    return dict(x=x, far=far, amb=amb, ups=ups, run=run, g=g, A_g=A_g)


def _old_passes_new_fails(t, doctored, keys):
    for k, v in t["g"].items():
        if k != "grid.aabb":                       # the 16 / 128 tests compared no box gradient at all
            assert _rel(doctored.get(k, v), v) < 1e-4, k
    bad, _ = deform_check({k: doctored[k] for k in keys}, t["g"], t["A_g"], DEFORM_COEF)
    assert set(bad) == set(keys), bad
    return bad


def test_teeth_cells_with_the_least_inflow_zeroed(teeth):
    """Every plane-gradient cell under 5e-5 of its tensor's largest (border cells and cells of the
    clamped time rows of the teeth fixture among them) set to zero, in a spatial and in two time planes."""
    keys = ("grid.grids.1.0", "grid.grids.0.2", "grid.grids.1.4")
    doctored = {}
    for k in keys:
        v = teeth["g"][k].copy()
        small = (np.abs(v) < 5e-5 * np.abs(v).max()) & (v != 0)
        assert small.sum() > v.size // 4
        assert small[0, :, 0, :].any() and small[0, :, -1, :].any()             # border rows (time planes: the clamped rows)
        v[small] = 0.0
        doctored[k] = v
    bad = _old_passes_new_fails(teeth, doctored, keys)
    assert all(b["elements"] > 100 for b in bad.values())


def test_teeth_smallest_row_of_the_sh_output_weight_zeroed(teeth):
    k = "shs_deform.3.weight"
    v = teeth["g"][k].copy()
    row = int(np.abs(v).max(1).argmin())
    assert row == 16                                                            # channel [5, 1], the scaled one
    v[row] = 0.0
    bad = _old_passes_new_fails(teeth, {k: v}, (k,))
    assert all(ix[0][0] == row for ix in bad[k]["first"])


def test_teeth_one_gaussian_removed_from_shared_cells(teeth):
    """One of the little-counting Gaussians contributes nothing: the cells it shares with many
    others change by its share only."""
    i = int(np.flatnonzero(teeth["far"] & ~teeth["amb"])[3])
    ups = {k: v.copy() for k, v in teeth["ups"].items()}
    for v in ups.values():
        v[i] = 0.0
    g2 = teeth["run"](ups)[1]
    keys = ("grid.grids.0.0", "grid.grids.1.0")
    for k in keys:
        changed = g2[k] != teeth["g"][k]
        assert changed.any() and (np.abs(g2[k][changed]) > 0).all()             # shared cells: others remain
    _old_passes_new_fails(teeth, {k: g2[k] for k in keys}, keys)


def test_teeth_box_face_with_the_sign_flipped(teeth):
    """grid.aabb with its largest face's sign flipped is caught by that element.  No test of the
    16 / 128 family compared a box gradient before."""
    v = teeth["g"]["grid.aabb"].copy()
    ix = np.unravel_index(np.abs(v).argmax(), v.shape)
    v[ix] = -v[ix]
    bad = _old_passes_new_fails(teeth, {"grid.aabb": v}, ("grid.aabb",))
    assert bad["grid.aabb"]["elements"] == 1 and bad["grid.aabb"]["first"][0][0] == tuple(ix)


# ---- teeth on the references the GPU module compares with ---------------------------------------------------
def _failing(native, ref, A):
    bad, _ = deform_check(native, ref, A, DEFORM_COEF)
    return {k: b["elements"] for k, b in bad.items()}


@pytest.mark.parametrize("name,window", [("time_rows", None), ("S2_P300", None), ("small_heads_only", None),
                                         ("apply_rotation", None), ("variant_lang", None), ("variant_discrete", None),
                                         ("depth4_S2", None), ("tiles_T3", "first_tile"), ("tiles_T4", None),
                                         ("narrow_on_lines", None)])
def test_teeth_box_on_the_cases_own_references(name, window):
    """On a case's own reference (time_rows is the call that wraps the 64 box slots): grid.aabb with
    its largest face's sign flipped fails on that element, a box gradient of zeros fails in five of its six
    elements at least and one at half its value in three.  (A sum over thousands of Gaussians
    cancels: A is 40 to 9,000 times the element there, and the share of one of 64 box slots alone
    stays under 1e-4 A at the large sizes.)"""
    r = dc.reference(name, window)
    g = r["g"]["grid.aabb"]
    v = g.copy()
    ix = np.unravel_index(np.abs(v).argmax(), v.shape)
    v[ix] = -v[ix]
    bad, _ = deform_check({"grid.aabb": v}, r["g"], r["A_g"], DEFORM_COEF)
    assert [b[0] for b in bad["grid.aabb"]["first"]] == [tuple(ix)]
    assert _failing({"grid.aabb": np.zeros_like(g)}, r["g"], r["A_g"])["grid.aabb"] >= 5
    assert _failing({"grid.aabb": 0.5 * g}, r["g"], r["A_g"])["grid.aabb"] >= 3


@pytest.mark.parametrize("name", ("depth3_S1", "depth4_S2", "depth3_S3", "depth4_S4", "apply_rotation_deep"))
def test_teeth_on_the_deep_cases_own_references(name):
    """The only cover of k_deform_bwd_a<S, true> must bite: on the case's own reference, plane
    gradients of zeros fail in most of the cells anything flows into, forward offsets off by 10 %
    fail in most elements, input gradients without their coordinate part fail, and parameter
    gradients at half their value fail in a third of the elements at least."""
    r = dc.reference(name)
    g, A = r["g"], r["A_g"]
    planes = {k: np.zeros_like(v) for k, v in g.items() if k.startswith("grid.grids")}
    inflow = sum(int((g[k] != 0).sum()) for k in planes)
    assert sum(_failing(planes, g, A).values()) > 0.5 * inflow
    off = dc.offsets(name, r["out"], r["rows"])
    assert sum(_failing({k: 0.9 * v for k, v in off.items()}, off, r["A_out"]).values()) > 0.5 * sum(v.size for v in off.values())
    assert _failing({"means3D": r["ups"]["means3D"]}, r["g_in"], r["A_in"])["means3D"] > 0
    assert sum(_failing({k: 0.5 * v for k, v in g.items()}, g, A).values()) > sum(v.size for v in g.values()) / 3


@pytest.mark.parametrize("name,window", [("S2_P300", None), ("S1_P1", None), ("S4_P65", None), ("time_rows", None),
                                         ("sh_head_only", None), ("variant_noresnet", None), ("tiles_T2", "last_row"),
                                         ("tiles_T4", None), ("tiles_T3", "last_tile"), ("narrow_on_lines", None)])
def test_teeth_on_the_plain_cases_own_references(name, window):
    """One case of every group on its own reference: plane gradients of zeros fail in most cells
    anything flows into, weight gradients 10 % off fail in every tensor and 1 % off (a tile of 100
    dropped or read twice) in a tenth of the elements at least, and forward offsets 1 % off fail."""
    r = dc.reference(name, window)
    g, A = r["g"], r["A_g"]
    planes = {k: np.zeros_like(v) for k, v in g.items() if k.startswith("grid.grids")}
    assert sum(_failing(planes, g, A).values()) > 0.5 * sum(int((g[k] != 0).sum()) for k in planes)
    weights = {k: v for k, v in g.items() if k.endswith(".weight")}
    assert set(_failing({k: 0.9 * v for k, v in weights.items()}, g, A)) == set(weights)
    assert sum(_failing({k: 0.99 * v for k, v in weights.items()}, g, A).values()) > 0.1 * sum(v.size for v in weights.values())
    off = dc.offsets(name, r["out"], r["rows"])
    assert _failing({k: 0.99 * v for k, v in off.items()}, off, r["A_out"])


def test_dropped_lo_hi_term_is_seen_by_both(teeth):
    """Sanity: the emulation with the lo hi term left out of one layer (pos_deform.1) fails
    deform_check in that layer's gradients -- and already fails the tensor-wide 1e-4 (2e-3 on
    pos_deform.1.weight): an error of 2^-9 per product is no subtle one.  The full emulation passes
    both."""
    full = teeth["run"](teeth["ups"], products="bf16x3")[1]
    drop = teeth["run"](teeth["ups"], products="bf16x3", drop_lo_hi="pos_deform.1")[1]
    assert not deform_check(full, teeth["g"], teeth["A_g"], DEFORM_COEF)[0]
    assert all(_rel(full[k], v) < 1e-4 for k, v in teeth["g"].items())
    bad, _ = deform_check(drop, teeth["g"], teeth["A_g"], DEFORM_COEF)
    assert "pos_deform.1.weight" in bad and "feature_out.0.weight" in bad
    assert _rel(drop["pos_deform.1.weight"], teeth["g"]["pos_deform.1.weight"]) > 1e-4
