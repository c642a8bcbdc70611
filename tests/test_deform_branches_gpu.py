"""Every reachable instantiation of the deformation field's kernels (csrc/deform*.hip), element by
element against the oracle: a forward and a backward through DeformationField with train_aabb on,
under lsr_testutil.deform_check -- |native - ref| <= 1e-4 |ref| + 1e-4 A per element, exactly 0 where
A = 0 -- with ref the float64 oracle on the kernels' own float32 cell and border decisions and A the
oracle's term scales.  The cases, what each one reaches and their inputs: tests/deform_cases.py; the
check's coefficient and the teeth: tests/test_deform_check.py (CPU).

The forward outputs are compared as the offsets the kernels compute; a residual output is stored
as fl(input + offset), so its element is given 2^-24 |output| beside coef A (the one rounding of
that sum, which is no product of the network and is not in A: a stated widening of the issue's
formula, of 6e-8 of the output's magnitude).  Parameter gradients accumulated
over two calls are compared at half their value.  A Gaussian with a ReLU input within 1e-4 of zero
has zero upstream in both runs (at most half of a case's Gaussians, checked on the oracle); a row
outside a tile case's window has zero upstream and must get exactly zero input gradients.

Measured max err / A on MI355X (recorded, not used for the bound; per group of tensors over all
cases of the group, from the DEFORM_ERR_OVER_A lines this module prints):
group             forward    inputs    planes   weights    biases      aabb   (tensor-wide rel)
S x P             5.8e-07   2.1e-08   2.5e-07   1.8e-05   6.8e-06   6.4e-06   6.6e-05
depths 1, 3, 4    5.0e-07   1.8e-08   1.8e-07   9.8e-06   4.6e-06   2.0e-06   3.7e-05
head masks        3.8e-07   5.9e-08   3.5e-07   1.1e-05   5.1e-06   3.0e-07   1.9e-05
apply_rotation    3.0e-07   6.4e-08   5.0e-07   1.3e-05   7.4e-06   1.8e-06   6.0e-05
golden variants   2.5e-07   1.8e-05   1.8e-06   9.9e-06   9.5e-06   2.9e-06   2.6e-04
time rows         3.4e-07   2.6e-08   1.1e-07   8.0e-06   4.2e-06   3.4e-08   1.7e-05
32 / 64           1.8e-08   5.9e-10   2.2e-08   3.7e-06   4.8e-08   5.1e-09   1.3e-05
tile regimes      6.2e-07   3.6e-08   1.4e-07   1.6e-05   7.5e-06   4.6e-06   3.6e-05
The bf16x3 emulation against the float64 oracle (CPU, tests/test_deform_check.py): at most 2.3e-5 A.
The last column is max |err| / max |ref| per tensor, printed and not asserted: on the discrete
variant's coff-head gradients it reaches 2.6e-4 where the emulation reaches 2.7e-4.
"""
import numpy as np
import pytest
import torch

import deform_cases as dc
from deformation import LANG_DISCRETE, LANG_NORESNET, LANG_PASS, LANG_RESIDUAL, DeformationField
from lsr_testutil import DEFORM_COEF, U24, deform_check

pytestmark = pytest.mark.gpu
KEYS = dc.KEYS
MODES = {"pass": LANG_PASS, "residual": LANG_RESIDUAL, "noresnet": LANG_NORESNET, "discrete": LANG_DISCRETE}


def _t(a):
    return None if a is None else torch.tensor(np.asarray(a, np.float32)).cuda()


def _field(name):
    x, c = dc.inputs(name), dc.CASES[name]
    cfg = x["cfg"]
    p = {k: _t(v) for k, v in x["params"].items()}
    p["grid.aabb"] = _t(x["aabb"])
    h = cfg.heads
    f = DeformationField(p, x["res"], x["multires"], depth=cfg.depth, no_dx=not h[0], no_ds=not h[1], no_dr=not h[2],
                         no_do=not h[3], no_dshs=not h[4], apply_rotation=cfg.apply_rotation,
                         lang_mode=MODES[cfg.lang_mode], lang_dim=cfg.lang_dim, centers=cfg.centers, time_pe=cfg.time_pe)
    assert (f.channels, f.width) == c["shape"]
    f.train_aabb = True
    return f


def _group(key):
    if key.startswith("grid.grids"):
        return "planes"
    return "aabb" if key == "grid.aabb" else ("biases" if key.endswith(".bias") else "weights")


def run_case(name, window=None):
    x, c = dc.inputs(name), dc.CASES[name]
    ref = dc.reference(name, window)
    rows, P = ref["rows"], c["P"]
    assert ref["amb"].mean() < dc.KINK_CAP if len(rows) >= 10 else not ref["amb"].all()
    f = _field(name)
    lang_on = x["cfg"].lang_mode != "pass"
    report = {}

    def check(native, want, A, what):
        bad, stats = deform_check(native, want, A, DEFORM_COEF)
        for k, st in stats.items():
            g = what if what != "param" else _group(k)
            report[g] = max(report.get(g, 0.0), st["max_err_over_A"])
            report["rel"] = max(report.get("rel", 0.0), st["rel"])          # tensor-wide, printed only
        assert not bad, (name, window, what, bad)

    # ---- forward (every row runs; the window's rows are compared) ----------------------------------
    out = f.forward(*[_t(x["inp"][k]) for k in KEYS], _t(x["lang"]) if lang_on else None, _t(x["times"][:, 0]))
    names = KEYS + (("lang", "coff") if lang_on else ())
    got = {k: o.cpu().numpy().astype(np.float64)[rows] for k, o in zip(names, out) if o is not None}
    want = dc.offsets(name, {k: ref["out"][k] for k in got}, rows)
    A = {}
    for k in got:
        A[k] = np.asarray(ref["A_out"][k], np.float64).reshape(want[k].shape)
        full = np.asarray(ref["out"][k], np.float64).reshape(want[k].shape)
        A[k] = A[k] + (A[k] > 0) * (U24 / DEFORM_COEF) * np.abs(full)       # the stored value's own rounding
    check(dc.offsets(name, got, rows), want, A, "forward")
    # ---- backward ----------------------------------------------------------------------------------
    ups = {k: np.zeros((P,) + v.shape[1:]) for k, v in ref["ups"].items()}
    for k, v in ref["ups"].items():
        ups[k][rows] = v
    f.zero_grad()
    for _ in range(c["calls"]):
        got = f.backward(_t(x["inp"]["means3D"]), _t(x["times"][:, 0]), *[_t(ups[k]) for k in KEYS],
                         rotations=_t(x["inp"]["rotations"]), lang=_t(x["lang"]) if lang_on else None,
                         d_lang=_t(ups.get("lang")) if lang_on else None, d_coff=_t(ups.get("coff")))
    torch.cuda.synchronize()
    g_in = {k: g.cpu().numpy().astype(np.float64) for k, g in zip(KEYS + ("lang",), got) if g is not None}
    outside = np.ones(P, bool)
    outside[rows] = False
    for k, g in g_in.items():
        assert not g[outside].any(), (name, window, k)                      # zero upstream: exactly nothing
    check({k: g[rows] for k, g in g_in.items()}, ref["g_in"], ref["A_in"], "inputs")
    grads = {k: v.cpu().numpy().astype(np.float64) / c["calls"] for k, v in f.grads.items()}
    assert set(grads) == set(ref["g"])
    check(grads, ref["g"], ref["A_g"], "param")
    print("\nDEFORM_ERR_OVER_A", name, window, " ".join(f"{k}={v:.2e}" for k, v in sorted(report.items())))


@pytest.mark.parametrize("name", dc.PLAIN_CASES)
def test_case_matches_oracle_per_element(name):
    """S = 1..4 at P = 1, 64, 65, 300; the depths 0, 1, 3, 4 (DEEP on and off); the launcher's runs
    (small heads only, the SH head only, one small head); apply_rotation; the golden variants lang,
    noresnet and discrete; the time rows; the 32 / 64 shape with points on lines and faces."""
    run_case(name)


@pytest.mark.parametrize("name,window", [(n, w) for n in dc.TILE_CASES for w in dc.windows(n)])
def test_tile_regime_matches_oracle_per_element(name, window):
    """k_head_wgrad3 at T = 2, 3, 4 (and 9, 17), k_head_wgrad2 at T = 3 (and 5), k_atb at 128 rows per
    block, each with the upstream nonzero only in every block's first tile, only in its last tile and
    only in the array's last row; up to P = 12,300 also with the full upstream (the middle tiles, which
    the prologue stages and the steady-state body handles)."""
    run_case(name, window)
