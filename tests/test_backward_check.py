"""The per-element gradient check (lsr_testutil.grad_check) and the scenes of
tests/test_backward_branches_gpu.py (bwd_cases), on the oracle alone.

(a) the float oracle passes grad_check against the double oracle on every scene, with the same
    radii and n_contrib: the bound is one the reference meets without any kernel.  Largest
    |f32 - f64| / A over the 13 scenes: language 6.6e-5, means2D 5.5e-5, opacity 3.5e-5 (bound:
    1e-4 A + 1e-4 |ref|); largest grad_err of any field 1.2e-5 (bound: 1e-4).  The float oracle
    rounds the projection (centres, conics) as well as the sums, which A does not measure, so these
    are upper limits for a kernel that shares the float oracle's projection bit for bit.
(b) every scene's preconditions hold (bwd_cases.check_preconditions): clamped colour channels,
    capped alphas, a quadrant wholly outside the image, long replays.
    The preprocess-backward scenes (bwd_cases.PP_CASES, tests/test_preprocess_bwd_branches_gpu.py)
    hold theirs (check_preprocess_preconditions): P mod 256 != 0, culled and visible rows in one
    256-row block, clamped SH colours; the oracle takes every one of them, M = 25 included.
    CLAMP (bwd_cases.PP_EXTRA) also holds its own: at least 20 visible rows outside the
    1.3 tan(fov) clamp, 20 of them with a means3D gradient, 16 visible rows of opacity <= 0.003
    (its float-against-double margin: tests/test_preprocess_fwd_check.py).
(c) the check has teeth: gradients doctored on the contributing Gaussians with the smallest terms
    -- language rows zeroed, one language channel zeroed, opacity sign flipped; as many Gaussians,
    in ascending order of A, as the tensor-wide measure lets through, at least 1 in 100 -- pass
    grad_err <= 1e-4 and fail grad_check.
"""
import numpy as np
import pytest

import bwd_cases
from lsr_testutil import GRAD_TOL, grad_check, grad_err


@pytest.mark.parametrize("name", list(bwd_cases.CASES))
def test_f32_oracle_passes_against_f64(name):
    r32, r64 = bwd_cases.reference(name, False), bwd_cases.reference(name, True)
    for a, b in zip(r32.views, r64.views):
        np.testing.assert_array_equal(a.radii, b.radii)
        np.testing.assert_array_equal(a.state()["n_contrib"], b.state()["n_contrib"])
    bad, stats = grad_check(r32.grads, r64.grads, r64.abs)
    print(name, stats)
    assert not bad, (bad, stats)
    assert set(stats) >= {"means3D", "means2D", "opacity", "colors"}


@pytest.mark.parametrize("name", list(bwd_cases.CASES))
def test_scene_preconditions(name):
    print(name, bwd_cases.check_preconditions(name, bwd_cases.reference(name)))


@pytest.mark.parametrize("name", list(bwd_cases.PP_CASES) + ["CLAMP"])
def test_preprocess_scene_preconditions(name):
    print(name, bwd_cases.check_preprocess_preconditions(name, bwd_cases.reference(name)))


def _smallest_terms(A, change, fmax):
    """The contributing Gaussians (A > 0 in every column) in ascending order of A, cut where the
    doctoring (`change`: each row's largest |doctored - true|) would first exceed GRAD_TOL of the
    tensor's largest magnitude: all that grad_err cannot see.  (A full tenth of them is too many in
    this scene: zeroing their language rows gives grad_err 3.6e-4.)"""
    rows = np.nonzero((A > 0).all(axis=1))[0]
    rows = rows[np.argsort(A[rows].max(axis=1))]
    n = int((np.maximum.accumulate(change[rows]) <= 0.9 * GRAD_TOL * fmax).sum())
    assert len(rows) >= 1000 and n >= len(rows) // 100, (len(rows), n)
    return rows[:n]


@pytest.mark.parametrize("doctor", ["lang_rows", "lang_last_channel", "opacity_sign"])
def test_grad_check_rejects_what_grad_err_accepts(doctor):
    ref = bwd_cases.reference("B")
    C = bwd_cases.case("B").C
    field = "opacity" if doctor == "opacity_sign" else "lang"
    g = {k: v.copy() for k, v in ref.grads.items()}
    assert not grad_check(g, ref.grads, ref.abs)[0]           # undoctored: passes
    true = np.abs(ref.grads[field])
    change = (2 * true[:, 0] if doctor == "opacity_sign" else
              true[:, C - 1] if doctor == "lang_last_channel" else true.max(axis=1))
    rows = _smallest_terms(ref.abs[field], change, true.max())
    if doctor == "lang_rows":
        g["lang"][rows] = 0.0
    elif doctor == "lang_last_channel":
        g["lang"][rows, C - 1] = 0.0
    else:
        g["opacity"][rows] *= -1.0
    assert true[rows].min() > 0                                # something was there to lose
    assert grad_err(g[field], ref.grads[field]) <= GRAD_TOL    # the tensor-wide measure accepts it
    bad, stats = grad_check(g, ref.grads, ref.abs)
    assert set(bad) == {field} and "grad_err" not in bad[field], (bad, stats)
    # every doctored element is caught, bar those whose terms cancel to under 1e-4 of their size
    expect = len(rows) * (C if doctor == "lang_rows" else 1)
    assert bad[field]["elements"] >= 0.95 * expect, (bad[field]["elements"], expect)
