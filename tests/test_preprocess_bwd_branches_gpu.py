"""The launcher branches of the preprocess backward (preprocess.hip, k_preprocess_bwd_views) through
backward_native, i.e. its one-view instantiations, against the oracle.

One kernel source serves one view (lsr_backward: atomic sums or, deterministic, the compositor's
records summed in instance order) and up to eight (lsr_backward_views).  Its launcher picks the
instantiation by the SH coefficient count M -- rows staged in LDS for M = 1, 4, 9, 16, the generic
kernel otherwise -- and by accumulate; colors_precomp and cov3D_precomp switch the SH chain and the
scale / rotation backward off.  The scenes (bwd_cases.PP_CASES) are the ragged 83 x 61 base scene
on 700 Gaussians: three 256-row blocks, the last one partial, the first with 40 culled rows beside
visible ones (tests/test_backward_check.py asserts it on the oracle).

    case   inputs                                   kernel
    M1     SH, 1 coefficient, degree 0              staged rows, MS = 1
    M4     SH, 4 coefficients, degree 1             staged rows, MS = 4
    M9     SH, 9 coefficients, degree 2             staged rows, MS = 9
    M16    SH, 16 coefficients, degree 3            staged rows, MS = 16
    M25    SH, 25 coefficients, degree 3            generic, MS = 0 (rows 16..24: zero gradient)
    COL    colors_precomp, scales and rotations     generic, no SH chain
    COV    SH 16, cov3D_precomp                     staged rows, no scale / rotation backward
    CLAMP  SH 16; 46 visible rows outside the       staged rows, MS = 16; cov2d_bwd zeroes the clamped
           1.3 tan(fov) clamp, 19 faint rows        Jacobian column (39 such rows with a means3D
           with a radius and no tiles               gradient, up to 117); unlisted rows: zero gradient

Asserted per case: the atomic and the deterministic backward pass lsr_testutil.grad_check against
the float oracle at its tolerances (per element 1e-4 |ref| + 1e-4 A for language, opacity and
means2D; grad_err <= 1e-4 for every field), and the deterministic one repeats bit for bit.  For M16
and COL, deterministic, accumulate=True into buffers prefilled with a fixed nonzero pattern gives
prefill + the accumulate=False result bit for bit in every row, and the rows of culled Gaussians
(radii 0) keep the prefill bit for bit.

Measured on an MI355X, maxima over the 8 cases (recorded, not used to set any bound): deterministic
err / A language 3.7e-07 and opacity 2.2e-07 (both CLAMP), means2D 2.2e-07, grad_err <= 3.7e-06 in
every field (language, COL); atomic err / A language 1.7e-05, opacity 4.7e-06, means2D 4.6e-06,
grad_err <= 2.7e-05 (scales).  CLAMP alone: atomic grad_err means3D 2.0e-06, deterministic 4.1e-07,
with means3D gradients of up to 117 on its frustum-clamped rows.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # CPU container: the driver only runs these on the MI355X box
    pytest.skip("needs a GPU", allow_module_level=True)

import diff_gaussian_rasterization as dgr  # noqa: E402
import bwd_cases  # noqa: E402
from lsr_testutil import grad_check, oracle_keyed, run_native  # noqa: E402


def _dev(x):
    return None if x is None else torch.tensor(x, device="cuda")


def _expected_fields(c):
    f = {"means3D", "means2D", "colors", "opacity", "lang"}
    f |= {"cov3D"} if c.cov3D else {"scales", "rotations"}
    return f | (set() if c.colors is not None else {"sh"})


def _setup(name):
    c, ref = bwd_cases.case(name), bwd_cases.reference(name)
    bwd_cases.check_preprocess_preconditions(name, ref)
    nat = run_native(c.scene, c.cams[0], **c.run_kw())
    np.testing.assert_array_equal(nat[2].cpu().numpy(), ref.views[0].radii)
    return c, ref, nat, (_dev(c.gcol[0]), _dev(c.glang[0]), _dev(c.gdep[0]))


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("name", list(bwd_cases.PP_CASES) + ["CLAMP"])
def test_one_view_branch(name, deterministic):
    c, ref, nat, ups = _setup(name)
    g = dgr.backward_native(nat[4], *ups, deterministic=deterministic)
    if deterministic:
        again = dgr.backward_native(nat[4], *ups, deterministic=True)
        for k, v in g.items():
            assert (v is None) == (again[k] is None) and (v is None or torch.equal(v, again[k])), (name, k)
    go = oracle_keyed(g)
    assert set(go) == _expected_fields(c), (name, sorted(go))
    bad, stats = grad_check(go, ref.grads, ref.abs)
    print(name, "deterministic" if deterministic else "atomic",
          {k: {n: float(f"{x:.2e}") for n, x in s.items()} for k, s in stats.items()})
    assert not bad, (name, bad, stats)
    if name == "M25":   # the coefficients past degree 3 are never read: exactly zero gradient
        assert not g["sh"][:, 16:].any()


@pytest.mark.parametrize("name", ["M16", "COL"])
def test_accumulate_adds_to_prefill(name):
    c, ref, nat, ups = _setup(name)
    g = dgr.backward_native(nat[4], *ups, deterministic=True)
    pre = {k: ((torch.arange(v.numel(), device="cuda", dtype=torch.float32) % 7.0) * 0.375 - 1.25).reshape(v.shape)
           for k, v in g.items() if v is not None}       # never 0: -1.25 .. 1.0 in steps of 0.375
    out = dgr.backward_native(nat[4], *ups, out={k: v.clone() for k, v in pre.items()}, accumulate=True,
                              deterministic=True)
    culled = nat[2] == 0
    assert 40 <= int(culled.sum()) < c.scene.P // 2
    for k, v in g.items():
        assert (v is None) == (out[k] is None), (name, k)
        if v is None:
            continue
        assert torch.equal(out[k], pre[k] + v), (name, k)
        assert torch.equal(out[k][culled], pre[k][culled]), (name, k)
