"""CPU checks of the HexPlane regularisers (plane_regularizer.py, include/lsr_plane_reg.h).

Reference: tests/golden/plane_reg.npz, the REFERENCE's compute_plane_smoothness and the sums of its
compute_regulation in float64 on a seeded field (tools/make_plane_reg_golden.py).  The float64 numpy
restatement of tests/plane_reg_cases.py and the module's torch formulation (the path every input but float32
CUDA planes takes) run the same float64 operations and must reproduce the file to 1e-12 relative; the GPU tests
then hold the kernel against the restatement.  The C ABI's refusals are checked here too: they are decided
before anything touches a device.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import plane_reg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plane_reg.npz")
RTOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    d = {k: z[k] for k in z.files}
    S = len(pc.GOLDEN_MULTIRES)
    d["planes"] = [[d[f"plane/{s}/{ci}"] for ci in range(6)] for s in range(S)]
    d["grads"] = [[d[f"grad/{s}/{ci}"] for ci in range(6)] for s in range(S)]
    return d


def _close(got, want, rtol=RTOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want)
    assert np.all(err <= rtol * np.abs(want)), float((err / np.maximum(np.abs(want), 1e-300)).max())


def test_golden_file_is_the_documented_field(golden):
    assert tuple(golden["weights"]) == pc.GOLDEN_WEIGHTS
    shapes = pc.plane_shapes(pc.GOLDEN_RES, pc.GOLDEN_MULTIRES)
    for s in range(2):
        for ci in range(6):
            p = golden["planes"][s][ci]
            assert p.dtype == np.float32 and p.shape == shapes[s][ci]
            assert golden["grads"][s][ci].dtype == np.float64 and golden["grads"][s][ci].shape == p.shape
            if ci in pc.TIME:                                  # the kink of |1 - t| is well populated
                assert 0.3 < float((p == 1).mean()) < 0.7
    assert golden["terms"].shape == (12, 2) and float(golden["total"]) > 0


def test_restatement_reproduces_the_reference(golden):
    total, terms, grads = pc.field_np(golden["planes"], pc.GOLDEN_WEIGHTS)
    _close(total, golden["total"])
    _close(terms, golden["terms"])
    for s in range(2):
        for ci in range(6):
            _close(grads[s][ci], golden["grads"][s][ci])


@pytest.mark.parametrize("accumulate", (False, True))
def test_torch_fallback_reproduces_the_reference(golden, accumulate):
    """float64 CPU planes take the torch formulation; overwrite, and accumulate onto a seeded gradient."""
    import plane_regularizer as pr
    planes = [[torch.tensor(p, dtype=torch.float64) for p in scale] for scale in golden["planes"]]
    g = torch.Generator().manual_seed(5)
    prev = [[torch.randn(p.shape, generator=g, dtype=torch.float64) * 1e-3 for p in scale] for scale in planes]
    grads = [[x.clone() for x in scale] for scale in prev]
    res = pr.regularize_planes(planes, pc.GOLDEN_WEIGHTS, grads, accumulate=accumulate)
    assert res.total.dtype == torch.float64 and res.terms.shape == (12, 2)
    _close(res.total.numpy(), golden["total"])
    _close(res.terms.numpy(), golden["terms"])
    _close(res.plane_smooth.numpy(), golden["plane_smooth"])
    _close(res.time_smooth.numpy(), golden["time_smooth"])
    _close(res.time_l1.numpy(), golden["time_l1"])
    total, plane_smooth, time_smooth, time_l1, terms = res     # unpacks in the documented order
    assert total is res.total and terms is res.terms
    for s in range(2):
        for ci in range(6):
            want = golden["grads"][s][ci]
            if accumulate:
                got = (grads[s][ci] - prev[s][ci]).numpy()
                err = np.abs(got - want)
                # the subtraction's own rounding: an ulp of the seeded gradient
                assert np.all(err <= RTOL * np.abs(want) + 2.0 ** -52 * np.abs(prev[s][ci].numpy()))
            else:
                _close(grads[s][ci].numpy(), want)
    # the loss alone: the same numbers, no gradient asked for
    alone = pr.regularize_planes(planes, pc.GOLDEN_WEIGHTS)
    assert torch.equal(alone.total, res.total) and torch.equal(alone.terms, res.terms)


def test_compute_regulation_autograd_is_the_closed_form(golden):
    import plane_regularizer as pr
    planes = [[torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in scale] for scale in golden["planes"]]
    tsw, l1w, tvw = pc.GOLDEN_WEIGHTS
    total = pr.compute_regulation(planes, tsw, l1w, tvw)
    assert total.dim() == 0 and total.grad_fn is not None
    _close(total.item(), golden["total"])
    (3.0 * total).backward()
    for s in range(2):
        for ci in range(6):
            _close(planes[s][ci].grad.numpy(), 3.0 * golden["grads"][s][ci])
    # float32 CPU planes: the same formulas in float32
    p32 = [[torch.nn.Parameter(torch.tensor(p)) for p in scale] for scale in golden["planes"]]
    t32 = pr.compute_regulation(p32, tsw, l1w, tvw)
    assert t32.dtype == torch.float32 and abs(t32.item() - float(golden["total"])) <= 1e-5 * float(golden["total"])
    t32.backward()
    g, want = p32[1][2].grad.numpy(), golden["grads"][1][2]
    assert g.dtype == np.float32 and np.abs(g - want).max() <= 1e-4 * np.abs(want).max()


def test_compute_regulation_takes_a_field_like_object(golden):
    import plane_regularizer as pr

    class Field:
        multires = pc.GOLDEN_MULTIRES
        p = {f"grid.grids.{s}.{ci}": torch.tensor(golden["planes"][s][ci], dtype=torch.float64)
             for s in range(2) for ci in range(6)}
    tsw, l1w, tvw = pc.GOLDEN_WEIGHTS
    _close(pr.compute_regulation(Field(), tsw, l1w, tvw).item(), golden["total"])


def test_l1_gradient_at_and_around_one():
    """An L1-only plane holding 1.0, its two neighbours, 0.0, -0.0 and negative values: exactly
    -sign(1 - t) / N, an exact 0 at 1.0."""
    import plane_regularizer as pr
    one = np.float32(1)
    vals = np.array([1.0, np.nextafter(one, np.float32(np.inf)), np.nextafter(one, np.float32(-np.inf)), 0.0, -0.0,
                     -1.0, -3.5, 2.0, 1.0, 1.0, 0.999, 1.001], np.float32)
    N = vals.size
    want = np.array([0, 1, -1, -1, -1, -1, -1, 1, 0, 0, -1, 1], np.float64) / N
    for dtype in (torch.float32, torch.float64):
        t = torch.tensor(vals.reshape(1, 2, 3, 2), dtype=dtype)
        planes = [[t] * 6]                                     # six views of one plane: only ci 2 is read back
        grads = [[torch.full_like(t, 7.0) for _ in range(6)]]
        res = pr.regularize_planes(planes, (0.0, 1.0, 0.0), grads, accumulate=False)
        got = grads[0][2].reshape(-1).numpy()
        assert np.array_equal(got, want.astype(got.dtype))     # 1 / 12 scaled by +-1 or 0: exact in either dtype
        assert np.all(got[[0, 8, 9]] == 0)
        assert np.array_equal(grads[0][0].numpy(), np.zeros_like(t.numpy()))   # a spatial plane: no L1 term
        # N roundings of the dtype at most (float32: each |1 - t|, each add and the division)
        _close(res.terms[2, 1].item(), np.abs(1 - vals.astype(np.float64)).sum() / N,
               2 * N * (2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53))
    g = pc.l1_np(vals.reshape(1, 2, 3, 2))[1].reshape(-1)
    assert np.array_equal(g, want)


def test_short_planes_and_bad_arguments_are_refused():
    import plane_regularizer as pr
    t = torch.ones(1, 2, 2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="H >= 3"):
        pr.regularize_planes([[t] * 6], (1e-3, 1e-4, 2e-4))
    with pytest.raises(ValueError, match="H >= 3"):            # only the time planes' smoothness is off
        pr.regularize_planes([[t] * 6], (0.0, 1e-4, 2e-4))
    res = pr.regularize_planes([[t] * 6], (0.0, 1e-4, 0.0))    # the L1 term alone needs no second difference
    assert float(res.total) == 0.0 and float(res.terms[:, 0].abs().max()) == 0.0
    with pytest.raises(ValueError, match="six planes"):
        pr.regularize_planes([[t] * 5], (0.0, 1e-4, 0.0))
    with pytest.raises(ValueError, match=r"\[1, C, H, W\]"):
        pr.regularize_planes([[t[0]] * 6], (0.0, 1e-4, 0.0))
    with pytest.raises(ValueError, match="gradient 0 must match"):
        pr.regularize_planes([[t] * 6], (0.0, 1e-4, 0.0), [[t.float()] * 6])
    assert float(pr.regularize_planes([], (1.0, 1.0, 1.0)).total) == 0.0


def test_plane_reg_from_hidden():
    import plane_regularizer as pr
    assert pr.plane_reg_from_hidden({}) == (0.01, 0.0001, 0.0001)          # arguments/__init__.py:93-95
    neu3d = dict(time_smoothness_weight=0.001, l1_time_planes=0.0001, plane_tv_weight=0.0002)
    assert pr.plane_reg_from_hidden(neu3d) == (0.001, 0.0001, 0.0002)      # arguments/neu3d/default.py:11-13

    class Hidden:
        def __init__(self):
            self.time_smoothness_weight, self.plane_tv_weight = 0.5, 0.25
    assert pr.plane_reg_from_hidden(Hidden()) == (0.5, 0.0001, 0.25)
    assert pr.plane_reg_from_hidden(dict(neu3d, time_smoothness_weight=0)) is None   # train.py:331's gate
    assert pr.plane_reg_from_hidden(dict(neu3d, l1_time_planes=0, plane_tv_weight=0)) == (0.001, 0.0, 0.0)


def test_train_step_refuses_plane_reg_without_a_field():
    import types
    from train_step import TrainStep
    trainer = types.SimpleNamespace(params={}, device="cpu")   # the constructor only looks (a real one needs a GPU)
    with pytest.raises(ValueError, match="a field is required"):
        TrainStep(trainer, None, stage="coarse-base", bg=torch.ones(3), plane_reg=(1e-3, 1e-4, 2e-4))
    step = TrainStep(trainer, None, stage="coarse-base", bg=torch.ones(3))
    assert step.plane_reg is None and step.plane_reg_terms is None and not step.plane_reg_active


# ---- the C ABI's argument checks -------------------------------------------------------------------------------
def _descs(*planes):
    from diff_gaussian_rasterization import _lib
    arr = (_lib.PlaneDesc * max(len(planes), 1))()
    for d, kw in zip(arr, planes):
        for k, v in dict(dict(t=64, grad=64, C=16, H=8, W=8, w_smooth=1e-3, w_l1=1e-4), **kw).items():
            setattr(d, k, v)
    return arr


def test_plane_desc_matches_the_header(tmp_path):
    """The ctypes mirror of lsr_plane_desc has the C compiler's field offsets and size, and the constants agree."""
    import subprocess
    from diff_gaussian_rasterization import _lib
    names = [f[0] for f in _lib.PlaneDesc._fields_]
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{os.path.join(ROOT, "include", "lsr_plane_reg.h")}"',
             "int main(void) {", 'printf("size %zu\\n", sizeof(lsr_plane_desc));']
    lines += [f'printf("{n} %zu\\n", offsetof(lsr_plane_desc, {n}));' for n in names]
    lines += ['printf("version %d\\n", LSR_PLANE_REG_API_VERSION);', 'printf("max %d\\n", LSR_PLANE_REG_MAX_PLANES);',
              'printf("block %d\\n", LSR_PLANE_REG_BLOCK_ELEMS);', "return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.splitlines())
    want = {n: str(getattr(_lib.PlaneDesc, n).offset) for n in names}
    want.update(size=str(ctypes.sizeof(_lib.PlaneDesc)), version=str(_lib.PLANE_REG_API_VERSION),
                max=str(_lib.PLANE_REG_MAX_PLANES), block=str(_lib.PLANE_REG_BLOCK_ELEMS))
    assert got == want


def test_abi_argument_checks():
    """Every refusal of include/lsr_plane_reg.h, with pointers that are never dereferenced: each call below fails
    before anything touches a device.  n_planes = 0 is valid (its size query answers; the call itself launches the
    finishing kernel, which the GPU tests run)."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    err = lambda: lib.lsr_last_error().decode()                # noqa: E731
    p = ctypes.c_void_p(64)
    EINVAL = 1

    def refused(planes, n, text, ws=p, outs=(p, p, p)):
        assert lib.lsr_plane_reg(n, planes, 0, ws, *outs, None) == EINVAL and text in err(), err()

    def both_refuse(planes, n, text):
        refused(planes, n, text)
        assert lib.lsr_plane_reg_workspace_bytes(n, planes) == -1 and text in err(), err()

    ok = _descs({}, {})
    B = _lib.PLANE_REG_BLOCK_ELEMS
    assert lib.lsr_plane_reg_workspace_bytes(2, ok) == 2 * (16 * 8 * 8 // B) * 16
    assert lib.lsr_plane_reg_workspace_bytes(0, None) == 16 and lib.lsr_plane_reg_workspace_bytes(0, ok) == 16
    odd = _descs(dict(C=3, H=9, W=257), dict(C=1, H=3, W=1))   # 6939 elements: a last block in part, and 1 block
    assert lib.lsr_plane_reg_workspace_bytes(2, odd) == (-(-6939 // B) + 1) * 16
    both_refuse(ok, -1, "n_planes must be in [0, 24]")
    both_refuse(_descs(*([{}] * 25)), 25, "n_planes must be in [0, 24]")
    assert lib.lsr_plane_reg_workspace_bytes(24, _descs(*([{}] * 24))) == 24 * (16 * 8 * 8 // B) * 16
    both_refuse(None, 2, "descriptors are required")
    refused(_descs({}, dict(t=None)), 2, "plane 1 is null")
    assert lib.lsr_plane_reg_workspace_bytes(2, _descs({}, dict(t=None))) > 0      # the query reads shapes only
    for bad in (dict(C=0), dict(H=0), dict(W=-1)):
        both_refuse(_descs({}, bad), 2, "plane 1: C, H and W must be >= 1")
    both_refuse(_descs(dict(H=2)), 1, "H >= 3 where w_smooth != 0")
    both_refuse(_descs(dict(H=1, w_l1=0.0)), 1, "H >= 3 where w_smooth != 0")
    assert lib.lsr_plane_reg_workspace_bytes(1, _descs(dict(H=2, w_smooth=0.0))) == 16    # L1 only: no stencil
    both_refuse(_descs(dict(C=2048, H=2048, W=2048)), 1, "must fit an int32 element index")
    both_refuse(_descs(dict(C=1 << 16, H=1 << 15, W=1)), 1, "must fit an int32 element index")   # 2^31 exactly
    both_refuse(_descs(dict(C=0x7fffffff, H=0x7fffffff, W=0x7fffffff)), 1, "must fit an int32 element index")
    assert lib.lsr_plane_reg_workspace_bytes(1, _descs(dict(C=0x7fffffff, H=1, W=1, w_smooth=0.0))) == -(-0x7fffffff // B) * 16
    refused(ok, 2, "workspace, terms, total and total64 are required", ws=None)
    for k in range(3):
        outs = [p, p, p]
        outs[k] = None
        refused(ok, 2, "workspace, terms, total and total64 are required", outs=tuple(outs))
    refused(ok, 2, "8-byte aligned", ws=ctypes.c_void_p(68))
    refused(ok, 0, "workspace, terms, total and total64 are required", ws=None)   # n_planes = 0 passes the plane checks
