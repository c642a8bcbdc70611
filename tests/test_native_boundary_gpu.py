"""The training glue's native paths take only what passes _lib.Boundary: anything else runs the torch expression (the
public functions that have one) or raises ValueError before the library is touched (GaussianTrainer).  In every test
the library is unreachable, so a wrapper that wrongly proceeds fails the test without launching anything."""
import pytest
import torch

import gaussian_scene
import train_step
from diff_gaussian_rasterization import _lib
from gaussian_train import GaussianTrainer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _reached():
    raise AssertionError("reached the library")


class _NoLibrary:
    def __getattr__(self, name):
        _reached()


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", _reached)


def _rand(*shape, dtype=torch.float32, seed=0, device=DEV):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype).to(device)


def _outcome(fn):
    """fn's result, or the type of what it raises"""
    try:
        return fn()
    except Exception as e:   # noqa: BLE001
        return type(e)


# ---- l1_loss_views ------------------------------------------------------------------------------
def _images(requires_grad=False):
    return [_rand(3, 5, 7, seed=v).requires_grad_(requires_grad) for v in range(2)]


def test_l1_float64_gts_runs_torch():
    images, gts = _images(), _rand(2, 4, 5, 7, dtype=torch.float64, seed=5)
    want = (torch.stack(images) - gts[:, :3]).abs().mean()
    got = train_step.l1_loss_views(images, gts)
    assert got.dtype == want.dtype == torch.float64 and torch.equal(got, want)


def test_l1_gts_gradient_is_kept():
    images = _images(True)
    gts = _rand(2, 4, 5, 7, seed=5).requires_grad_(True)
    ref = gts.detach().clone().requires_grad_(True)
    (torch.stack([x.detach() for x in images]) - ref[:, :3]).abs().mean().backward()
    train_step.l1_loss_views(images, gts).backward()
    assert gts.grad is not None and torch.equal(gts.grad, ref.grad)
    assert all(x.grad is not None for x in images)


def test_l1_host_gts_is_torchs_error():
    with pytest.raises(RuntimeError, match="same device"):
        train_step.l1_loss_views(_images(), _rand(2, 4, 5, 7, seed=5, device="cpu"))


def test_l1_eligible_inputs_still_go_native():
    with pytest.raises(AssertionError, match="reached the library"):
        train_step.l1_loss_views(_images(), _rand(2, 4, 5, 7, seed=5))


def test_l1_forward_confirms_before_any_address():
    with pytest.raises(ValueError, match="l1 loss"):
        train_step._L1Views.apply(_rand(2, 4, 5, 7, dtype=torch.float64, seed=5)[:, :3], *_images())


# ---- activate -----------------------------------------------------------------------------------
def _torch_activate(s, r, o):
    return torch.exp(s), torch.nn.functional.normalize(r), torch.sigmoid(o)


def test_activate_float64_rotations_runs_torch():
    s, r, o = _rand(9, 3, seed=1), _rand(9, 4, dtype=torch.float64, seed=2), _rand(9, 1, seed=3)
    got, want = gaussian_scene.activate(s, r, o), _torch_activate(s, r, o)
    assert [g.dtype for g in got] == [torch.float32, torch.float64, torch.float32]
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_activate_host_opacity_does_what_torch_does():
    """The three torch ops are independent, so torch itself raises nothing here: the opacity comes back a host
    tensor.  Whatever torch does with these inputs, activate() does the same and does not reach the library."""
    s, r, o = _rand(9, 3, seed=1), _rand(9, 4, seed=2), _rand(9, 1, seed=3, device="cpu")
    want = _outcome(lambda: _torch_activate(s, r, o))
    got = _outcome(lambda: gaussian_scene.activate(s, r, o))
    if isinstance(want, type):
        assert got is want
    else:
        assert [g.device for g in got] == [w.device for w in want] and all(torch.equal(g, w) for g, w in zip(got, want))


def test_activate_backward_refuses_a_foreign_gradient():
    class Ctx:
        saved_tensors = (_rand(9, 3, seed=1), _rand(9, 4, seed=2), _rand(9, 1, seed=3))
        needs_input_grad = (True, True, True)
    good = [torch.ones_like(t) for t in Ctx.saved_tensors]
    for k, bad in ((0, good[0].double()), (1, good[1].cpu()), (2, good[2].to(torch.uint8))):
        gs = list(good)
        gs[k] = bad
        with pytest.raises(ValueError, match="^grad .*: contiguous float32 tensor on cuda:0 required"):
            gaussian_scene._Activate.backward(Ctx, *gs)


def test_activate_backward_keeps_contiguous_copies_of_expanded_gradients(monkeypatch):
    """sum() of each output delivers expanded (stride 0) gradients: the backward makes contiguous copies, which
    must outlive the launch (an address alone keeps nothing alive).  Run with the library, against torch."""
    monkeypatch.undo()
    N = 100003
    g = torch.Generator().manual_seed(3)
    raw = [(torch.randn(N, k, generator=g) * m).to(DEV) for k, m in ((3, 2.0), (4, 1.0), (1, 3.0))]
    a = [t.clone().requires_grad_(True) for t in raw]
    b = [t.clone().requires_grad_(True) for t in raw]
    s, r, o = gaussian_scene.activate(*a)
    (s.sum() * 2 + r.sum() * 3 + o.sum() * 5).backward()
    s, r, o = _torch_activate(*b)
    (s.sum() * 2 + r.sum() * 3 + o.sum() * 5).backward()
    # every element is a handful of float32 operations (the rotations' a 4-term dot product and a division) on terms
    # no larger than the tensor's largest gradient: 1e-5 of that is about 80 ulp of the largest term, where a
    # gradient read from a reused block is wrong by the gradient's own size
    for x, y in zip(a, b):
        assert x.grad is not None and float((x.grad - y.grad).abs().max()) <= 1e-5 * float(y.grad.abs().max())


def test_activate_eligible_inputs_still_go_native():
    with pytest.raises(AssertionError, match="reached the library"):
        gaussian_scene.activate(_rand(9, 3, seed=1), _rand(9, 4, seed=2), _rand(9, 1, seed=3))


# ---- repeat_views / split_views -------------------------------------------------------------------
def test_repeat_and_split_with_a_float64_tensor_run_torch():
    xs = [_rand(6, 3, seed=1), _rand(6, 4, dtype=torch.float64, seed=2), _rand(6, 2, 3, seed=3)]
    got = gaussian_scene.repeat_views(2, *xs)
    for g, x in zip(got, xs):
        assert g.dtype == x.dtype and torch.equal(g, x.repeat(2, *([1] * (x.dim() - 1))))
    got = gaussian_scene.split_views(2, xs[0], None, xs[1], xs[2])
    assert got[1] == (None, None)
    for g, x in zip([got[0]] + got[2:], xs):
        assert len(g) == 2 and all(torch.equal(a, b) for a, b in zip(g, x.split(3)))


def test_repeat_and_split_backward_refuse_a_foreign_gradient():
    class Ctx:
        V, P, shapes, device = 2, 3, [(3, 4)], DEV
        needs_input_grad = (False, True)
    for bad in (torch.ones(6, 4, dtype=torch.float64, device=DEV), torch.ones(6, 4)):
        with pytest.raises(ValueError, match="contiguous float32 tensor on cuda:0 required"):
            gaussian_scene._RepeatViews.backward(Ctx, bad)
    Ctx.shapes = [(6, 4)]
    good = torch.ones(3, 4, device=DEV)
    for bad in (good.double(), good.cpu()):
        with pytest.raises(ValueError, match="contiguous float32 tensor on"):
            gaussian_scene._SplitViews.backward(Ctx, good, bad)


# ---- GaussianTrainer ----------------------------------------------------------------------------
def _trainer(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: None)
    tr = GaussianTrainer({"xyz": _rand(5, 3, seed=1), "opacity": _rand(5, 1, seed=2)}, {"xyz": 1e-3, "opacity": 1e-2})
    tr._L = _NoLibrary()
    monkeypatch.setattr(_lib, "load", _reached)
    return tr


def test_densification_stats_refuse_a_host_gradient(monkeypatch):
    tr = _trainer(monkeypatch)
    radii = torch.ones(5, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="viewspace_point_grad: float32 tensor on cuda:0 required, got float32 on cpu"):
        tr.add_densification_stats(torch.ones(5, 3), radii)
    with pytest.raises(ValueError):
        tr.add_densification_stats(torch.ones(5, 3, dtype=torch.float64, device=DEV), radii)


def test_densification_stats_never_pass_host_radii(monkeypatch):
    """Host radii are moved to the trainer's device: every address is confirmed by the boundary before the
    library's entry point is looked up, so reaching the library means only device tensors went in."""
    tr = _trainer(monkeypatch)
    grad = torch.ones(5, 3, device=DEV)
    for radii in (torch.ones(5, dtype=torch.int32), torch.ones(5, dtype=torch.int64), torch.ones(5, device=DEV)):
        try:
            tr.add_densification_stats(grad, radii)
        except ValueError:
            continue
        except AssertionError as e:
            assert "reached the library" in str(e)
        else:
            raise AssertionError("add_densification_stats returned without the library")
