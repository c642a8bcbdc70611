"""The fused image loss (lsr_image_loss_views / _backward, image_loss.py, TrainStep(lambda_dssim=...)) on the GPU.

Reference: tests/golden/image_loss_golden.npz (the REFERENCE's l1_loss, ssim and psnr in float64,
tests/golden/make_image_loss_golden.py) on the cases of tests/image_loss_cases.py, the smallest shapes at
which the stencil can go wrong.  Bounds: the L1 and the SSIM (over all views and per view) 1e-5 absolute, the
language-supervision tests' loss bound; PSNR 1e-4 dB; the SSIM gradient 8 x the error the reference's own
float32 run makes (recorded per case in the fixture), the project's margin for a re-ordered float32
evaluation; the L1 gradient equal to lsr_l1_loss_views_backward's bit for bit.

Every run through the C ABI here is guarded: the images, gradients, stats, totals and the workspace are carved
from canary-filled allocations that must come back intact, and the gradients start as NaN and must come back
finite.  The TrainStep tests compare whole iterations; where the deformation field is in the graph, two runs
of the same code differ by the order of its float atomics, and the gradients are held to
1e-4 |want| + 1e-5 max |want| (tests/test_language_supervision_gpu.py's bound for that); what is reproducible
(the loss, the gradient towards the renders, a whole iteration without the field in the rasterizer's
fixed-order mode) is compared bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import image_loss_cases as ic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda"
NAMES = list(ic.CASES)
CANARY = 7.25e11


@pytest.fixture(scope="module")
def gold():
    out = {}
    for f in ["image_loss_golden.npz"] + sorted(set(ic.GRAD_FILE_OF.values())):
        z = np.load(os.path.join(GOLDEN, f))
        out.update({k: z[k] for k in z.files})
    return out


@pytest.fixture(scope="module")
def cases(gold):
    out = {}
    for name in NAMES:
        x, gt_full = ic.inputs(name)
        assert ic.checksum([x, gt_full]) == str(gold[name + "_inputs_sha256"]), name
        out[name] = (x, gt_full)
    return out


def _carved(arr, pad, canary=CANARY):
    """`arr` (float32) inside a larger device buffer filled with `canary`, `pad` floats from its start."""
    flat = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).reshape(-1)
    buf = torch.full((flat.numel() + 2 * pad + 64,), canary, dtype=torch.float32, device=DEV)
    buf[pad:pad + flat.numel()] = flat.to(DEV)
    return buf, buf[pad:pad + flat.numel()]


def _intact(buf, pad, n, canary=CANARY):
    return bool((torch.cat([buf[:pad], buf[pad + n:]]) == canary).all())


class Abi:
    """One case through the C ABI with every buffer guarded.  pad: floats in front of each image and gradient
    (64: 16-byte aligned; 1: 4-byte aligned only)."""

    def __init__(self, x, gt_full, pad=64):
        from diff_gaussian_rasterization import _lib
        self.lib, self.L = _lib, _lib.load()
        self.V, self.C, self.H, self.W = x.shape
        self.n, self.pad = self.C * self.H * self.W, pad
        self.x = [_carved(x[v], pad) for v in range(self.V)]
        self.g = [_carved(np.full(x[v].shape, np.nan, np.float32), pad) for v in range(self.V)]
        self.gt_buf, gt = _carved(gt_full, pad)                  # views gt_full.shape[1] H W floats apart
        self.gt, self.stride = gt, gt_full.shape[1] * self.H * self.W
        self.nws = int(self.L.lsr_image_loss_workspace_bytes(self.V, self.C, self.H, self.W))
        assert self.nws > 0
        self.ws_buf = torch.full((self.nws + 512,), 0x5A, dtype=torch.uint8, device=DEV)
        self.ws = self.ws_buf[256:256 + self.nws]
        self.out_buf = torch.full((128,), CANARY, dtype=torch.float32, device=DEV)
        self.stats, self.totals = self.out_buf[32:32 + 3 * self.V], self.out_buf[96:98]
        for _, t in self.x + self.g:
            assert (t.data_ptr() % 16 == 0) == (pad % 4 == 0)
        self.st = torch.cuda.current_stream().cuda_stream

    def _ptrs(self, pairs):
        return (ctypes.c_void_p * self.V)(*[t.data_ptr() for _, t in pairs])

    def forward(self):
        self.lib.check(self.L.lsr_image_loss_views(self.V, self.C, self.H, self.W, self._ptrs(self.x), self.gt.data_ptr(),
                                                   self.stride, self.stats.data_ptr(), self.totals.data_ptr(),
                                                   self.ws.data_ptr(), self.st), "lsr_image_loss_views")
        torch.cuda.synchronize()
        return self.stats.view(self.V, 3).clone(), self.totals.clone()

    def backward(self, d_l1, d_ssim):
        """The gradients [V, C, H, W] for upstream gradients given as floats, device tensors or None (NULL)."""
        keep = [torch.tensor([d], dtype=torch.float32, device=DEV) if isinstance(d, float) else d for d in (d_l1, d_ssim)]
        for _, g in self.g:
            g.fill_(float("nan"))
        self.lib.check(self.L.lsr_image_loss_views_backward(
            self.V, self.C, self.H, self.W, self._ptrs(self.x), self.gt.data_ptr(), self.stride,
            *[None if d is None else d.data_ptr() for d in keep], self._ptrs(self.g), self.ws.data_ptr(), self.st),
            "lsr_image_loss_views_backward")
        torch.cuda.synchronize()
        out = torch.stack([g.view(self.C, self.H, self.W) for _, g in self.g]).clone()
        assert bool(torch.isfinite(out).all()), "an element of d_images was not written"
        return out

    def l1_backward(self, d_l1):
        """lsr_l1_loss_views_backward on the same inputs (unguarded buffers of its own)."""
        grads = [torch.full((self.n,), float("nan"), device=DEV) for _ in range(self.V)]
        d = torch.tensor([d_l1], dtype=torch.float32, device=DEV)
        self.lib.check(self.L.lsr_l1_loss_views_backward(
            self.V, self.n, self._ptrs(self.x), self.gt.data_ptr(), self.stride, d.data_ptr(),
            (ctypes.c_void_p * self.V)(*[g.data_ptr() for g in grads]), self.st), "lsr_l1_loss_views_backward")
        torch.cuda.synchronize()
        return torch.stack(grads).view(self.V, self.C, self.H, self.W)

    def assert_guards_intact(self):
        for buf, _ in self.x + self.g:
            assert _intact(buf, self.pad, self.n)
        assert _intact(self.gt_buf, self.pad, self.gt.numel())
        assert bool((self.ws_buf[:256] == 0x5A).all()) and bool((self.ws_buf[256 + self.nws:] == 0x5A).all())
        o = self.out_buf
        outside = torch.cat([o[:32], o[32 + 3 * self.V:96], o[98:]])
        assert bool((outside == CANARY).all())


def _f64(t):
    return t.detach().cpu().double().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_fixture_parity_through_the_abi(gold, cases, name):
    x, gt_full = cases[name]
    run = Abi(x, gt_full)
    stats, totals = run.forward()
    stats, totals = _f64(stats), _f64(totals)
    psnr = 20 * np.log10(1.0 / np.sqrt(stats[:, 2]))
    e = dict(l1=abs(totals[0] - float(gold[name + "_l1"])), ssim=abs(totals[1] - float(gold[name + "_ssim"])),
             ssim_view=np.abs(stats[:, 1] - gold[name + "_ssim_view"]).max(),
             psnr=np.abs(psnr - gold[name + "_psnr_view"][:, 0].astype(np.float64)).max())
    # the per-view L1 has no entry of its own in the fixture: its mean over the views is the L1
    e["l1_views"] = abs(stats[:, 0].mean() - float(gold[name + "_l1"]))
    g_ssim = run.backward(None, 1.0)
    e_grad = float(np.abs(_f64(g_ssim) - gold[name + "_ssim_grad"]).max())
    bound = 8 * float(gold[name + "_ssim_grad_f32_err"])
    print(f"{name}: errors {({k: float(f'{v:.3g}') for k, v in e.items()})}; ssim gradient error {e_grad:.3g}, "
          f"bound {bound:.3g} (max |gradient| {float(np.abs(gold[name + '_ssim_grad']).max()):.3g})")
    assert e["l1"] <= 1e-5 and e["ssim"] <= 1e-5 and e["ssim_view"] <= 1e-5 and e["l1_views"] <= 1e-5, e
    assert e["psnr"] <= 1e-4, e
    assert e_grad <= bound, (e_grad, bound)
    # both upstream gradients at once: the sum of the two parts
    both = run.backward(0.7, -0.3)
    want = 0.7 * gold[name + "_l1_grad"] - 0.3 * gold[name + "_ssim_grad"]
    assert float(np.abs(_f64(both) - want).max()) <= 0.3 * bound + 1e-7 * float(np.abs(want).max())
    run.assert_guards_intact()


@pytest.mark.parametrize("name", NAMES)
def test_l1_gradient_is_the_l1_kernels_bit_for_bit(cases, name):
    """With d_ssim NULL, and again with a device 0 behind it, for a unit and an odd upstream gradient."""
    run = Abi(*cases[name])
    run.forward()
    zero = torch.zeros(1, device=DEV)
    for d in (1.0, 0.37):
        want = run.l1_backward(d)
        assert bool(torch.isfinite(want).all())
        assert torch.equal(run.backward(d, None), want)
        assert torch.equal(run.backward(d, zero), want)
    assert bool((run.backward(None, None) == 0).all())
    run.assert_guards_intact()


@pytest.mark.parametrize("name", ("b", "c", "e2"))
def test_two_runs_give_the_same_bits(cases, name):
    res = []
    for _ in range(2):
        run = Abi(*cases[name])
        stats, totals = run.forward()
        res.append((stats, totals, run.backward(1.0, 1.0), run.backward(None, 0.2)))
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", ("a", "b", "e1"))
def test_images_four_bytes_off_alignment_give_the_same_values(cases, name):
    aligned, off = Abi(*cases[name], pad=64), Abi(*cases[name], pad=1)
    sa, ta = aligned.forward()
    so, to = off.forward()
    assert torch.equal(sa, so) and torch.equal(ta, to)
    assert torch.equal(aligned.backward(0.5, 1.0), off.backward(0.5, 1.0))
    off.assert_guards_intact()


def _module_run(x, gt, device, dtype=torch.float32, lam=0.2):
    """(loss, l1, ssim, gradients [V, C, H, W]) of image_loss_views on `device` in `dtype`."""
    import image_loss as il
    xs = [torch.from_numpy(x[v].copy()).to(device=device, dtype=dtype).requires_grad_(True) for v in range(len(x))]
    loss, l1, ss = il.image_loss_views(xs, gt, lam)
    loss.backward()
    return loss.detach(), l1.detach(), ss.detach(), torch.stack([t.grad for t in xs])


@pytest.mark.parametrize("name", ("b", "e2"))
def test_module_takes_the_native_path_and_matches_the_fixture(gold, cases, name):
    """image_loss_views / ssim / psnr on CUDA float32 tensors; case b's ground truth is the [:, :3] view of a
    [V, 4, H, W] tensor, which the native path reads in place."""
    import image_loss as il
    x, gt_full = cases[name]
    gts = torch.from_numpy(gt_full).to(DEV)
    xs = [torch.from_numpy(x[v].copy()).to(DEV) for v in range(len(x))]
    assert il.native_eligible(xs, gts[:, :3])
    loss, l1, ss, grad = _module_run(x, gts, DEV)
    assert abs(float(l1) - float(gold[name + "_l1"])) <= 1e-5 and abs(float(ss) - float(gold[name + "_ssim"])) <= 1e-5
    want = gold[name + "_l1_grad"] - 0.2 * gold[name + "_ssim_grad"]
    bound = 0.2 * 8 * float(gold[name + "_ssim_grad_f32_err"]) + 1e-7 * float(np.abs(want).max())
    assert float(np.abs(_f64(grad) - want).max()) <= bound
    stacked = torch.stack(xs)
    per_view = il.ssim(stacked, gts[:, :3], size_average=False)
    assert per_view.shape == (len(x),) and float(np.abs(_f64(per_view) - gold[name + "_ssim_view"]).max()) <= 1e-5
    assert abs(float(il.ssim(xs[0], gts[0, :3])) - float(gold[name + "_ssim_view"][0])) <= 1e-5
    p = il.psnr(stacked, gts[:, :3])
    assert p.shape == (len(x), 1) and p.dtype == torch.float32
    assert float(np.abs(_f64(p) - gold[name + "_psnr_view"].astype(np.float64)).max()) <= 1e-4


def test_nine_views_float64_and_a_host_ground_truth_take_the_torch_path(monkeypatch, gold, cases):
    import image_loss as il
    x, gt_full = cases["b"]
    gt = torch.from_numpy(gt_full)[:, :3]
    native = _module_run(x, torch.from_numpy(gt_full).to(DEV), DEV)

    def no_native(*a, **k):
        raise AssertionError("the native path was taken")
    monkeypatch.setattr(il._ImageLossViews, "apply", no_native)
    bound = 0.2 * 8 * float(gold["b_ssim_grad_f32_err"]) + 2e-7 * float(np.abs(gold["b_l1_grad"]).max())
    # float64 on the GPU
    l64 = _module_run(x, gt.to(DEV).double(), DEV, torch.float64)
    assert l64[0].dtype == torch.float64 and l64[0].is_cuda
    assert abs(float(l64[1]) - float(gold["b_l1"])) <= 1e-12 and abs(float(l64[2]) - float(gold["b_ssim"])) <= 1e-12
    assert abs(float(native[0]) - float(l64[0])) <= 1e-5
    assert float(np.abs(_f64(native[3]) - _f64(l64[3])).max()) <= bound
    # a ground truth on the host: moved by the torch path, no host pointer reaches a kernel
    xs = [torch.from_numpy(x[v].copy()).to(DEV) for v in range(2)]
    assert not il.native_eligible(xs, gt)
    moved = _module_run(x, torch.from_numpy(gt_full), DEV)
    assert moved[0].is_cuda and abs(float(moved[0]) - float(l64[0])) <= 1e-5
    assert float(np.abs(_f64(moved[3]) - _f64(l64[3])).max()) <= bound
    # nine views (the first view nine times), float32
    x9 = np.repeat(x[:1], 9, 0)
    gt9 = gt[:1].repeat(9, 1, 1, 1).to(DEV)
    assert not il.native_eligible([torch.from_numpy(x9[v]).to(DEV) for v in range(9)], gt9)
    nine = _module_run(x9, gt9, DEV)
    assert nine[3].shape[0] == 9 and nine[0].dtype == torch.float32
    assert abs(float(nine[2]) - float(gold["b_ssim_view"][0])) <= 1e-5
    # another window size, a ground truth that wants a gradient, a non-contiguous image
    assert not il.native_eligible(xs, gt.to(DEV), window_size=7)
    assert not il.native_eligible(xs, gt.to(DEV).requires_grad_(True))
    assert not il.native_eligible([t.transpose(1, 2).contiguous().transpose(1, 2) for t in xs], gt.to(DEV))
    assert il.ssim(torch.stack(xs), gt.to(DEV), window_size=7).is_cuda


# ---- TrainStep ---------------------------------------------------------------------------------------------------
AABB = [[7.0, 5.5, 10.5], [-7.0, -5.5, 1.5]]
RES, MULTIRES = [16, 16, 16, 10], [1, 2]
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-2, "f_rest": 2.5e-2 / 20, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}


def _base_step(with_field=True, **kw):
    """A fresh TrainStep on the synthetic scene of tests/test_train_step_gpu.py (4000 Gaussians, two 160 x 120
    views), with seeded ground truth [V, 4, H, W]."""
    import synthetic
    from deformation import DeformationField
    from gaussian_train import GaussianTrainer
    from train_step import TrainStep
    P, W, H = 4000, 160, 120
    dev = torch.device(DEV)
    sc = synthetic.make_scene(P, C=3, tanfovx=0.6, tanfovy=0.6 * H / W, seed=3, logscale_mean=-3.0).to(dev)
    cams = synthetic.camera_batch(2, W, H, tanfovx=0.6, seed=2)
    raw = {"xyz": sc.means3D.contiguous(), "f_dc": sc.shs[:, :1].contiguous(), "f_rest": sc.shs[:, 1:].contiguous(),
           "opacity": torch.logit(sc.opacities.reshape(P, 1)).contiguous(), "scaling": torch.log(sc.scales).contiguous(),
           "rotation": sc.rotations.contiguous()}
    field = None
    if with_field:
        field_p = DeformationField.init_params(RES, MULTIRES, AABB, seed=1)
        field = DeformationField({k: v.to(dev) for k, v in field_p.items()}, RES, MULTIRES)
    gts = torch.rand(2, 4, H, W, generator=torch.Generator().manual_seed(11)).to(dev)
    step = TrainStep(GaussianTrainer(raw, LRS), field, stage="fine-base" if with_field else "coarse-base", **kw)
    return step, cams, gts


def _grads(step):
    torch.cuda.synchronize()
    out = {k: p.grad.detach().clone() for k, p in step.trainer.params.items() if p.grad is not None}
    if step.field is not None:
        out.update({"field/" + k: v.detach().clone() for k, v in step.field.grads.items()})
    return out


def _assert_close_up_to_atomic_order(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        tol = 1e-4 * w.abs() + 1e-5 * w.abs().max()
        over = ((got[k] - w).abs() - tol).max()
        assert float(over) <= 0, (k, float(over), float(w.abs().max()))


def test_train_step_with_dssim_equals_the_torch_assembly(monkeypatch):
    """'fine-base' at lambda_dssim 0.2: the fused loss against the same step with the loss assembled from the
    module's torch formulation."""
    import image_loss as il
    step, cams, gts = _base_step(lambda_dssim=0.2)
    calls = []
    real = il._ImageLossViews.apply
    monkeypatch.setattr(il._ImageLossViews, "apply", lambda *a: calls.append(1) or real(*a))
    loss, _ = step.forward_backward(cams, gts)
    got = _grads(step)
    assert calls == [1]                                       # one fused forward (and its one backward)
    monkeypatch.setattr(il, "native_eligible", lambda *a, **k: False)
    ref_step, cams, gts = _base_step(lambda_dssim=0.2)
    want_loss, _ = ref_step.forward_backward(cams, gts)
    want = _grads(ref_step)
    assert calls == [1]
    loss, want_loss = float(loss.detach()), float(want_loss.detach())
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
    assert "xyz" in want and "field/grid.grids.1.3" in want
    _assert_close_up_to_atomic_order(got, want)
    # and the term is in the loss: without it the value is another
    plain, cams, gts = _base_step()
    l_plain, _ = plain.forward_backward(cams, gts)
    assert loss > float(l_plain.detach()) * (1 + 1e-3)


def test_train_step_with_lambda_zero_is_the_default_step():
    """lambda_dssim=0 against a TrainStep built without the argument.  On one set of renders the losses and the
    gradients towards the renders are identical; a whole iteration without the deformation field, in the
    rasterizer's fixed-order mode, gives identical gradients in every parameter; with the field (whose backward
    adds with float atomics: two runs of one step differ) every gradient agrees up to that order."""
    from gaussian_scene import render_views
    zero, cams, gts = _base_step(lambda_dssim=0.0)
    default, _, _ = _base_step()
    with torch.no_grad():
        outs = render_views(cams, zero.scene(), zero.bg, stage="fine-base")
    renders = [o["render"].detach().clone().requires_grad_(True) for o in outs]
    res = []
    for step in (zero, default):
        loss = step.loss([{"render": r} for r in renders], gts)
        res.append((loss.detach(), torch.autograd.grad(loss, renders)))
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))

    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        runs = []
        for kw in (dict(lambda_dssim=0.0), {}):
            step, cams, gts = _base_step(with_field=False, **kw)
            loss, _ = step.forward_backward(cams, gts)
            runs.append((loss.detach(), _grads(step)))
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(runs[0][0], runs[1][0])
    assert set(runs[0][1]) == set(runs[1][1]) and "xyz" in runs[0][1]
    for k, want in runs[1][1].items():
        assert torch.equal(runs[0][1][k], want), k

    l_zero, _ = zero.forward_backward(cams, gts)
    l_default, _ = default.forward_backward(cams, gts)
    assert torch.equal(l_zero.detach(), l_default.detach())
    _assert_close_up_to_atomic_order(_grads(zero), _grads(default))


def test_joint_lang_stage_with_dssim(monkeypatch):
    """'fine-lang' with joint_train at lambda_dssim 0.2 on the scene of tests/golden/lang_train_golden.npz: the
    gradients reach the geometry and the loss is the torch assembly's."""
    import image_loss as il
    from test_train_lang_gpu import _load, _setup
    d = _load("cos_joint")

    def run(lambda_dssim):
        step, tr, field, cam, gt_img, gt_lang, mask = _setup(d)
        assert step.joint_train
        step.lambda_dssim = lambda_dssim
        loss, outs = step.forward_backward([cam], gt_img, gt_lang=gt_lang, lang_mask=mask)
        return float(loss.detach()), _grads(step), outs[0]["render"].detach(), gt_img

    loss, grads, image, gt_img = run(0.2)
    for k in ("xyz", "scaling", "rotation", "opacity", "f_dc"):
        assert k in grads and bool(torch.isfinite(grads[k]).all()) and float(grads[k].abs().max()) > 0, k
    l_plain, g_plain, _, _ = run(0.0)
    with torch.no_grad():
        ss = float(il.ssim_map(image[None].double(), gt_img[:, :3].double()).mean())
    assert abs(loss - (l_plain + 0.2 * (1 - ss))) <= 1e-5 * abs(loss), (loss, l_plain, ss)
    assert not torch.allclose(grads["xyz"], g_plain["xyz"], rtol=1e-3, atol=0)      # the term reaches the geometry
    monkeypatch.setattr(il, "native_eligible", lambda *a, **k: False)
    l_torch, g_torch, _, _ = run(0.2)
    assert abs(loss - l_torch) <= 1e-5 * abs(l_torch)
    _assert_close_up_to_atomic_order(grads, g_torch)
