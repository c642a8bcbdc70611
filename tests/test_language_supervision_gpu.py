"""The fused 'lang' stage loss (lsr_seg_loss_views, language_supervision.segment_lang_loss) on the GPU.

References: tests/golden/langsup_golden.npz (the REFERENCE's get_language_feature, l1_loss and
cos_loss in float64, tests/golden/make_langsup_golden.py) and, for the shape sweep, the module's
torch fallback in float64 on the CPU (which tests/test_language_supervision.py holds to that fixture
at 1e-12).  Bounds: the loss 1e-5 relative against the fixture (tests/test_train_lang_gpu.py's); every
other figure 8 x the error the same float32 evaluation makes as torch ops on the CPU (the fixture's
recorded float32 reference error, or the float32 fallback's), the margin tests/test_query_gpu.py
uses for a re-ordered float32 evaluation.

The sweep's shapes are the smallest that reach each path (tests/langsup_cases.py SWEEP): the
smallest input, the scalar path under and over one wave, the largest V, an odd C, the 16-byte path
with more pixels than one 256-thread pass, and the headline row width with a table of 89.6 KB.  Each
carries unlabelled pixels and indices outside [-1, S); those of two rows or more a wholly unlabelled
row (the 1 x 1 input is one labelled pixel)."""
import os

import numpy as np
import pytest
import torch

import langsup_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "langsup_golden.npz")
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _sups(segs, tables, device):
    import language_supervision as ls
    return [ls.SegmentSupervision(torch.from_numpy(np.ascontiguousarray(segs[v])),
                                  torch.from_numpy(np.ascontiguousarray(tables[v]))).to(device)
            for v in range(len(segs))]


def _run(images, segs, tables, cos, device, dtype=torch.float32, lam=lc.LAM, beta=lc.BETA):
    """(loss, gradients [V, C, H, W]) of segment_lang_loss on `device` in `dtype`."""
    import language_supervision as ls
    xs = [torch.from_numpy(np.ascontiguousarray(x)).to(device=device, dtype=dtype).requires_grad_(True) for x in images]
    loss = ls.segment_lang_loss(xs, _sups(segs, tables, device), lam, beta, addcosloss=cos)
    loss.backward()
    return loss.detach(), torch.stack([x.grad for x in xs])


def _f64(t):
    return t.detach().cpu().double().numpy()


@pytest.fixture(scope="module")
def sweep_refs():
    """{(shape, cos): (inputs, float64 loss, float64 gradient, float32 loss error, float32 gradient error)},
    both by the torch fallback on the CPU, computed once."""
    out = {}
    for shape in lc.SWEEP:
        inp = lc.sweep_case(*shape)
        segs, tables, images = inp
        for cos in (False, True):
            l64, g64 = _run(images, segs, tables, cos, "cpu", torch.float64)
            l32, g32 = _run(images, segs, tables, cos, "cpu", torch.float32)
            out[shape, cos] = (inp, float(l64), _f64(g64), abs(float(l32) - float(l64)),
                               float(np.abs(_f64(g32) - _f64(g64)).max()))
    return out


@pytest.mark.parametrize("name", ("l1", "cos"))
@pytest.mark.parametrize("k", range(len(lc.FIXTURE_CASES)))
def test_fixture_parity(gold, k, name):
    import language_supervision as ls
    inp = lc.fixture_inputs(k)
    assert lc.checksum([inp["images"]]) == str(gold[f"c{k}_images_sha256"])
    segs = gold[f"c{k}_segs"][:, int(gold[f"c{k}_level"])]
    assert ls.native_eligible([torch.zeros(1, device=DEV)] * len(segs), _sups(segs, gold[f"c{k}_tables"], DEV))
    loss, grad = _run(inp["images"], segs, gold[f"c{k}_tables"], name == "cos", DEV)
    ref_loss, ref_grad = float(gold[f"c{k}_{name}_loss"]), gold[f"c{k}_{name}_grad"]
    e_loss = abs(float(loss) - ref_loss) / abs(ref_loss)
    e_grad = float(np.abs(_f64(grad) - ref_grad).max())
    bound = 8 * float(gold[f"c{k}_{name}_grad_f32_err"])
    print(f"case {k} {name}: loss rel error {e_loss:.3g}; gradient error {e_grad:.3g}, bound {bound:.3g}")
    assert e_loss <= 1e-5, (float(loss), ref_loss)
    assert e_grad <= bound, (e_grad, bound)
    unlabelled = torch.from_numpy(segs < 0)[:, None].expand(grad.shape)
    assert bool((grad.cpu()[unlabelled] == 0).all())


def _dense_l1_grad(images, segs, tables, lam):
    """Autograd's gradient of the dense expression TrainStep.loss runs, on the GPU."""
    xs = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_(True) for x in images]
    dense = [s.dense() for s in _sups(segs, tables, DEV)]
    gt, mask = torch.stack([g for g, _ in dense]), torch.stack([m for _, m in dense])
    lang = torch.stack(xs)
    loss = lam * (lang * mask - gt * mask).abs().mean()
    loss.backward()
    return loss.detach(), torch.stack([x.grad for x in xs])


@pytest.mark.parametrize("shape", [(2, 32, 19, 37, 11), (2, 32, 3, 300, 40), (1, 7, 3, 37, 5)])
def test_l1_gradient_equals_autograd_of_the_dense_expression_bit_for_bit(shape):
    segs, tables, images = lc.sweep_case(*shape, oob=False)
    for lam in (lc.LAM, 1.0, 0.37):
        _, want = _dense_l1_grad(images, segs, tables, lam)
        _, got = _run(images, segs, tables, False, DEV, lam=lam)
        assert torch.equal(got, want), (lam, float((got - want).abs().max()), float(want.abs().max()))


@pytest.mark.parametrize("cos", (False, True))
@pytest.mark.parametrize("shape", lc.SWEEP)
def test_shape_sweep_against_the_float64_fallback(sweep_refs, shape, cos):
    (segs, tables, images), l64, g64, e_l32, e_g32 = sweep_refs[shape, cos]
    loss, grad = _run(images, segs, tables, cos, DEV)
    e_loss, e_grad = abs(float(loss) - l64), float(np.abs(_f64(grad) - g64).max())
    print(f"{shape} cos={cos}: loss error {e_loss:.3g} (float32 fallback {e_l32:.3g}); "
          f"gradient error {e_grad:.3g} (float32 fallback {e_g32:.3g})")
    assert e_loss <= 8 * e_l32 and e_grad <= 8 * e_g32
    S = shape[4]
    unlabelled = torch.from_numpy((segs < 0) | (segs >= S))[:, None].expand(grad.shape)
    assert bool((grad.cpu()[unlabelled] == 0).all())


@pytest.mark.parametrize("cos", (False, True))
def test_a_wholly_unlabelled_view(cos):
    segs, tables, images = lc.sweep_case(1, 5, 4, 68, 3, all_unlabelled=True)
    loss, grad = _run(images, segs, tables, cos, DEV)
    want = torch.tensor(lc.BETA if cos else 0.0, dtype=torch.float32)
    assert loss.cpu() == want, (float(loss), float(want))
    assert bool((grad == 0).all())


CANARY = 7.25e11


def _carved(arr, pad, dtype, canary):
    """`arr` inside a larger device buffer filled with `canary`, `pad` elements from its start."""
    flat = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.full((flat.numel() + 2 * pad + 64,), canary, dtype=dtype, device=DEV)
    buf[pad:pad + flat.numel()] = flat.to(DEV)
    return buf, buf[pad:pad + flat.numel()]


def _intact(buf, pad, n, canary):
    outside = torch.cat([buf[:pad], buf[pad + n:]])
    return bool((outside == canary).all())


@pytest.mark.parametrize("pad", (1, 64))
@pytest.mark.parametrize("shape", [(2, 6, 3, 300, 40), (1, 3, 2, 1352, 700)])
def test_nothing_is_touched_outside_the_tensors(shape, pad):
    """Images, maps, tables, gradients and the workspace carved from canary-filled allocations, through
    the C ABI itself; pad 1 leaves them 4-byte aligned (the scalar path on a W % 4 == 0 image), pad 64
    16-byte aligned (the vector path).  The gradients start as NaN and come back finite."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    V, C, H, W, S = shape
    segs, tables, images = lc.sweep_case(*shape)
    nws = int(L.lsr_seg_loss_workspace_bytes(V, C, H, W))
    ws_buf = torch.full((nws + 512,), 0x5A, dtype=torch.uint8, device=DEV)
    loss_buf = torch.full((64,), CANARY, dtype=torch.float32, device=DEV)
    g_one = torch.ones(1, device=DEV)
    keep, views = [], (_lib.SegView * V)()
    for v in range(V):
        xb, x = _carved(images[v], pad, torch.float32, CANARY)
        sb, s = _carved(segs[v], pad, torch.int32, 0x7FFFFFF0)
        tb, t = _carved(tables[v], pad, torch.float32, CANARY)
        gb, g = _carved(np.full(images[v].shape, np.nan, np.float32), pad, torch.float32, CANARY)
        keep.append((xb, sb, tb, gb, g))
        views[v].image, views[v].d_image, views[v].seg, views[v].table = x.data_ptr(), g.data_ptr(), s.data_ptr(), \
            t.data_ptr()
        views[v].n_seg = S
        assert (x.data_ptr() % 16 == 0) == (pad == 64)
    st = torch.cuda.current_stream().cuda_stream
    ws = ws_buf[256:256 + nws]
    _lib.check(L.lsr_seg_loss_views(V, C, H, W, views, lc.LAM, lc.BETA, 1, loss_buf[32:].data_ptr(), ws.data_ptr(), st),
               "lsr_seg_loss_views")
    _lib.check(L.lsr_seg_loss_views_backward(V, C, H, W, views, lc.LAM, lc.BETA, 1, g_one.data_ptr(), ws.data_ptr(),
                                             st), "lsr_seg_loss_views_backward")
    torch.cuda.synchronize()
    n_img, n_seg, n_tab = C * H * W, H * W, S * C
    for xb, sb, tb, gb, g in keep:
        assert _intact(xb, pad, n_img, CANARY) and _intact(tb, pad, n_tab, CANARY) and _intact(gb, pad, n_img, CANARY)
        assert _intact(sb, pad, n_seg, 0x7FFFFFF0)
        assert bool(torch.isfinite(g).all())
    assert bool((ws_buf[:256] == 0x5A).all()) and bool((ws_buf[256 + nws:] == 0x5A).all())
    assert bool((loss_buf[:32] == CANARY).all()) and bool((loss_buf[33:] == CANARY).all())
    # and the values are the ones the autograd path computes from ordinary tensors
    loss, grad = _run(images, segs, tables, True, DEV)
    got = torch.stack([g.view(C, H, W) for *_, g in keep])
    if pad == 64:                                          # the same path: the same bits
        assert loss_buf[32] == loss and torch.equal(got, grad)
    else:      # the scalar path adds the rows' float32 sums in another order than the vector path
        assert abs(float(loss_buf[32]) - float(loss)) <= 1e-6 * abs(float(loss))
        assert float((got - grad).abs().max()) <= 1e-5 * float(grad.abs().max())


@pytest.mark.parametrize("cos", (False, True))
def test_two_calls_give_the_same_bits(cos):
    segs, tables, images = lc.sweep_case(2, 32, 3, 300, 40)
    a, b = _run(images, segs, tables, cos, DEV), _run(images, segs, tables, cos, DEV)
    assert a[0].view(torch.int32) == b[0].view(torch.int32)
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_peak_memory_is_the_gradients_and_the_workspace():
    import language_supervision as ls
    from diff_gaussian_rasterization import _lib
    V, C, H, W, S = 2, 32, 256, 256, 50
    gen = torch.Generator(device="cpu").manual_seed(3)
    xs = [torch.randn(C, H, W, generator=gen).to(DEV).requires_grad_(True) for _ in range(V)]
    segs = torch.randint(-1, S, (V, H, W), generator=gen, dtype=torch.int32)
    sups = [ls.SegmentSupervision(segs[v], torch.randn(S, C, generator=gen)).to(DEV) for v in range(V)]
    dense = [s.dense() for s in sups]
    gt, mask = torch.stack([g for g, _ in dense]), torch.stack([m for _, m in dense])

    def peak(fn):
        for x in xs:
            x.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def dense_loss():
        lang = torch.stack(xs)
        a, b = lang * mask, gt * mask
        return lc.LAM * (a - b).abs().mean() + lc.BETA * (1 - torch.nn.functional.cosine_similarity(a, b, dim=-1).mean())

    fused = peak(lambda: ls.segment_lang_loss(xs, sups, lc.LAM, lc.BETA, addcosloss=True))
    torch_dense = peak(dense_loss)
    allowed = V * C * H * W * 4 + int(_lib.load().lsr_seg_loss_workspace_bytes(V, C, H, W)) + (1 << 20)
    assert fused <= allowed, (f"fused peak {fused} bytes over forward + backward, allowed {allowed}; "
                              f"the dense torch expression needs {torch_dense} on the same inputs")
    print(f"peak over forward + backward: fused {fused} bytes (allowed {allowed}), dense torch {torch_dense}")


@pytest.mark.parametrize("cos", (False, True))
def test_float64_and_nine_views_take_the_fallback(monkeypatch, cos):
    import language_supervision as ls
    shape = (1, 7, 3, 37, 5)
    segs, tables, images = lc.sweep_case(*shape)
    native_loss, native_grad = _run(images, segs, tables, cos, DEV)
    l64c, g64c = _run(images, segs, tables, cos, "cpu", torch.float64)
    l32c, g32c = _run(images, segs, tables, cos, "cpu", torch.float32)
    e_l32, e_g32 = abs(float(l32c) - float(l64c)), float(np.abs(_f64(g32c) - _f64(g64c)).max())

    def no_native(*a, **k):
        raise AssertionError("the native path was taken")
    monkeypatch.setattr(ls._SegLoss, "apply", no_native)
    # float64 on the GPU
    l64, g64 = _run(images, segs, tables, cos, DEV, torch.float64)
    assert l64.dtype == torch.float64 and l64.is_cuda
    assert abs(float(native_loss) - float(l64)) <= 8 * e_l32
    assert float(np.abs(_f64(native_grad) - _f64(g64)).max()) <= 8 * e_g32
    # nine views (the one view nine times), float32: the fallback again, held to its own CPU run's error
    nine = [np.repeat(a, 9, 0) for a in (images, segs, tables)]
    l64n, g64n = _run(nine[0], nine[1], nine[2], cos, "cpu", torch.float64)
    l32n, g32n = _run(nine[0], nine[1], nine[2], cos, "cpu", torch.float32)
    l9, g9 = _run(nine[0], nine[1], nine[2], cos, DEV)
    assert l9.dtype == torch.float32 and g9.shape[0] == 9 and g9.is_cuda
    assert abs(float(l9) - float(l64n)) <= 8 * abs(float(l32n) - float(l64n))
    assert float(np.abs(_f64(g9) - _f64(g64n)).max()) <= 8 * float(np.abs(_f64(g32n) - _f64(g64n)).max())
    # supervision on another device falls back too, never reaching the library with a host pointer
    xs = [torch.from_numpy(images[0].copy()).to(DEV)]
    assert not ls.native_eligible(xs, _sups(segs, tables, "cpu"))
    moved = ls.segment_lang_loss(xs, _sups(segs, tables, "cpu"), lc.LAM, lc.BETA, addcosloss=cos)
    assert moved.is_cuda and abs(float(moved) - float(l64c)) <= 8 * e_l32


def test_train_step_with_segment_supervision_equals_the_dense_form():
    """One 'lang' stage iteration on the scene of tests/golden/lang_train_golden.npz, supervised by a
    seeded SegmentSupervision and again, on a fresh copy, by its dense() form: the rendered language
    images identical, the losses within 1e-5, every gradient within 1e-4 |dense| + 1e-5 max |dense|
    (the bound for gradients that differ only by float-atomic order)."""
    import language_supervision as ls
    from test_train_lang_gpu import _load, _setup
    d = _load("cos_joint")
    runs = []
    for form in ("segments", "dense"):
        step, tr, field, cam, gt_img, gt_lang, _ = _setup(d)
        C, H, W = gt_lang.shape[-3:]
        sup = ls.SegmentSupervision(torch.from_numpy(lc.seg_map(H, W, 9, 401)),
                                    torch.from_numpy(lc.table(9, C, 402))).to(DEV)
        if form == "segments":
            loss, outs = step.forward_backward([cam], gt_img, lang_sup=[sup])
        else:
            gt, mask = sup.dense()
            loss, outs = step.forward_backward([cam], gt_img, gt_lang=gt[None], lang_mask=mask[None])
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in tr.params.items() if p.grad is not None}
        grads.update({"field/" + k: v.detach().clone() for k, v in field.grads.items()})
        runs.append((float(loss.detach()), outs[0]["language_feature_image"].detach().clone(), grads))
    (l_seg, img_seg, g_seg), (l_dense, img_dense, g_dense) = runs
    assert abs(l_seg - l_dense) <= 1e-5 * abs(l_dense), (l_seg, l_dense)
    assert torch.equal(img_seg, img_dense)
    assert set(g_seg) == set(g_dense) and "language_feature" in g_seg
    for k, want in g_dense.items():
        tol = 1e-4 * want.abs() + 1e-5 * want.abs().max()
        over = ((g_seg[k] - want).abs() - tol).max()
        assert float(over) <= 0, (k, float(over), float(want.abs().max()))
