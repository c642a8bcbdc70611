"""The status centres on the GPU (include/lsr_centers.h, language_centers.py): the per-row k-means
against the numpy restatement (tests/centers_cases.py) on separated data, exactly determined degenerate
rows, invariants on unseparated data, bit reproducibility, the fused field path against the two-step
path and against DeformationField.forward, the refusals, and the hand-over into the
'fine-lang-discrete' TrainStep."""
import math

import numpy as np
import pytest
import torch

import centers_cases as cc

pytestmark = pytest.mark.gpu

AABB = [[1.5, 1.5, 1.5], [-1.5, -1.5, -1.5]]
RES, MULTIRES = [8, 8, 8, 6], [1, 2, 4]                     # HyperNeRF structure (3 scales), small planes
HYPER_HEADS = ("pos_deform", "scales_deform", "rotations_deform")


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


def _field(mode, lang_dim, seed=1, centers=0, edit=None):
    from deformation import DeformationField
    p = DeformationField.init_params(RES, MULTIRES, AABB, seed=seed, depth=1, heads=HYPER_HEADS, lang_mode=mode,
                                     lang_dim=lang_dim, centers=centers)
    if edit:
        edit(p)
    return DeformationField({k: v.cuda() for k, v in p.items()}, RES, MULTIRES, depth=1, no_do=True, no_dshs=True,
                            lang_mode=mode, lang_dim=lang_dim, centers=centers)


def _gaussians(P, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return dict(means3D=(torch.rand(P, 3, generator=g) * 2 - 1).cuda(), scales=r(P, 3).cuda(), rotations=r(P, 4).cuda(),
                opacity=r(P, 1).cuda(), shs=r(P, 16, 3).cuda(), lang=(r(P, D) * 1.7).cuda())


# ---- 1. k-means against the restatement on separated data -----------------------------------------
@pytest.mark.parametrize("shape", cc.SEPARATED, ids=str)
def test_kmeans_matches_restatement_on_separated_data(shape):
    from language_centers import kmeans_rows
    P, S, D, K = shape
    x, sizes = cc.separated_case(P, S, D, K)
    ref_c, ref_n, ref_inertia, ref_it, _ = cc.separated_ref(P, S, D, K)
    c, n, inertia, it = _np(*kmeans_rows(torch.tensor(x).cuda(), K))
    assert c.shape == (P, K, D) and n.shape == (P, K) and inertia.shape == (P,) and it.shape == (P,)
    # each centre against its nearest restated centre
    near = ((c[:, :, None, :].astype(np.float64) - ref_c[:, None, :, :]) ** 2).sum(axis=3).argmin(axis=2)   # [P, K]
    assert all(sorted(row) == list(range(K)) for row in near)
    matched_c = np.take_along_axis(ref_c, near[:, :, None], axis=1)
    matched_n = np.take_along_axis(ref_n, near, axis=1)
    assert np.array_equal(n, matched_n)
    assert np.abs(c - matched_c).max() <= 2e-5
    assert (np.abs(inertia - ref_inertia) <= 1e-4 * np.abs(ref_inertia) + 1e-6).all()
    assert np.array_equal(near, np.tile(np.arange(K), (P, 1)))          # and in the seeding order
    assert np.array_equal(it, ref_it)


# ---- 2. exactly determined degenerate rows -----------------------------------------------------------
def test_degenerate_rows_are_exact():
    from language_centers import kmeans_rows
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(6, 1, 5, generator=g)
    x0 = x0 / x0.norm(dim=-1, keepdim=True)
    S, K = 100, 3
    c, n, inertia, it = kmeans_rows(x0.repeat(1, S, 1).cuda(), K)
    assert torch.equal(c.cpu(), x0.repeat(1, K, 1))                       # bit for bit
    assert torch.equal(n.cpu(), torch.tensor([[S, 0, 0]] * 6, dtype=torch.int32))
    assert torch.equal(inertia.cpu(), torch.zeros(6)) and torch.equal(it.cpu(), torch.ones(6, dtype=torch.int32))
    # S == K with distinct samples
    x = torch.randn(9, 8, 16, generator=g)
    c, n, inertia, it = kmeans_rows(x.cuda(), 8)
    for p in range(9):
        assert sorted(map(tuple, c[p].cpu().tolist())) == sorted(map(tuple, x[p].tolist()))
    assert (n == 1).all() and (inertia == 0).all() and (it == 1).all()


# ---- 3. invariants on unseparated data -------------------------------------------------------------------
@pytest.mark.parametrize("shape", cc.UNSEPARATED, ids=str)
def test_invariants_on_unseparated_data(shape):
    from language_centers import kmeans_rows
    P, S, D, K = shape
    max_iter = 100
    x = cc.unseparated_case(P, S, D)
    xd = torch.tensor(x).cuda()
    c, n, inertia, it = _np(*kmeans_rows(xd, K, max_iter=max_iter))
    assert (n.sum(axis=1) == S).all() and (n >= 0).all()
    assert (it >= 1).all() and (it <= max_iter).all()
    gap, a64 = cc.margins(x, c)
    low = gap < cc.LOW_MARGIN
    print("low-margin share", low.mean(), "iters max", it.max())
    assert low.mean() <= cc.LOW_MARGIN_SHARE
    clear = ~low.any(axis=1)
    cnt64 = np.stack([((a64 == j) & ~low).sum(axis=1) for j in range(K)], axis=1)
    assert (cnt64 <= n).all() and ((n - cnt64).sum(axis=1) == low.sum(axis=1)).all()
    assert np.array_equal(cnt64[clear], n[clear])
    x64 = x.astype(np.float64)
    checked = 0
    for p in np.nonzero(clear & (it < max_iter))[0]:
        for j in range(K):
            if n[p, j]:
                assert np.abs(c[p, j] - x64[p][a64[p] == j].mean(axis=0)).max() <= 2e-5, (p, j)
                checked += 1
    assert checked > P                                                   # the check saw converged rows
    want = np.take_along_axis(((x64[:, :, None, :] - c[:, None].astype(np.float64)) ** 2).sum(axis=3),
                              a64[:, :, None], axis=2).sum(axis=(1, 2))
    assert (np.abs(inertia - want) <= 1e-4 * want).all()
    it1 = kmeans_rows(xd, K, max_iter=1)[3]
    assert (it1 == 1).all()


# ---- 4. two calls give the same bits --------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    from deformation import LANG_RESIDUAL
    from language_centers import kmeans_rows, sample_centers
    P, S, D, K = 67, 100, 6, 3
    x = torch.tensor(cc.separated_case(P, S, D, K)[0]).cuda()
    a, b = kmeans_rows(x, K), kmeans_rows(x, K)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    field = _field(LANG_RESIDUAL, D)
    lang = _gaussians(P, D)["lang"]
    a, b = sample_centers(field, lang, k=K, samples=S, seed=4), sample_centers(field, lang, k=K, samples=S, seed=4)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    c = sample_centers(field, lang, k=K, samples=S, seed=5)
    assert not torch.equal(a[0], c[0])


# ---- 5. the fused path is the two-step path ----------------------------------------------------------------
@pytest.mark.parametrize("mode", ("residual", "noresnet"))
@pytest.mark.parametrize("lang_dim", (3, 6))
def test_fused_path_is_the_two_step_path(mode, lang_dim):
    from deformation import LANG_NORESNET, LANG_RESIDUAL
    from language_centers import kmeans_rows, sample_centers
    P, S, K, seed = 67, 100, 3, 9
    field = _field(LANG_RESIDUAL if mode == "residual" else LANG_NORESNET, lang_dim)
    g = _gaussians(P, lang_dim)
    c, n, inertia, it, xs, ts = sample_centers(field, g["lang"], k=K, samples=S, seed=seed, debug=True)
    assert np.array_equal(ts.cpu().numpy(), cc.times_ref(seed, P, S))
    unit = g["lang"] / (g["lang"].norm(dim=-1, keepdim=True) + 1e-9)
    for s in (0, 63, 64, 99):
        ref = field.forward(g["means3D"], g["scales"], g["rotations"], g["opacity"], g["shs"], unit, ts[:, s])[5]
        assert _rel(xs[:, s].cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)) < 1e-4, s
    assert float((xs.norm(dim=-1) - 1).abs().max()) < 1e-5
    two = kmeans_rows(xs, K)
    assert torch.equal(c, two[0]) and torch.equal(n, two[1]) and torch.equal(it, two[3]) and torch.equal(inertia, two[2])
    plain = sample_centers(field, g["lang"], k=K, samples=S, seed=seed)
    assert len(plain) == 4 and all(torch.equal(u, v) for u, v in zip(plain, (c, n, inertia, it)))
    # explicit times are echoed and used
    tt = torch.rand(P, S, generator=torch.Generator().manual_seed(2)).cuda()
    out = sample_centers(field, g["lang"], k=K, samples=S, seed=seed, times=tt, debug=True)
    assert torch.equal(out[5], tt)
    ref = field.forward(g["means3D"], g["scales"], g["rotations"], g["opacity"], g["shs"], unit, tt[:, 64])[5]
    assert _rel(out[4][:, 64].cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)) < 1e-4
    again = sample_centers(field, g["lang"], k=K, samples=S, times=ts, debug=True)
    assert torch.equal(again[4], xs) and torch.equal(again[0], c)


# ---- 6. a time-independent language collapses -----------------------------------------------------------------
def _collapse(p):
    p["lang_deform.5.weight"].zero_()
    p["lang_deform.5.bias"].zero_()


def test_time_independent_language_collapses():
    from deformation import LANG_RESIDUAL
    from language_centers import sample_centers
    P, S, K, D = 67, 100, 3, 3
    field = _field(LANG_RESIDUAL, D, edit=_collapse)
    lang = _gaussians(P, D)["lang"]
    c, n, inertia, it = sample_centers(field, lang, k=K, samples=S)
    unit = lang / (lang.norm(dim=-1, keepdim=True) + 1e-9)
    assert float((c - unit[:, None]).abs().max()) <= 1e-6
    assert torch.equal(n.cpu(), torch.tensor([[S, 0, 0]] * P, dtype=torch.int32))


# ---- 7. refusals ----------------------------------------------------------------------------------------
def test_refusals():
    from deformation import LANG_DISCRETE, LANG_PASS, LANG_RESIDUAL
    from language_centers import kmeans_rows, sample_centers
    x = torch.zeros(4, 10, 3, device="cuda")
    for k, text in ((0, "1 <= K <= 8"), (9, "1 <= K <= 8")):
        with pytest.raises(RuntimeError, match=text):
            kmeans_rows(x, k)
    with pytest.raises(RuntimeError, match="K <= S <= 256"):
        kmeans_rows(x[:, :2], 3)
    with pytest.raises(RuntimeError, match="K <= S <= 256"):
        kmeans_rows(torch.zeros(2, 257, 3, device="cuda"), 3)
    with pytest.raises(RuntimeError, match="1 <= D <= 32"):
        kmeans_rows(torch.zeros(2, 10, 33, device="cuda"), 3)
    with pytest.raises(RuntimeError, match="max_iter >= 1"):
        kmeans_rows(x, 3, max_iter=0)
    field = _field(LANG_RESIDUAL, 3)
    lang = torch.ones(5, 3, device="cuda")
    for kw, text in ((dict(k=0), "1 <= K <= 8"), (dict(k=9, samples=100), "1 <= K <= 8"), (dict(k=3, samples=2), "K <= S"),
                     (dict(k=3, samples=257), "K <= S <= 256")):
        with pytest.raises(RuntimeError, match=text):
            sample_centers(field, lang, **kw)
    for other in (_field(LANG_PASS, 3), _field(LANG_DISCRETE, 3, centers=3)):
        with pytest.raises(RuntimeError, match="RESIDUAL or NORESNET"):
            sample_centers(other, lang)
    for bad in (lang.double(), lang.cpu()):
        with pytest.raises(ValueError, match="float32 CUDA tensor"):
            sample_centers(field, bad)
        with pytest.raises(ValueError, match="float32 CUDA tensor"):
            kmeans_rows(bad.reshape(1, 5, 3), 3)
    empty = kmeans_rows(torch.zeros(0, 10, 3, device="cuda"), 3)       # P = 0: nothing to do
    assert empty[0].shape == (0, 3, 3)
    torch.cuda.synchronize()                                               # nothing above left an error behind


# ---- 8. the stage hand-over runs ------------------------------------------------------------------------------
def _lang_step(collapsed=False):
    import synthetic
    from deformation import LANG_RESIDUAL, DeformationField
    from gaussian_train import GaussianTrainer
    from train_step import TrainStep
    P, W, H, D = 500, 64, 64, 3
    dev = torch.device("cuda")
    sc = synthetic.make_scene(P, C=D, tanfovx=0.6, tanfovy=0.6, seed=3, logscale_mean=-2.5).to(dev)
    cams = synthetic.camera_batch(2, W, H, tanfovx=0.6, seed=2)
    for i, cam in enumerate(cams):
        cam.time = 0.25 + 0.5 * i
    res, multires = [16, 16, 16, 10], [1, 2]
    aabb = [[7.0, 7.0, 10.5], [-7.0, -7.0, 1.5]]
    p = DeformationField.init_params(res, multires, aabb, seed=1, lang_mode=LANG_RESIDUAL, lang_dim=D)
    if collapsed:
        _collapse(p)
    field = DeformationField({k: v.to(dev) for k, v in p.items()}, res, multires, lang_mode=LANG_RESIDUAL, lang_dim=D)
    raw = {"xyz": sc.means3D.contiguous(), "f_dc": sc.shs[:, :1].contiguous(), "f_rest": sc.shs[:, 1:].contiguous(),
           "opacity": torch.logit(sc.opacities.reshape(P, 1)).contiguous(), "scaling": torch.log(sc.scales).contiguous(),
           "rotation": sc.rotations.contiguous(), "language_feature": (sc.lang * 1.3).contiguous()}
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3,
           "language_feature": 2.5e-3}
    step = TrainStep(GaussianTrainer(raw, lrs), field, stage="fine-lang", lam=0.2, addcosloss=True)
    g = torch.Generator().manual_seed(8)
    gt_lang = torch.rand(2, D, H, W, generator=g).to(dev)
    mask = (torch.rand(2, 1, H, W, generator=g) < 0.8).float().to(dev)
    return step, cams, gt_lang, mask, P, D


@pytest.mark.parametrize("init_from_stage", ("fine-base", "fine-lang"))
def test_stage_hand_over_runs(init_from_stage):
    from deformation import LANG_DISCRETE
    from language_centers import enter_discrete_stage
    step, cams, gt_lang, mask, P, D = _lang_step()
    assert math.isfinite(float(step(cams, None, gt_lang=gt_lang, lang_mask=mask)))
    old_field, old_tr = step.field, step.trainer
    kw = dict(generator=torch.Generator(device="cuda").manual_seed(1)) if init_from_stage == "fine-base" else dict(seed=3)
    new = enter_discrete_stage(step, init_from_stage, centers=3, **kw)
    assert new.stage == "fine-lang-discrete" and new.addcosloss and new.lam == 0.2
    tr, field = new.trainer, new.field
    assert tr["language_feature"].shape == (P, 3 * D)
    assert tr.steps["language_feature"] == 0 and not tr.exp_avg["language_feature"].any()
    assert tr.steps["xyz"] == old_tr.steps["xyz"] and torch.equal(tr["xyz"], old_tr["xyz"])
    assert field.lang_mode == LANG_DISCRETE and field.centers == 3 and field.lang_in == 3 * D
    shared = [k for k in old_field.p if not k.startswith("lang_deform.")]
    assert set(field.p) == set(shared) | {f"discrete_coff_generator.{i}.{w}" for i in (1, 3) for w in ("weight", "bias")}
    assert all(torch.equal(field.p[k], old_field.p[k]) for k in shared)
    before = tr["language_feature"].detach().clone()
    losses = [float(new(cams, None, gt_lang=gt_lang, lang_mask=mask)) for _ in range(2)]
    assert all(math.isfinite(v) for v in losses), losses
    assert not torch.equal(tr["language_feature"].detach(), before)
    assert len(new.coff) == 2 and all(tuple(c.shape) == (P, 3) for c in new.coff)
    with pytest.raises(ValueError, match="not lang_dim"):   # a language group that already holds centres
        enter_discrete_stage(new, init_from_stage, centers=3, **kw)


def test_hand_over_of_a_collapsed_field_keeps_the_static_feature():
    """With a time-independent language (test 6) all three centres are the normalised static feature, so
    whatever coff the fresh head gives, the discrete field's language is +- that feature."""
    from language_centers import enter_discrete_stage
    step, cams, gt_lang, mask, P, D = _lang_step(collapsed=True)
    lang = step.trainer["language_feature"].detach().clone()
    new = enter_discrete_stage(step, "fine-lang", centers=3)
    tr, g = new.trainer, _gaussians(P, D, seed=4)
    out = new.field.forward(tr["xyz"].detach(), g["scales"], g["rotations"], g["opacity"], g["shs"],
                            tr["language_feature"].detach(), 0.4)
    unit = lang / (lang.norm(dim=-1, keepdim=True) + 1e-9)
    err = torch.minimum((out[5] - unit).abs().amax(dim=1), (out[5] + unit).abs().amax(dim=1))
    assert float(err.max()) <= 1e-5
    assert tuple(out[6].shape) == (P, 3)


# ---- the fused kernel reads no LDS it did not write ---------------------------------------------------------------
def test_fused_path_under_lds_poison():
    """k_centers_from_field carries LDS_POISON like its neighbours in deform.hip: in the poison build
    (tests/test_deform_lds_poison_gpu.py) every block fills its shared memory with NaN words first, so a read
    of a row, a time or a sample the block never wrote turns the centres into NaN.  A child process,
    because the library is chosen when it is first loaded."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "4dlangsplat_amd", "build", "variants", "liblsr_ldspoison.so")
    assert os.path.exists(lib), "build the library first (make -C 4dlangsplat_amd/csrc builds the poison variant)"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        "tests/test_centers_gpu.py", "-k", "two_step_path or collapses"],
                       cwd=root, env=dict(os.environ, LSR_LIBRARY=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "5 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
