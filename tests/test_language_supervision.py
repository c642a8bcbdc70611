"""CPU checks of language_supervision (the 'lang' stages' supervision files and their fused loss)
against tests/golden/langsup_golden.npz: the REFERENCE's Camera.get_language_feature, l1_loss and
cos_loss on the seeded files and images of tests/langsup_cases.py
(tests/golden/make_langsup_golden.py), plus the argument checks of the C ABI, which run before a
device is touched."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import langsup_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "langsup_golden.npz")
CASES = range(len(lc.FIXTURE_CASES))


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def inputs(gold):
    out = []
    for k in CASES:
        inp = lc.fixture_inputs(k)
        assert lc.checksum([inp["images"]]) == str(gold[f"c{k}_images_sha256"]), "the seeded images changed"
        assert np.array_equal(inp["segs"], gold[f"c{k}_segs"]) and np.array_equal(inp["tables"], gold[f"c{k}_tables"])
        out.append(inp)
    return out


def _write(dirname, stem, segs, table):
    np.save(os.path.join(dirname, stem + "_s.npy"), segs)
    np.save(os.path.join(dirname, stem + "_f.npy"), table)


def _sups(gold, k):
    import language_supervision as ls
    level = int(gold[f"c{k}_level"])
    return [ls.SegmentSupervision(torch.from_numpy(gold[f"c{k}_segs"][v, level].copy()),
                                  torch.from_numpy(gold[f"c{k}_tables"][v].copy()))
            for v in range(lc.FIXTURE_CASES[k][0])]


@pytest.mark.parametrize("k", CASES)
def test_loader_and_dense_equal_the_reference(gold, tmp_path, k):
    import language_supervision as ls
    V = lc.FIXTURE_CASES[k][0]
    for v in range(V):
        colmap_id, data_type, split, cam_name = lc.FIXTURE_VIEWS[k][v]
        stem = ls.supervision_stem(colmap_id, data_type, split, cam_name)
        assert stem == str(gold[f"c{k}_stems"][v])
        _write(tmp_path, stem, gold[f"c{k}_segs"][v], gold[f"c{k}_tables"][v])
    for level in range(4):
        stems = [str(s) for s in gold[f"c{k}_stems"]]
        sups = ls.load_all(str(tmp_path), stems + [None], level, "cpu")
        assert sups[-1] is None and len(sups) == V + 1
        for v in range(V):
            gt, mask = sups[v].dense()
            ref_gt = torch.from_numpy(gold[f"c{k}_gt_hwc"][v, level]).permute(2, 0, 1)
            ref_mask = torch.from_numpy(gold[f"c{k}_mask"][v, level])
            assert gt.dtype == torch.float32 and mask.dtype == torch.bool
            assert gt.shape == ref_gt.shape and mask.shape == ref_mask.shape == (1,) + tuple(gt.shape[1:])
            assert torch.equal(gt, ref_gt) and torch.equal(mask, ref_mask)
            assert sups[v].seg.dtype == torch.int32 and sups[v].table.dtype == torch.float32


def test_a_float_map_of_whole_numbers_loads(gold, tmp_path):
    import language_supervision as ls
    _write(tmp_path, "f", gold["c1_segs"][0].astype(np.float32), gold["c1_tables"][0].astype(np.float64))
    _write(tmp_path, "i", gold["c1_segs"][0], gold["c1_tables"][0])
    a, b = ls.load_language_supervision(str(tmp_path), "f", 2), ls.load_language_supervision(str(tmp_path), "i", 2)
    assert torch.equal(a.seg, b.seg) and torch.equal(a.table, b.table) and a.seg.dtype == torch.int32


def test_stems_equal_the_references_names(gold):
    import language_supervision as ls
    for (colmap_id, data_type, split, cam_name), want in zip(lc.STEM_QUERIES, gold["stems"]):
        got = ls.supervision_stem(colmap_id, data_type, split, cam_name)
        assert (got or "") == str(want), (colmap_id, data_type, split, cam_name)
    assert ls.supervision_stem(612, "dynerf", "video", "cam03") is None
    assert ls.supervision_stem(5, "nerfies") == "000021"
    with pytest.raises(ValueError, match="colmap_id < 300"):
        ls.supervision_stem(300, "dynerf", "test", "cam00")
    with pytest.raises(ValueError, match="nerfies"):
        ls.supervision_stem(1, "PanopticSports")


def test_loader_refusals(gold, tmp_path):
    import language_supervision as ls
    segs, table = gold["c1_segs"][0], gold["c1_tables"][0]
    S = table.shape[0]
    d = str(tmp_path)
    _write(d, "ok", segs, table)
    for level in (-1, 4, 1.0, "1", True):
        with pytest.raises(ValueError, match="feature_level"):
            ls.load_language_supervision(d, "ok", level)
    _write(d, "rank_s", segs[0], table)
    with pytest.raises(ValueError, match=r"\[4, H, W\]"):
        ls.load_language_supervision(d, "rank_s", 0)
    _write(d, "rank_f", segs, table[0])
    with pytest.raises(ValueError, match=r"\[S, C\]"):
        ls.load_language_supervision(d, "rank_f", 0)
    _write(d, "levels", segs[:2], table)
    with pytest.raises(ValueError, match=r"\[4, H, W\]"):
        ls.load_language_supervision(d, "levels", 2)
    frac = segs.astype(np.float32)
    frac[1, 0, 0] = 0.5
    _write(d, "frac", frac, table)
    with pytest.raises(ValueError, match="whole numbers"):
        ls.load_language_supervision(d, "frac", 1)
    assert ls.load_language_supervision(d, "frac", 0).seg.dtype == torch.int32      # the other levels are whole
    nan = segs.astype(np.float64)
    nan[3, 2, 2] = np.nan
    _write(d, "nan", nan, table)
    with pytest.raises(ValueError, match="whole numbers"):
        ls.load_language_supervision(d, "nan", 3)
    big = segs.copy()
    big[2, 1, 1] = S                                   # the reference would fail with an IndexError
    _write(d, "big", big, table)
    with pytest.raises(ValueError, match="outside"):
        ls.load_language_supervision(d, "big", 2)
    low = segs.copy()
    low[2, 1, 1] = -2
    _write(d, "low", low, table)
    with pytest.raises(ValueError, match="outside"):
        ls.load_language_supervision(d, "low", 2)
    with pytest.raises(ValueError, match="int32"):
        ls.SegmentSupervision(torch.zeros(3, 3, dtype=torch.int64), torch.zeros(2, 3))
    with pytest.raises(ValueError, match="float32"):
        ls.SegmentSupervision(torch.zeros(3, 3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.float64))


def _loss_and_grads(images, sups, cos, dtype):
    import language_supervision as ls
    xs = [torch.from_numpy(x.copy()).to(dtype).requires_grad_(True) for x in images]
    loss = ls.segment_lang_loss(xs, sups, lc.LAM, lc.BETA, addcosloss=cos)
    loss.backward()
    return loss.detach(), torch.stack([x.grad for x in xs])


@pytest.mark.parametrize("name", ("l1", "cos"))
@pytest.mark.parametrize("k", CASES)
def test_fallback_float64_equals_the_reference(gold, inputs, k, name):
    loss, grad = _loss_and_grads(inputs[k]["images"], _sups(gold, k), name == "cos", torch.float64)
    ref_loss, ref_grad = float(gold[f"c{k}_{name}_loss"]), gold[f"c{k}_{name}_grad"]
    assert loss.dtype == torch.float64
    assert abs(float(loss) - ref_loss) <= 1e-12 * abs(ref_loss), (float(loss), ref_loss)
    err = float(np.abs(grad.numpy() - ref_grad).max())
    assert err <= 1e-12 * float(np.abs(ref_grad).max()), err


@pytest.mark.parametrize("name", ("l1", "cos"))
@pytest.mark.parametrize("k", CASES)
def test_fallback_float32_within_the_references_float32_error(gold, inputs, k, name):
    """8 x the float32 reference run's own error against float64: the margin the query tests use for
    a re-ordered float32 evaluation."""
    loss, grad = _loss_and_grads(inputs[k]["images"], _sups(gold, k), name == "cos", torch.float32)
    assert loss.dtype == torch.float32 and grad.dtype == torch.float32
    e_loss = abs(float(loss) - float(gold[f"c{k}_{name}_loss"]))
    e_grad = float(np.abs(grad.numpy().astype(np.float64) - gold[f"c{k}_{name}_grad"]).max())
    print(f"case {k} {name}: loss error {e_loss:.3g} (reference {float(gold[f'c{k}_{name}_loss_f32_err']):.3g}), "
          f"gradient error {e_grad:.3g} (reference {float(gold[f'c{k}_{name}_grad_f32_err']):.3g})")
    assert e_loss <= 8 * float(gold[f"c{k}_{name}_loss_f32_err"])
    assert e_grad <= 8 * float(gold[f"c{k}_{name}_grad_f32_err"])


@pytest.mark.parametrize("cos", (False, True))
def test_indices_past_the_table_count_as_unlabelled(cos):
    import language_supervision as ls
    V, C, H, W, S = 2, 5, 4, 23, 6
    segs, tables, images = lc.sweep_case(V, C, H, W, S, oob=True)
    assert (segs >= S).any() and (segs < -1).any()
    marked = np.where((segs >= 0) & (segs < S), segs, -1).astype(np.int32)
    mk = lambda s: [ls.SegmentSupervision(torch.from_numpy(s[v].copy()), torch.from_numpy(tables[v].copy()))  # noqa: E731
                    for v in range(V)]
    l0, g0 = _loss_and_grads(images, mk(segs), cos, torch.float64)
    l1, g1 = _loss_and_grads(images, mk(marked), cos, torch.float64)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert bool((g0[torch.from_numpy(marked < 0)[:, None].expand_as(g0)] == 0).all())
    gt, mask = mk(segs)[0].dense()                       # never an index error, the mask the labelled pixels
    assert torch.equal(mask[0], torch.from_numpy(marked[0] >= 0)) and gt.shape == (C, H, W)


def test_argument_mismatches_are_refused():
    import language_supervision as ls
    sup = ls.SegmentSupervision(torch.zeros(4, 6, dtype=torch.int32), torch.zeros(2, 3))
    x = torch.zeros(3, 4, 6)
    with pytest.raises(ValueError, match="one SegmentSupervision per image"):
        ls.segment_lang_loss([x, x], [sup])
    with pytest.raises(ValueError, match="one SegmentSupervision per image"):
        ls.segment_lang_loss([], [])
    with pytest.raises(ValueError, match="share one"):
        ls.segment_lang_loss([x, torch.zeros(3, 4, 5)], [sup, sup])
    with pytest.raises(ValueError, match="share one"):
        ls.segment_lang_loss([x, x.double()], [sup, sup])
    with pytest.raises(ValueError, match="channels"):
        ls.segment_lang_loss([torch.zeros(2, 4, 6)], [sup])
    with pytest.raises(ValueError, match="SegmentSupervision per view"):
        ls.segment_lang_loss([x], [(sup.seg, sup.table)])
    assert not ls.native_eligible([x], [sup])            # CPU tensors never reach the library


def test_abi_refusals():
    """Every refusal of lsr_seg_loss_* is LSR_EINVAL with a message, decided before a device is touched."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    err = lambda: lib.lsr_last_error().decode()   # noqa: E731
    FAKE = 64                                      # never dereferenced: every call below returns early

    def views(n=2, **over):
        arr = (_lib.SegView * max(n, 1))()
        for v in arr:
            v.image = v.d_image = v.seg = v.table = FAKE
            v.n_seg = 3
        for name, val in over.items():
            setattr(arr[n - 1], name, val)
        return arr

    p = ctypes.c_void_p(FAKE)
    assert lib.lsr_seg_loss_workspace_bytes(2, 32, 19, 37) >= 8 * 2 * 19 + 12 * 2 * 32 * 19
    assert lib.lsr_seg_loss_workspace_bytes(8, 1, 1, 1) > 0
    for sizes in ((0, 3, 4, 5), (9, 3, 4, 5), (-1, 3, 4, 5), (2, 0, 4, 5), (2, 3, 0, 5), (2, 3, 4, 0), (2, 3, 4, -7)):
        assert lib.lsr_seg_loss_workspace_bytes(*sizes) == -1 and "1 <= V <= 8" in err()
        assert lib.lsr_seg_loss_views(*sizes, views(), 0.2, 0.01, 1, p, p, None) == 1 and "1 <= V <= 8" in err()
        assert lib.lsr_seg_loss_views_backward(*sizes, views(), 0.2, 0.01, 1, p, p, None) == 1
        assert "1 <= V <= 8" in err()
    ok = (2, 3, 4, 5)
    fwd = lambda v, loss=p, ws=p, cos=1: lib.lsr_seg_loss_views(*ok, v, 0.2, 0.01, cos, loss, ws, None)   # noqa: E731
    bwd = lambda v, g=p, ws=p, cos=1: lib.lsr_seg_loss_views_backward(*ok, v, 0.2, 0.01, cos, g, ws, None)  # noqa: E731
    for f in (fwd, bwd):
        assert f(None) == 1 and "views required" in err()
        for n_seg in (0, -1):
            assert f(views(n_seg=n_seg)) == 1 and "n_seg >= 1" in err()
        for field in ("image", "seg", "table"):
            assert f(views(**{field: None})) == 1 and "null image, seg or table" in err()
        assert f(views(), ws=None) == 1 and "workspace required" in err()
    assert fwd(views(), loss=None) == 1 and "loss required" in err()
    assert fwd(views(), ws=None, cos=0) == 1 and "workspace required" in err()
    assert bwd(views(), g=None) == 1 and "d_loss required" in err()
    assert bwd(views(d_image=None)) == 1 and "null gradient image" in err()


def test_seg_view_mirror_matches_the_header(tmp_path):
    """SegView against gcc's offsetof / sizeof of lsr_seg_view, as test_ctypes_structs_match_the_headers."""
    from diff_gaussian_rasterization import _lib
    names = [f[0] for f in _lib.SegView._fields_]
    assert len(names) == len(set(names))
    lines = ["#include <stddef.h>", "#include <stdio.h>",
             f'#include "{os.path.join(ROOT, "include", "lsr_train.h")}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(lsr_seg_view));']
    lines += [f'printf("{n} %zu\\n", offsetof(lsr_seg_view, {n}));' for n in names] + ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    want = {n: str(getattr(_lib.SegView, n).offset) for n in names}
    want["size"] = str(ctypes.sizeof(_lib.SegView))
    assert got == want
    assert _lib.SEG_LOSS_MAX_VIEWS == 8


def _cpu_step(**kw):
    """A TrainStep over a stand-in trainer: enough for loss() and the argument checks, no device."""
    from train_step import TrainStep
    trainer = types.SimpleNamespace(params={"language_feature": torch.zeros(4, 3)}, device=torch.device("cpu"))
    return TrainStep(trainer, None, stage="fine-lang", **kw)


def test_train_step_refuses_both_supervision_forms(gold):
    step = _cpu_step()
    sup = _sups(gold, 1)[0]
    gt, mask = sup.dense()
    for call in (lambda **k: step.loss([], None, **k), lambda **k: step.forward_backward([], None, **k),
                 lambda **k: step([], None, **k)):
        with pytest.raises(ValueError, match="not both"):
            call(gt_lang=gt[None], lang_mask=mask[None], lang_sup=[sup])
        with pytest.raises(ValueError, match="not both"):
            call(gt_lang=gt[None], lang_sup=[sup])
    with pytest.raises(ValueError, match="needs gt_lang and lang_mask"):
        step.loss([], None)
    assert step.iteration == 0


@pytest.mark.parametrize("cos", (False, True))
def test_train_step_loss_takes_either_form(gold, inputs, cos):
    """TrainStep.loss with lang_sup equals its dense expression on sup.dense() (float64, CPU)."""
    step = _cpu_step(addcosloss=cos, lam=0.3, beta=0.02)
    sups = _sups(gold, 0)
    outs = [{"language_feature_image": torch.from_numpy(x.copy()).double()} for x in inputs[0]["images"]]
    dense = [s.dense() for s in sups]
    want = step.loss(outs, None, gt_lang=torch.stack([g for g, _ in dense]).double(),
                     lang_mask=torch.stack([m for _, m in dense]))
    got = step.loss(outs, None, lang_sup=sups)
    assert abs(float(got) - float(want)) <= 1e-13 * abs(float(want))
