"""CPU checks of the open-vocabulary segmentation (language_query.segment / segment_frames): the torch
fallback against the fixture made from the reference's own activate_stream and smooth_cuda
(tests/golden/make_segment_golden.py), the edge maps, the argument checks of the Python surface and of
the C ABI (include/lsr_segment.h; no GPU compute is called here).

Tolerance rule, as tests/test_query_gpu.py: against the float64 value, blended and score may be off by
at most 8x the float32 reference's own error (stored in the fixture); in float64 by 1e-12.  Masks,
counts, levels and the chosen IoU are equal."""
import ctypes
import os

import numpy as np
import pytest
import torch

import query_cases as qc
import segment_cases as sc
from diff_gaussian_rasterization import _lib
from language_query import LanguageDecoder, Segmentation, relevancy, segment, segment_frames

TOL = 8.0


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "segment_golden.npz")))
    rel, gt = sc.fixture_inputs()
    assert str(g["inputs_sha256"]) == sc.checksum([rel, gt])
    return g, torch.from_numpy(rel), torch.from_numpy(gt)


def check_against_fixture(seg, g, strategy, dtype):
    """A Segmentation of the fixture's inputs against the fixture, under the module's rule."""
    tol_b = TOL * float(g["blended_f32_err"]) if dtype == torch.float32 else 1e-12
    tol_s = TOL * float(g[f"score_{strategy}_f32_err"]) if dtype == torch.float32 else 1e-12
    e_b = float((seg.blended.cpu().double() - torch.from_numpy(g["blended"])).abs().max())
    e_s = float((seg.score.cpu().double() - torch.from_numpy(g[f"score_{strategy}"])).abs().max())
    print(f"{strategy} {dtype}: blended error {e_b:.3g} (allowed {tol_b:.3g}), score error {e_s:.3g} (allowed {tol_s:.3g})")
    assert seg.blended.dtype == dtype and seg.score.dtype == dtype
    assert e_b <= tol_b and e_s <= tol_s
    assert seg.mask_raw.dtype == torch.bool and seg.mask.dtype == torch.bool
    assert np.array_equal(seg.mask_raw.cpu().numpy(), g["mask_raw"] != 0)
    assert np.array_equal(seg.mask.cpu().numpy(), g["mask"] != 0)
    assert np.array_equal(seg.inter.cpu().numpy(), g["inter"]) and np.array_equal(seg.union.cpu().numpy(), g["union"])
    level = torch.from_numpy(g[f"level_{strategy}"])
    assert seg.level.dtype == torch.int64 and torch.equal(seg.level.cpu(), level)
    assert torch.equal(seg.chosen_mask.cpu(), seg.mask.cpu()[level, torch.arange(level.numel())])
    # the reference keeps its IoU in float32: the quotient of the same two integers, rounded once
    assert np.array_equal(seg.chosen_iou.cpu().float().numpy(), g[f"chosen_iou_{strategy}"])
    assert torch.equal(seg.iou.cpu(), (seg.inter.cpu().to(dtype) / seg.union.cpu().to(dtype)))


@pytest.mark.parametrize("strategy", ["point", "mean"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_fallback_matches_the_fixture(golden, strategy, dtype):
    g, rel, gt = golden
    assert float(g["thresh"]) == 0.4 and int(g["scale"]) == 29           # segment()'s defaults
    seg = segment(rel.to(dtype), gt, strategy=strategy)
    assert isinstance(seg, Segmentation) and seg.blended.shape == (2, 3, 61, 83) and seg.score.shape == (2, 3)
    check_against_fixture(seg, g, strategy, dtype)
    # bool annotations, and one level alone ([n_pos, H, W]: the level axis is dropped)
    assert torch.equal(segment(rel.to(dtype), gt != 0, strategy=strategy).inter, seg.inter)
    one = segment(rel[1].to(dtype), gt, strategy=strategy)
    assert one.blended.shape == (3, 61, 83) and one.score.shape == (3,) and one.iou.shape == (3,)
    assert torch.equal(one.blended, seg.blended[1]) and torch.equal(one.mask, seg.mask[1])
    assert torch.equal(one.union, seg.union[1]) and torch.equal(one.level, torch.zeros(3, dtype=torch.int64))
    assert torch.equal(one.chosen_iou, seg.iou[1])


def test_the_fixture_tests_something(golden):
    g, _, _ = golden
    iou = g["inter"] / g["union"]
    assert 0.2 < float(g["mask_raw"].mean()) < 0.5 and iou.min() > 0.2 and iou.max() < 0.9
    assert len(set(g["level_point"].tolist())) == 2


def test_without_annotations(golden):
    g, rel, gt = golden
    seg = segment(rel)
    assert seg.inter is None and seg.union is None and seg.iou is None and seg.chosen_iou is None
    assert np.array_equal(seg.mask.numpy(), g["mask"] != 0)


def test_rel_is_not_modified_and_views_are_taken(golden):
    _, rel, gt = golden
    keep = rel.clone()
    seg = segment(rel, gt)
    assert torch.equal(rel, keep)                      # the reference overwrites its maps in place
    t = rel.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)          # same values, other strides
    assert not t.is_contiguous()
    seg_t = segment(t, gt.permute(0, 2, 1).contiguous().permute(0, 2, 1))
    assert torch.equal(seg_t.blended, seg.blended) and torch.equal(seg_t.inter, seg.inter)


def test_smaller_windows(golden):
    """scale 1 is no smoothing at all (blended == rel); scale 63 is wider than the 61-row image."""
    _, rel, gt = golden
    assert torch.equal(segment(rel, gt, scale=1).blended, 0.5 * (rel + rel))
    b = segment(rel.double(), gt, scale=63).blended
    a = 2 * b - rel.double()                           # the smoothed map: the window at row 30 holds all 61 rows
    assert float((a[..., 30, 41] - rel.double()[..., :, 10:73].mean(dim=(-1, -2))).abs().max()) < 1e-12


def test_edge_maps():
    H, W = 9, 11
    gt = torch.zeros(2, H, W, dtype=torch.uint8)
    gt[0, 2:6, 3:8] = 1
    # a constant map: o = 0 / 1e-9 * 2 - 1 = -1 everywhere, empty masks, union = the annotation, IoU 0 (0 / 0 = NaN)
    seg = segment(torch.full((3, 2, H, W), 0.5), gt)
    assert not seg.mask_raw.any() and not seg.mask.any()
    assert torch.equal(seg.union, torch.tensor([[20, 0]] * 3)) and torch.equal(seg.inter, torch.zeros(3, 2, dtype=torch.int64))
    assert bool((seg.iou[:, 0] == 0).all()) and bool(seg.iou[:, 1].isnan().all())
    assert bool((seg.score == 0.5).all()) and torch.equal(seg.level, torch.zeros(2, dtype=torch.int64))   # ties: level 0
    assert float(seg.chosen_iou[0]) == 0.0 and bool(seg.chosen_iou[1].isnan())
    assert bool((segment(torch.full((3, 2, H, W), 0.5), gt, strategy="mean").score == 0).all())
    # one NaN pixel: min and max are NaN, the masks empty, the score NaN, and that level is chosen
    rel, _ = sc.maps(3, 2, H, W, 5)
    rel = torch.from_numpy(rel)
    rel[1, 0, 4, 4] = float("nan")
    seg = segment(rel, gt)
    assert not seg.mask_raw[1, 0].any() and not seg.mask[1, 0].any() and bool(seg.score[1, 0].isnan())
    assert int(seg.score.isnan().sum()) == 1 and seg.mask_raw[1, 1].any() and seg.mask_raw[0, 0].any()
    assert seg.level.tolist()[0] == 1 and int(seg.union[1, 0]) == 20
    mean = segment(rel, gt, strategy="mean")
    assert float(mean.score[1, 0]) == 0.0 and not mean.mask_raw[1, 0].any()


def test_the_threshold_is_compared_in_the_maps_dtype():
    """torch compares a float32 tensor with float32(thresh) (eval.py:241): a threshold 1e-10 below a
    pixel's stretched value o rounds to o in float32, and o > o is False, where a comparison in double
    would say True.  (With the default 0.4 the two never differ: o = 2 q - 1 with q in [0.5, 1) is a
    multiple of 2^-23, and 0.4 and float32(0.4) lie between the same two multiples.)"""
    v = torch.tensor([[0.0, 0.7, 1.0]])[None]          # blended = the map at scale 1: 0.5 * (v + v)
    o = float((v[0, 0, 1] - 0.0) / (torch.tensor(1.0) + 1e-9) * 2.0 + (-1.0))
    t = o - 1e-10
    assert t < o and float(torch.tensor(t, dtype=torch.float32)) == o
    assert segment(v, scale=1, thresh=t).mask_raw.tolist() == [[[False, False, True]]]
    assert segment(v, scale=1, thresh=o - 1e-7).mask_raw.tolist() == [[[False, True, True]]]


def test_argument_checks(golden):
    _, rel, gt = golden
    with pytest.raises(ValueError, match="scale must be odd .* got scale = 28"):
        segment(rel, gt, scale=28)
    with pytest.raises(ValueError, match="got scale = 65"):
        segment(rel, gt, scale=65)
    with pytest.raises(ValueError, match=r"gt_masks must be \[n_pos, H, W\] = \(3, 61, 83\).*got \(3, 83, 61\)"):
        segment(rel, gt.permute(0, 2, 1))
    with pytest.raises(ValueError, match=r"got \(2, 61, 83\)"):
        segment(rel, gt[:2])
    with pytest.raises(ValueError, match="gt_masks is on meta but rel is on cpu"):
        segment(rel, gt.to("meta"))
    with pytest.raises(ValueError, match="gt_masks must be bool or uint8, got torch.float32"):
        segment(rel, gt.float())
    with pytest.raises(ValueError, match='strategy must be "point" or "mean", got \'adaptive\''):
        segment(rel, gt, strategy="adaptive")
    with pytest.raises(ValueError, match=r"rel must be \[L, n_pos, H, W\] or \[n_pos, H, W\], got \(61, 83\)"):
        segment(rel[0, 0])


def test_segment_frames(tmp_path):
    """Three tiny frames in three level folders: the written masks are segment()'s chosen masks of
    relevancy() of the frame, and the table and mean IoU are eval.py:667-690's."""
    dims, H, W = [3, 16, 32], 12, 10
    ws, bs = qc.decoder_arrays(dims, 21)
    dec = LanguageDecoder.from_state_dict(qc.state_dict(ws, bs, torch))
    frames = [qc.latents((3, H, W, 3), 22 + i) for i in range(3)]
    frames[0] = np.abs(frames[0]) * 0.9 + 0.05         # saved in (0, 1): mapped back by x * 2 - 1
    levels = []
    for l in range(3):
        d = tmp_path / f"level_{l + 1}"
        (d / "renders_npy").mkdir(parents=True)
        for i, fr in enumerate(frames):
            np.save(d / "renders_npy" / f"{i:05d}.npy", fr[l].astype(np.float32))
        levels.append(str(d))
    e = torch.from_numpy(qc.phrase_embeddings(ws, bs, frames[1].reshape(-1, 3), 4, 25))
    pos, neg = e[:2], e[2:]
    gt = {f"{i:05d}": sc.maps(1, 2, H, W, 30 + i)[1] for i in (0, 2)}     # frame 1 has no annotation
    out = tmp_path / "seg"
    res = segment_frames(levels, dec, pos, neg, str(out), gt=gt, scale=5, thresh=0.3)
    assert [os.path.relpath(p, out) for p in res["paths"]] == [f"mask_npy/{i:05d}.npy" for i in range(3)]
    assert sorted(res["table"]) == ["00000", "00002"]
    ious = []
    for i, fr in enumerate(frames):
        x = torch.from_numpy(fr)
        rel = relevancy(x * 2.0 - 1 if i == 0 else x, dec, pos, neg)
        want = segment(rel, None if i == 1 else torch.from_numpy(gt[f"{i:05d}"]), scale=5, thresh=0.3)
        got = np.load(res["paths"][i])
        assert got.dtype == np.uint8 and got.shape == (2, H, W)
        assert np.array_equal(got, want.chosen_mask.numpy().astype(np.uint8))
        if i != 1:
            rows = res["table"][f"{i:05d}"]
            assert [r[1] for r in rows] == want.level.tolist()
            assert [r[2] for r in rows] == want.score.T.tolist()
            assert np.array_equal(np.array([r[0] for r in rows]), want.chosen_iou.double().numpy(), equal_nan=True)
            ious.append(want.chosen_iou.double().numpy())
    per_phrase = np.mean(ious, axis=0)
    assert np.allclose(res["phrase_iou"], per_phrase, equal_nan=True, rtol=0, atol=1e-12)
    assert res["mean_iou"] == pytest.approx(per_phrase.mean(), abs=1e-12, nan_ok=True)
    assert set(segment_frames(levels, dec, pos, neg, str(tmp_path / "plain"))) == {"paths"}
    with pytest.raises(FileNotFoundError):
        segment_frames([str(tmp_path / "nowhere")], dec, pos, neg, str(out))


def test_abi_argument_checks():
    """include/lsr_segment.h: invalid arguments are LSR_EINVAL with a message, before anything touches a
    device; n_maps = 0 is accepted and launches nothing."""
    lib = _lib.load()
    err = lambda: lib.lsr_last_error().decode()
    p = ctypes.c_void_p(64)                            # never dereferenced: every call below returns early

    def call(n_maps=4, H=32, W=48, rel=p, scale=29, thresh=0.4, strategy=0, gt=p, gt_count=2, blended=p, mask_raw=p,
             mask=p, score=p, inter=p, union=p, ws=p):
        return lib.lsr_segment(n_maps, H, W, rel, scale, thresh, strategy, gt, gt_count, blended, mask_raw, mask, score,
                               inter, union, ws, None)

    def refused(rc, text):
        assert rc == 1 and text in err(), (rc, err())  # LSR_EINVAL

    for scale in (0, 2, 28, 64, 65, -1):
        refused(call(scale=scale), f"scale must be odd and in 1 ... 63, got {scale}")
    for kw in (dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(n_maps=-1)):
        refused(call(**kw), "n_maps >= 0 and 1 <= H, W <= 16384")
    refused(call(strategy=2), "strategy must be 0 (point) or 1 (mean)")
    for name in ("rel", "blended", "mask_raw", "mask", "score"):
        refused(call(**{name: None}), "null rel, blended, mask_raw, mask or score")
    refused(call(ws=None), "workspace required")
    refused(call(ws=ctypes.c_void_p(72)), "16-byte aligned")
    refused(call(gt=None), "given together or not at all")
    refused(call(inter=None), "given together or not at all")
    refused(call(union=None), "given together or not at all")
    refused(call(gt_count=0), "gt_count >= 1")
    assert call(n_maps=0) == 0 and call(n_maps=0, rel=None, ws=None) == 0
    refused(call(n_maps=0, scale=4), "scale must be odd")

    assert lib.lsr_segment_workspace_bytes(0, 32, 48) >= 0
    one, many = lib.lsr_segment_workspace_bytes(1, 1014, 1352), lib.lsr_segment_workspace_bytes(24, 1014, 1352)
    tiles = ((1352 + 63) // 64) * ((1014 + 31) // 32)
    assert one >= tiles * (8 + 8 + 4) and one < many <= 24 * one and many < 1 << 20
    for args in ((-1, 8, 8), (1, 0, 8), (1, 8, 16385)):
        assert lib.lsr_segment_workspace_bytes(*args) == -1 and "1 <= H, W <= 16384" in err()
