"""GPU checks of the fused segmentation (csrc/segment.hip through language_query.segment).

Two kinds of check:
  * exact: on maps quantised to multiples of 2^-12 every window sum is exact in float32 in any order
    (63 * 63 * 4096 < 2^24), so the native path must equal the float32 CPU fallback (torch ops) bit for
    bit in every output.  This pins the count-excluding-padding divisor, the halo logic, the float32
    cast of thresh, the two-rounding stretch and the integer majority rule.  The "mean" score is a
    double sum rounded to float32 on both sides; the two sum in different orders, which could differ
    only where the exact mean lies within about 1e-13 (relative) of a float32 rounding boundary.
  * within the tolerance rule of tests/test_query_gpu.py on unquantised maps: against the float64
    fallback, blended and score may be off by at most 8x the float32 reference's own error (for the
    fixture the one its generator measured on the reference's code, otherwise the float32 fallback's,
    measured here).  mask_raw must equal the float64 mask wherever the float64 stretched value is
    further than 1e-5 from thresh, and such near pixels may be at most 0.1 % of a map; mask must be
    smooth_cuda of the kernel's own mask_raw, and the counts exact sums over the kernel's own mask."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import language_query
import query_cases as qc
import segment_cases as sc
from diff_gaussian_rasterization import _lib
from language_query import LanguageDecoder, relevancy, segment

pytestmark = pytest.mark.gpu
TOL = 8.0
NEAR = 1e-5
# (1, 1), (5, 7): smaller than both windows; (33, 65): one pixel past a tile each way; (97, 150): interior halos
SHAPES = [(1, 1), (5, 7), (29, 30), (37, 29), (33, 65), (70, 131), (97, 150)]
STRATEGIES = ["point", "mean"]
FIELDS = ("blended", "mask_raw", "mask", "score", "level", "chosen_mask", "inter", "union", "iou", "chosen_iou")


@functools.lru_cache(maxsize=None)
def quantised(H, W, L=3, n_pos=5):
    rel, gt = sc.maps(L, n_pos, H, W, 1000 + 7 * H + W, quantised=True)
    return torch.from_numpy(rel), torch.from_numpy(gt)


def same(a, b):
    """Equal bit for bit, NaN equal to NaN."""
    a, b = a.cpu(), b.cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))
    return torch.equal(a, b)


def assert_same_segmentation(got, want, what):
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None) == (w is None), (what, f)
        if g is not None:
            assert g.is_cuda and same(g, w), f"{what}: {f} differs from the float32 CPU fallback"


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_exact_parity_on_quantised_maps(H, W, strategy):
    rel, gt = quantised(H, W)
    want = segment(rel, gt, strategy=strategy)
    got = segment(rel.cuda(), gt.cuda(), strategy=strategy)
    assert got.blended.dtype == torch.float32 and got.mask.dtype == torch.bool and got.inter.dtype == torch.int64
    assert_same_segmentation(got, want, f"{H}x{W} {strategy}")
    if H * W > 1000:
        assert 0.1 < float(want.mask_raw.float().mean()) < 0.6          # the case tests something


@pytest.mark.parametrize("scale", [1, 3, 57, 59, 63])
def test_exact_parity_at_other_scales(scale):
    """1 and 3: windows inside the cleaning window's halo; 57 is the widest window of the 32-row tile, 59 the
    first of the 16-row tile, 63 the widest allowed.  With a threshold of its own and no annotations."""
    rel, _ = quantised(70, 131)
    for strategy in STRATEGIES:
        want = segment(rel, thresh=0.25, scale=scale, strategy=strategy)
        got = segment(rel.cuda(), thresh=0.25, scale=scale, strategy=strategy)
        assert_same_segmentation(got, want, f"scale {scale} {strategy}")


def test_annotation_kinds_and_single_level():
    rel, gt = quantised(33, 65)
    want = segment(rel, gt)
    assert_same_segmentation(segment(rel.cuda(), gt.cuda() != 0), want, "bool annotations")
    assert_same_segmentation(segment(rel.cuda(), gt.cuda() * 255), want, "annotations of 0 / 255")
    one = segment(rel[2].cuda(), gt.cuda())
    assert one.blended.shape == (5, 33, 65) and same(one.mask, want.mask[2]) and same(one.iou, want.iou[2])
    t = rel.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).cuda()   # same values, other strides
    keep = t.clone()
    assert_same_segmentation(segment(t, gt.cuda()), want, "non-contiguous rel")
    assert torch.equal(t, keep)                        # rel is not modified


def stretched(b64):
    """eval.py:185-189 on [..., H, W] float64 blended maps."""
    o = b64 - b64.amin(dim=(-1, -2), keepdim=True)
    o = o / (o.amax(dim=(-1, -2), keepdim=True) + 1e-9)
    return torch.clip(o * 2.0 + (-1.0), 0, 1)


def smooth_cuda(mask_raw):
    """eval/eval_utils.py:95-100 on [..., H, W] bool."""
    x = mask_raw.float().reshape(-1, 1, *mask_raw.shape[-2:])
    f = torch.nn.functional.avg_pool2d(x, 7, 1, 3, count_include_pad=False)
    return (f > 0.5).reshape(mask_raw.shape)


def check_rules(seg, gt, b64, score64, err_b, err_s, what, thresh=0.4):
    e_b = float((seg.blended.cpu().double() - b64).abs().max())
    e_s = float((seg.score.cpu().double() - score64).abs().max())
    o64 = stretched(b64)
    far = (o64 - thresh).abs() > NEAR
    near_share = float((~far).double().mean(dim=(-1, -2)).max())
    differ = int(((seg.mask_raw.cpu() != (o64 > thresh)) & far).sum())
    print(f"{what}: blended error {e_b:.3g} (float32 reference {err_b:.3g}), score error {e_s:.3g} (float32 reference "
          f"{err_s:.3g}), near-threshold share {near_share:.3g}, "
          f"{int((seg.mask_raw.cpu() != (o64 > thresh)).sum())} mask_raw pixels differ from float64")
    assert e_b <= TOL * err_b and e_s <= TOL * err_s
    assert near_share <= 1e-3 and differ == 0
    assert torch.equal(seg.mask.cpu(), smooth_cuda(seg.mask_raw.cpu()))
    g = (gt != 0).to(seg.mask.device)
    assert torch.equal(seg.inter, (g & seg.mask).flatten(-2).sum(-1))
    assert torch.equal(seg.union, (g | seg.mask).flatten(-2).sum(-1))
    assert same(seg.iou, seg.inter.float() / seg.union.float())
    assert torch.equal(seg.level, torch.argmax(seg.score.reshape(-1, seg.score.shape[-1]), dim=0))


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_fixture_parity(golden_dir, strategy):
    g = dict(np.load(os.path.join(golden_dir, "segment_golden.npz")))
    rel, gt = sc.fixture_inputs()
    assert str(g["inputs_sha256"]) == sc.checksum([rel, gt])
    seg = segment(torch.from_numpy(rel).cuda(), torch.from_numpy(gt).cuda(), strategy=strategy)
    check_rules(seg, torch.from_numpy(gt), torch.from_numpy(g["blended"]), torch.from_numpy(g[f"score_{strategy}"]),
                float(g["blended_f32_err"]), float(g[f"score_{strategy}_f32_err"]), f"fixture {strategy}")
    # and, no pixel of the fixture being near the threshold, the reference's masks, counts and choice
    assert np.array_equal(seg.mask_raw.cpu().numpy(), g["mask_raw"] != 0)
    assert np.array_equal(seg.mask.cpu().numpy(), g["mask"] != 0)
    assert np.array_equal(seg.inter.cpu().numpy(), g["inter"]) and np.array_equal(seg.union.cpu().numpy(), g["union"])
    assert np.array_equal(seg.level.cpu().numpy(), g[f"level_{strategy}"])
    assert np.array_equal(seg.chosen_iou.cpu().numpy(), g[f"chosen_iou_{strategy}"])


def against_float64(rel, gt, what):
    """rel float32 CPU: the native path against the float64 fallback, the float32 fallback's error the yardstick."""
    for strategy in STRATEGIES:
        s64 = segment(rel.double(), gt, strategy=strategy)
        s32 = segment(rel, gt, strategy=strategy)
        err_b = float((s32.blended.double() - s64.blended).abs().max())
        err_s = float((s32.score.double() - s64.score).abs().max())
        seg = segment(rel.cuda(), gt.cuda(), strategy=strategy)
        check_rules(seg, gt, s64.blended, s64.score, err_b, err_s, f"{what} {strategy}")


@pytest.mark.parametrize("H,W", [(70, 131), (97, 150)])
def test_unquantised_maps(H, W):
    rel, gt = sc.maps(3, 5, H, W, 2000 + H)
    against_float64(torch.from_numpy(rel), torch.from_numpy(gt), f"{H}x{W}")


def test_end_to_end_from_the_renderer():
    """render() -> relevancy(layout="chw") -> segment(), all on the GPU; the yardstick is the float64
    fallback on the relevancy maps copied to the host."""
    from helpers import small_case
    from lsr_testutil import run_native
    sc_, cam = small_case(P=1500, W=64, H=48, C=3, seed=3)
    _, lang, _, _, _ = run_native(sc_, cam)
    ws, bs = qc.decoder_arrays(qc.FIXTURE_DIMS, 1000)
    pix = lang.detach().cpu().permute(1, 2, 0).reshape(-1, 3).numpy()
    e = torch.from_numpy(qc.phrase_embeddings(ws, bs, pix, 9, 1001)).cuda()
    dec = LanguageDecoder.from_state_dict(qc.state_dict(ws, bs, torch)).to("cuda")
    rel = relevancy(lang, dec, e[:5], e[5:], layout="chw")
    assert rel.shape == (5, 48, 64) and rel.is_cuda
    gt = torch.from_numpy(sc.maps(1, 5, 48, 64, 77)[1])
    seg = segment(rel, gt.cuda())
    assert seg.blended.shape == (5, 48, 64) and seg.score.shape == (5,) and seg.level.tolist() == [0] * 5
    against_float64(rel.cpu(), gt, "renderer")


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_outputs_stay_inside_their_buffers(strategy):
    """Every output is a view into a larger buffer pre-filled with a sentinel, at 33 x 65 with 7 maps:
    the bytes outside are intact and the inside is what the Python surface returns."""
    H, W, M, PAD = 33, 65, 7, 4096
    rel, gt = quantised(H, W, 1, M)
    rel, gt = rel.cuda(), gt.cuda()
    want = segment(rel, gt, strategy=strategy)
    lib = _lib.load()

    def padded(n, dtype, sentinel):
        return torch.full((PAD + n + PAD,), sentinel, dtype=dtype, device="cuda")

    bufs = {"blended": padded(M * H * W, torch.float32, -77.0), "mask_raw": padded(M * H * W, torch.uint8, 0xAB),
            "mask": padded(M * H * W, torch.uint8, 0xAB), "score": padded(M, torch.float32, -77.0),
            "inter": padded(M, torch.int64, -77), "union": padded(M, torch.int64, -77)}
    sentinels = {k: v[0].item() for k, v in bufs.items()}
    n_ws = lib.lsr_segment_workspace_bytes(M, H, W)
    ws = padded(n_ws, torch.uint8, 0xAB)
    p = {k: v[PAD:].data_ptr() for k, v in bufs.items()}
    _lib.check(lib.lsr_segment(M, H, W, rel.data_ptr(), 29, 0.4, _lib.SEGMENT_STRATEGIES[strategy], gt.data_ptr(), M,
                               p["blended"], p["mask_raw"], p["mask"], p["score"], p["inter"], p["union"],
                               ws[PAD:].data_ptr(), torch.cuda.current_stream().cuda_stream), "lsr_segment")
    torch.cuda.synchronize()
    for k, buf in bufs.items():
        n = buf.numel() - 2 * PAD
        assert bool((buf[:PAD] == sentinels[k]).all()) and bool((buf[PAD + n:] == sentinels[k]).all()), k
        inside = buf[PAD:PAD + n]
        w = getattr(want, k).reshape(-1)
        assert torch.equal(inside, w.to(inside.dtype) if w.dtype == torch.bool else w), k
    assert bool((ws[:PAD] == 0xAB).all()) and bool((ws[PAD + n_ws:] == 0xAB).all())


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_repeats_bit_for_bit(strategy):
    rel, gt = sc.maps(3, 5, 97, 150, 3000)
    rel, gt = torch.from_numpy(rel).cuda(), torch.from_numpy(gt).cuda()
    a, b = segment(rel, gt, strategy=strategy), segment(rel, gt, strategy=strategy)
    for f in FIELDS:
        assert same(getattr(a, f), getattr(b, f)), f


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_edge_maps(strategy):
    """A NaN pixel, a constant map and an empty annotation, exactly as the float32 CPU fallback."""
    rel, gt = quantised(37, 29)
    rel, gt = rel.clone(), gt.clone()
    rel[1, 0, 20, 11] = float("nan")                   # the level is chosen: NaN counts as greatest
    rel[:, 1] = 0.5                                    # empty masks, IoU 0, equal scores: level 0
    gt[2] = 0
    rel[:, 2] = 0.25                                   # an empty mask on an empty annotation: IoU NaN
    want = segment(rel, gt, strategy=strategy)
    got = segment(rel.cuda(), gt.cuda(), strategy=strategy)
    assert_same_segmentation(got, want, f"edge maps {strategy}")
    assert not got.mask_raw[1, 0].any() and not got.mask_raw[:, 1].any()
    assert bool(got.iou[:, 2].isnan().all()) and bool((got.iou[:, 1] == 0).all()) and got.level.tolist()[1:3] == [0, 0]
    if strategy == "point":
        assert bool(got.score[1, 0].isnan()) and got.level.tolist()[0] == 1
    else:
        assert float(got.score[1, 0]) == 0.0 and bool((got.score[:, 1] == 0).all())


def test_peak_memory_is_the_outputs_and_the_workspace():
    L, K, H, W = 3, 5, 97, 150
    rel, gt = quantised(H, W)
    rel, gt = rel.cuda(), gt.cuda()
    M = L * K
    outputs = M * H * W * (4 + 1 + 1) + M * (4 + 8 + 8 + 4) + K * (8 + 4) + K * H * W
    ws = _lib.load().lsr_segment_workspace_bytes(M, H, W)
    for strategy in STRATEGIES:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        seg = segment(rel, gt, strategy=strategy)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        assert seg.chosen_mask.shape == (K, H, W)
        assert rise <= outputs + ws + 64 * 1024, (rise, outputs, ws)


def test_fallback_dispatch(monkeypatch):
    rel, gt = quantised(33, 65)
    want = segment(rel.double(), gt)

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(language_query._lib, "load", no_library)
    s = segment(rel.double().cuda(), gt.cuda())        # float64 on the GPU: torch ops there
    assert s.blended.dtype == torch.float64 and s.blended.is_cuda
    assert float((s.blended.cpu() - want.blended).abs().max()) <= 1e-12 and torch.equal(s.mask.cpu(), want.mask)
    assert torch.equal(s.inter.cpu(), want.inter)
    assert torch.equal(segment(rel, gt).union, want.union)                # CPU float32
    with pytest.raises(ValueError, match="gt_masks is on cpu but rel is on cuda"):
        segment(rel.cuda(), gt)
    with pytest.raises(AssertionError, match="the library was reached"):
        segment(rel.cuda(), gt.cuda())
