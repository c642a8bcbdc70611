"""CPU checks of the time-sensitive query (4dlangsplat_amd/video_query.py, include/lsr_video.h): the torch
fallback against the reference's recorded results (tests/golden/video_query_golden.npz, written by
tests/golden/make_video_query_golden.py from the reference's own cal_avg_video_feature and
evaluate_video_feature), the smoothing's edge rule, the two threshold rules, and the C ABI's refusals,
which are decided before a device is touched."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import video_query_cases as vc
import video_query as vq
from diff_gaussian_rasterization import _lib
from language_query import LanguageDecoder


def decoder_of(ws, bs, dtype=torch.float32, device="cpu"):
    return LanguageDecoder.from_state_dict(vc.state_dict(ws, bs, torch)).to(dtype).to(device)


def t(a, dtype=None, device="cpu"):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(device)


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "video_query_golden.npz")))
    inp = vc.fixture_inputs()
    assert str(g["weights_sha256"]) == vc.checksum(inp["ws"] + inp["bs"])
    assert str(g["inputs_sha256"]) == vc.checksum([inp["latent"], inp["masks"], inp["queries"]])
    host = json.dumps([vc.eval_cases(), vc.smooth_cases(), vc.sequence_case()], sort_keys=True).encode()
    assert str(g["host_sha256"]) == vc.checksum([np.frombuffer(host, np.uint8)])
    for k in ("evaluate", "smooth", "sequence"):
        g[k] = json.loads(str(g[k]))
    return g, inp


# ---- masked_similarity, the torch fallback ------------------------------------------------------------------
def test_fallback_matches_the_reference_in_float64(golden):
    g, inp = golden
    dec = decoder_of(inp["ws"], inp["bs"], torch.float64)
    sims, counts = vq.masked_similarity(t(inp["latent"], torch.float64), t(inp["masks"]), dec,
                                        t(inp["queries"], torch.float64))
    assert sims.dtype == torch.float64 and counts.dtype == torch.int64
    assert counts.tolist() == g["counts"].tolist() and 40 <= int(counts.min()) and int(counts.max()) <= 150
    e = float((sims - torch.from_numpy(g["similarity"])).abs().max())
    print(f"float64 fallback against the reference: {e:.3g}")
    assert e <= 1e-12


def test_fallback_matches_the_reference_in_float32(golden):
    """Within twice the error the reference's own float32 run showed (two float32 runs, each that far off)."""
    g, inp = golden
    dec = decoder_of(inp["ws"], inp["bs"])
    sims, counts = vq.masked_similarity(t(inp["latent"]), t(inp["masks"]), dec, t(inp["queries"]))
    assert sims.dtype == torch.float32 and counts.tolist() == g["counts"].tolist()
    e = float((sims.double() - torch.from_numpy(g["similarity"])).abs().max())
    print(f"float32 fallback against the reference: {e:.3g} (float32 reference {float(g['similarity_f32_err']):.3g})")
    assert e <= 2 * float(g["similarity_f32_err"])


def test_fallback_layouts_masks_and_empty():
    ws, bs, rows, q = vc.case([6, 16, 48], 7 * 5, 3, 11)
    dec = decoder_of(ws, bs, torch.float64)
    lat = t(rows, torch.float64).reshape(7, 5, 6)
    m = torch.zeros(3, 7, 5, dtype=torch.int64)
    m[0, 1:4, 1:3] = 1
    m[0, 4:6] = 2                                               # a label that is not 1 does not count
    m[2, 6, 4] = 1
    qs = t(q, torch.float64)
    sims, counts = vq.masked_similarity(lat, m, dec, qs)
    assert counts.tolist() == [6, 0, 1] and bool(sims[1].isnan())
    chw, _ = vq.masked_similarity(lat.permute(2, 0, 1).contiguous(), m, dec, qs, layout="chw")
    assert torch.equal(chw[[0, 2]], sims[[0, 2]])
    as_bool, _ = vq.masked_similarity(lat, m == 1, dec, qs)
    assert torch.equal(as_bool[[0, 2]], sims[[0, 2]])
    # by hand: the one pixel of mask 2
    y = lat[6, 4]
    for i, (w, b) in enumerate(zip(dec.weights, dec.biases)):
        y = w @ (torch.relu(y) if i else y) + b
    want = (y @ qs[2]) / (y.norm() * qs[2].norm())
    assert abs(float(sims[2] - want)) <= 1e-14
    # row_cosines is the per-row quantity the means are taken of
    cos = vq.row_cosines(lat.reshape(-1, 6), dec, qs)
    assert cos.shape == (3, 35)
    assert abs(float(cos[0].reshape(7, 5)[1:4, 1:3].mean() - sims[0])) <= 1e-14
    with pytest.raises(ValueError, match="bool or integer"):
        vq.masked_similarity(lat, m.double(), dec, qs)
    with pytest.raises(ValueError, match="queries must be"):
        vq.masked_similarity(lat, m, dec, qs[:2])
    with pytest.raises(ValueError, match="channels"):
        vq.masked_similarity(lat[..., :5], m, dec, qs)


# ---- smoothing ----------------------------------------------------------------------------------------------
def test_smoothing_matches_the_recorded_values(golden):
    g, _ = golden
    cases = vc.smooth_cases()
    assert set(cases) == set(g["smooth"])
    for name, c in cases.items():
        got = vq.smooth_similarity(c["values"], c["coeffs"])
        assert got == g["smooth"][name], name
    # shorter than the window: every frame keeps its raw value
    for name in ("two_by_three", "four_by_five", "one_by_three"):
        assert g["smooth"][name] == cases[name]["values"]
    # the edge rule: raw at the ends (not a renormalised partial window), the full window inside
    v = cases["nine_by_five"]["values"]
    s = vq.smooth_similarity(v, vc.COEFFS[1])
    assert s[:2] == v[:2] and s[-2:] == v[-2:]
    assert s[2] == pytest.approx(sum(a * b for a, b in zip(v[0:5], vc.COEFFS[1])), abs=1e-15)
    partial = (0.8 * v[0] + 0.1 * v[1]) / 0.9
    assert vq.smooth_similarity(v, vc.COEFFS[0])[0] == v[0] != partial
    assert vq.smooth_similarity(torch.tensor(v), vc.COEFFS[0])[1:8] == pytest.approx(g["smooth"]["nine_by_three"][1:8],
                                                                                     abs=1e-6)
    with pytest.raises(ValueError, match="odd length"):
        vq.smooth_similarity(v, [0.5, 0.5])
    with pytest.raises(ValueError, match="sum to 1"):
        vq.smooth_similarity(v, [0.5, 0.5, 0.5])


# ---- evaluate_frames ----------------------------------------------------------------------------------------
def same_result(got, ref):
    assert got["labels"] == ref["label_list"] and got["predictions"] == ref["predict_list"]
    for mine, theirs in (("accuracy", "accuracy"), ("precision", "precision"), ("recall", "recall"),
                         ("viou", "average_iou")):
        assert got[mine] == ref[theirs], (mine, got[mine], ref[theirs])


def test_evaluate_frames_matches_the_recorded_results(golden):
    g, _ = golden
    cases = vc.eval_cases()
    assert set(cases) == set(g["evaluate"])
    for name, c in cases.items():
        same_result(vq.evaluate_frames(c["ids"], c["sims"], c["ious"], c["intervals"], c["thresh"]), g["evaluate"][name])
    r = g["evaluate"]["nothing_predicted_nothing_labelled"]
    assert r["average_iou"] == 0 and not any(r["label_list"]) and not any(r["predict_list"])
    r = g["evaluate"]["no_predictions"]
    assert r["precision"] == 0 and any(r["label_list"]) and not any(r["predict_list"])
    r = g["evaluate"]["interval_ends"]                          # ids 4, 5, 7, 9, 10 against [5, 9]: both ends inside
    assert r["label_list"] == [False, True, True, True, False]
    with pytest.raises(ValueError, match="no frames"):
        vq.evaluate_frames([], [], [], [[0, 1]], 0.5)
    with pytest.raises(ValueError, match="one entry per frame"):
        vq.evaluate_frames([1, 2], [0.5], [0.5, 0.5], [[0, 1]], 0.5)


# ---- the two threshold rules --------------------------------------------------------------------------------
def test_threshold_asymmetry_matches_the_recorded_sequence(golden):
    """The video similarities are thresholded at the mean of the unsmoothed list, the CLIP scores at the
    mean of the smoothed list (eval/eval.py:740, 760)."""
    g, _ = golden
    c = vc.sequence_case()
    assert c["ids"] != sorted(c["ids"])
    for name, coeffs in (("none", None), ("three", vc.COEFFS[0]), ("five", vc.COEFFS[1])):
        ref = g["sequence"][name]
        got = vq.evaluate_sequence(c["ids"], c["sims"], c["ious"], c["intervals"], coeffs=coeffs, clip_scores=c["clip"])
        assert got["frame_ids"] == sorted(c["ids"])
        assert got["video_thresh"] == ref["video_thresh"] and got["clip_thresh"] == ref["clip_thresh"]
        assert got["smoothed"] == ref["smoothed"] and got["clip_smoothed"] == ref["clip_smoothed"]
        same_result(got["video"], ref["video"])
        same_result(got["clip"], ref["clip"])
        assert [r[1] for r in got["table"]] == ref["smoothed"]
    got = vq.evaluate_sequence(c["ids"], c["sims"], c["ious"], c["intervals"], coeffs=vc.COEFFS[1], clip_scores=c["clip"])
    n = len(c["ids"])
    assert got["video_thresh"] == sum(c["sims"]) / n != sum(got["smoothed"]) / n
    assert got["clip_thresh"] == sum(got["clip_smoothed"]) / n != sum(c["clip"]) / n
    # the rule matters on this data: the symmetric alternatives predict other frames
    other_video = [s >= sum(got["smoothed"]) / n for s in got["smoothed"]]
    other_clip = [s >= sum(c["clip"]) / n for s in got["clip_smoothed"]]
    assert other_video != got["video"]["predictions"] or other_clip != got["clip"]["predictions"]


def test_time_sensitive_query_end_to_end_on_the_cpu(tmp_path):
    """Frames as tensors and as renders_npy files (one saved in (0, 1): mapped back by x * 2 - 1), given out
    of order: the per-frame similarities are masked_similarity's, the rest is evaluate_sequence."""
    ws, bs, rows, q = vc.case([6, 16, 32], 5 * 6 * 4, 1, 21)
    dec = decoder_of(ws, bs)
    frames = t(rows).reshape(5, 6, 4, 6)
    masks = torch.zeros(5, 6, 4, dtype=torch.uint8)
    masks[:, 1:5, 1:3] = 1
    masks[3] = 0                                                # an empty mask: NaN, never predicted
    ids, ious = [7, 3, 9, 4, 5], [0.5, 0.6, 0.7, 0.8, 0.9]
    paths = []
    for i in range(5):
        arr = frames[i].numpy()
        if i == 1:
            arr = (arr + 1) / 2 * 0.98 + 0.01                   # saved in (0, 1)
        p = str(tmp_path / f"{i:05d}.npy")
        np.save(p, arr)
        paths.append(p)
    given = [frames[0], paths[1], paths[2], frames[3], paths[4]]
    res = vq.time_sensitive_query(given, masks, ious, dec, t(q)[0], [[4, 7]], coeffs=vc.COEFFS[0], frame_ids=ids,
                                  clip_scores=[0.1, 0.2, 0.3, 0.4, 0.5])
    sims = []
    for i in range(5):
        x = frames[i]
        if i == 1:
            x = torch.from_numpy(np.load(paths[1])).float() * 2.0 - 1
        sims.append(float(vq.masked_similarity(x, masks[i:i + 1], dec, t(q))[0][0]))
    assert np.isnan(sims[3]) and res["counts"] == [8, 0, 8, 8, 8]
    want = vq.evaluate_sequence(ids, sims, ious, [[4, 7]], coeffs=vc.COEFFS[0], clip_scores=[0.1, 0.2, 0.3, 0.4, 0.5])
    assert res["frame_ids"] == [3, 4, 5, 7, 9]
    np.testing.assert_array_equal(res["similarity"], want["similarity"])
    assert res["clip"] == want["clip"] and res["clip_thresh"] == want["clip_thresh"]
    assert res["video"]["labels"] == [False, True, True, True, False]


# ---- the C ABI: refusals before the device is touched ------------------------------------------------------
FAKE = 64      # never dereferenced: every call below returns early


def struct_of(dims, pointers=True):
    s = _lib.Decoder()
    s.n_layers = len(dims) - 1
    for i, d in enumerate(dims[:9]):
        s.dims[i] = d
    for i in range(min(len(dims) - 1, 8)):
        s.weight[i] = s.bias[i] = FAKE if pointers else None
    return s


def test_abi_refusals_and_workspace_size():
    lib = _lib.load()
    err = lambda: lib.lsr_last_error().decode()
    ok = struct_of(vc.FULL_DIMS)
    need = lib.lsr_video_workspace_bytes(ctypes.byref(ok), 1000)
    assert need > 0

    def cosine(dec=ok, n_rows=1000, rows=FAKE, n_q=3, queries=FAKE, out=FAKE, ws=FAKE, ws_bytes=need):
        return lib.lsr_video_cosine(ctypes.byref(dec) if dec is not None else None, n_rows, rows, n_q, queries, out, ws,
                                    ws_bytes, None)

    for dims, text in (([6, 32, 4112], "layer width 4112"), ([6, 24, 64], "layer width 24"),
                       ([33, 32, 64], "c_in = dims[0]"), ([0, 32], "c_in = dims[0]"), ([6, 32, 0], "layer width 0")):
        bad = struct_of(dims)
        assert lib.lsr_video_workspace_bytes(ctypes.byref(bad), 10) == -1 and text in err(), (dims, err())
        assert cosine(dec=bad) == 1 and text in err(), (dims, err())
    for layers in (0, 9):
        bad = struct_of(vc.FULL_DIMS)
        bad.n_layers = layers
        assert cosine(dec=bad) == 1 and "n_layers" in err()
        assert lib.lsr_video_workspace_bytes(ctypes.byref(bad), 10) == -1
    for n_q in (0, 17, -1):
        assert cosine(n_q=n_q) == 1 and "n_q must be in [1, 16]" in err()
    assert cosine(n_rows=-1) == 1 and "n_rows must be >= 0" in err()
    assert lib.lsr_video_workspace_bytes(ctypes.byref(ok), -1) == -1
    assert lib.lsr_video_workspace_bytes(None, 10) == -1 and "null decoder" in err()
    assert cosine(dec=None) == 1 and "null decoder" in err()
    for kw in ("rows", "queries", "out", "ws"):
        assert cosine(**{kw: None}) == 1 and "are required" in err(), kw
    assert cosine(dec=struct_of(vc.FULL_DIMS, pointers=False)) == 1 and "missing weight or bias" in err()
    assert cosine(ws=FAKE + 4) == 1 and "16-byte aligned" in err()
    # a workspace one byte short, and the exact size with no rows (nothing is launched)
    assert cosine(ws_bytes=need - 1) == 1 and "are needed" in err()
    zero = lib.lsr_video_workspace_bytes(ctypes.byref(ok), 0)
    assert zero > 0 and cosine(n_rows=0, ws_bytes=zero) == 0
    assert cosine(n_rows=0, ws_bytes=zero - 1) == 1

    # the size grows with the rows and with the widths, and covers the two activation images
    sizes = [lib.lsr_video_workspace_bytes(ctypes.byref(ok), n) for n in (1, 127, 128, 129, 8192)]
    assert sizes == sorted(set(sizes))
    assert sizes[-1] >= 8192 * (2048 + 1024) * 4
    narrow, wide = struct_of([6, 32, 64, 128]), struct_of([6, 32, 2048, 128])
    assert lib.lsr_video_workspace_bytes(ctypes.byref(narrow), 512) < lib.lsr_video_workspace_bytes(ctypes.byref(wide), 512)
    short, long = struct_of([6, 32, 128]), struct_of([6, 32, 4096])
    assert lib.lsr_video_workspace_bytes(ctypes.byref(short), 512) < lib.lsr_video_workspace_bytes(ctypes.byref(long), 512)

    def seg_mean(n_rows=10, n_q=2, cos=FAKE, n_seg=2, offs=FAKE, sq=FAKE, mean=FAKE):
        return lib.lsr_video_segment_mean(n_rows, n_q, cos, n_seg, offs, sq, mean, None)

    for kw in ("cos", "offs", "sq", "mean"):
        assert seg_mean(**{kw: None}) == 1 and "are required" in err(), kw
    assert seg_mean(n_q=0) == 1 and seg_mean(n_q=17) == 1 and "n_q must be in [1, 16]" in err()
    assert seg_mean(n_rows=-1) == 1 and seg_mean(n_seg=-1) == 1
    assert seg_mean(n_seg=0) == 0                              # no segments: no launch
    assert _lib.VIDEO_ROW_TILE == vq.ROW_TILE == 128 and _lib.VIDEO_MAX_WIDTH == 4096 and _lib.VIDEO_MAX_QUERIES == 16


def test_constants_match_the_header():
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lsr_video.h")).read()
    import re
    defs = {k: int(v) for k, v in re.findall(r"#define (LSR_VIDEO_\w+) (\d+)", txt)}
    assert defs == {"LSR_VIDEO_API_VERSION": _lib.VIDEO_API_VERSION, "LSR_VIDEO_MAX_WIDTH": _lib.VIDEO_MAX_WIDTH,
                    "LSR_VIDEO_MAX_QUERIES": _lib.VIDEO_MAX_QUERIES, "LSR_VIDEO_ROW_TILE": _lib.VIDEO_ROW_TILE,
                    "LSR_VIDEO_COL_TILE": _lib.VIDEO_COL_TILE}


def test_callers_of_another_header_version_are_refused():
    """lsr_video_require_api: until a caller has declared its lsr_video.h version every entry point refuses;
    a mismatched declaration is refused too.  Fresh process: the handshake is per process."""
    import subprocess
    import sys
    code = f"""
import ctypes
L = ctypes.CDLL({_lib.LIB_PATH!r})
L.lsr_last_error.restype = ctypes.c_char_p
L.lsr_video_workspace_bytes.restype = ctypes.c_int64
L.lsr_video_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int64]
assert L.lsr_video_workspace_bytes(None, 1) == -1 and b"lsr_video_require_api" in L.lsr_last_error()
assert L.lsr_video_require_api(2) == 1 and b"mismatch" in L.lsr_last_error()
assert L.lsr_video_workspace_bytes(None, 1) == -1 and b"lsr_video_require_api" in L.lsr_last_error()
assert L.lsr_video_segment_mean(ctypes.c_int64(1), 1, None, 0, None, None, None, None) == 1
assert b"lsr_video_require_api" in L.lsr_last_error()
assert L.lsr_video_require_api(1) == 0
assert L.lsr_video_workspace_bytes(None, 1) == -1 and b"null decoder" in L.lsr_last_error()
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr
