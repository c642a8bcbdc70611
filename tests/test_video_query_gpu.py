"""GPU checks of the time-sensitive query's native path (csrc/video_query.hip through video_query.py).

Tolerance rule, that of tests/test_query_gpu.py: against the float64 value the native result's max abs error
may be at most TOL = 8 times the float32 reference's error against that same float64 value.  For the
fixture the float32 error is the one its generator measured on the reference's own code
(cal_avg_video_feature in float32 against float64); for other shapes it is measured here, the torch fallback
in float32 against the fallback in float64, on the CPU.  A wrong lane map or a lost tile is orders of
magnitude outside it.

The full-width decoder (6 -> 32 -> ... -> 4096, 45 MB) appears in three tests through one module-scoped
fixture; everything else uses narrow decoders that still cross every boundary of the kernel: a K tail (6,
48, 528 are no multiples of the 32-wide k block), column tiles that are not full (48, 528, 1040, 2064 are no
multiples of 128), more than one column tile, and row counts around the row tile."""
import ctypes
import os

import numpy as np
import pytest
import torch

import video_query_cases as vc
import video_query as vq
from diff_gaussian_rasterization import _lib
from language_query import LanguageDecoder

pytestmark = pytest.mark.gpu
TOL = 8.0
T = vq.ROW_TILE
NARROW = [6, 48, 528, 1040]
TALL = [3, 16, 2064]


def decoder_of(ws, bs, dtype=torch.float32, device="cpu"):
    return LanguageDecoder.from_state_dict(vc.state_dict(ws, bs, torch)).to(dtype).to(device)


def t(a, dtype=None, device="cpu"):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(device)


def err(a, ref):
    return float((a.detach().cpu().double() - ref).abs().max())


def check_case(dims, n_rows, n_q, seed, what):
    """Native per-row cosines of [n_rows, c_in] latents against the float64 fallback, within the rule."""
    ws, bs, rows, q = vc.case(dims, n_rows, n_q, seed)
    c64 = vq.row_cosines(t(rows, torch.float64), decoder_of(ws, bs, torch.float64), t(q, torch.float64))
    ref = err(vq.row_cosines(t(rows), decoder_of(ws, bs), t(q)), c64)
    cos = vq.row_cosines(t(rows, device="cuda"), decoder_of(ws, bs, device="cuda"), t(q, device="cuda"))
    assert cos.shape == (n_q, n_rows) and cos.dtype == torch.float32 and cos.is_cuda
    e = err(cos, c64)
    print(f"{what}: cosine error {e:.3g} (float32 reference {ref:.3g}); range [{float(c64.min()):.3f}, "
          f"{float(c64.max()):.3f}]")
    assert e <= TOL * ref
    return cos


@pytest.fixture(scope="module")
def full(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "video_query_golden.npz")))
    inp = vc.fixture_inputs()
    assert str(g["weights_sha256"]) == vc.checksum(inp["ws"] + inp["bs"])
    assert str(g["inputs_sha256"]) == vc.checksum([inp["latent"], inp["masks"], inp["queries"]])
    dec = decoder_of(inp["ws"], inp["bs"], device="cuda")
    assert vq.native_ok(dec) and dec.dims == vc.FULL_DIMS
    return g, inp, dec


@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_fixture_parity(full, layout):
    g, inp, dec = full
    lat = t(inp["latent"], device="cuda")                      # [H, W, 6] as loaded from npy
    masks, q = t(inp["masks"], device="cuda"), t(inp["queries"], device="cuda")
    x = lat if layout == "hwc" else lat.permute(2, 0, 1).contiguous()
    sims, counts = vq.masked_similarity(x, masks, dec, q, layout=layout)
    assert sims.shape == (3,) and sims.dtype == torch.float32 and sims.is_cuda
    assert counts.tolist() == g["counts"].tolist()
    e = err(sims, torch.from_numpy(g["similarity"]))
    print(f"{layout}: similarity error {e:.3g} (float32 reference {float(g['similarity_f32_err']):.3g}); "
          f"similarities {sims.tolist()}")
    assert e <= TOL * float(g["similarity_f32_err"])
    if layout == "chw":                                        # a permuted view (no copy) gives the same bits
        view, _ = vq.masked_similarity(lat.permute(2, 0, 1), masks, dec, q, layout="chw")
        assert not lat.permute(2, 0, 1).is_contiguous() and torch.equal(view, sims)
        hwc, _ = vq.masked_similarity(lat, masks, dec, q)
        assert torch.equal(hwc, sims)


def test_full_width_bits(full):
    """At the full width: two calls are equal, 64-row chunks equal the unchunked call, and a row computed
    alone equals the same row inside the larger call."""
    g, inp, dec = full
    lat, q = t(inp["latent"], device="cuda"), t(inp["queries"], device="cuda")
    rows = lat.reshape(-1, 6)[:T + 37].contiguous()
    a = vq.row_cosines(rows, dec, q)
    assert torch.equal(a, vq.row_cosines(rows, dec, q))
    assert torch.equal(a, vq.row_cosines(rows, dec, q, chunk_rows=64))
    for r in (0, T - 1, T + 36):
        assert torch.equal(vq.row_cosines(rows[r:r + 1].contiguous(), dec, q), a[:, r:r + 1])
    masks = t(inp["masks"], device="cuda")
    s, _ = vq.masked_similarity(lat, masks, dec, q)
    s64, _ = vq.masked_similarity(lat, masks, dec, q, chunk_rows=64)
    assert torch.equal(s, s64)


@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 1])
def test_sweep_row_counts(n_rows):
    check_case(NARROW, n_rows, 4, 100 + n_rows, f"n_rows {n_rows}")


@pytest.mark.parametrize("widths", [[16], [4096], [48, 528], [1040, 16], [32] * 8], ids=lambda w: "-".join(map(str, w)))
def test_sweep_widths(widths):
    check_case([6] + widths, T + 1, 4, 200 + len(widths) + widths[0], f"decoder {widths}")


@pytest.mark.parametrize("c_in", [1, 3, 6, 32])
def test_sweep_input_channels(c_in):
    check_case([c_in] + NARROW[1:], T + 1, 4, 300 + c_in, f"c_in {c_in}")


@pytest.mark.parametrize("n_q", [1, 2, 8, 16])
def test_sweep_query_counts(n_q):
    check_case(TALL, T + 1, n_q, 400 + n_q, f"n_q {n_q}")


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def test_segments():
    """lsr_video_segment_mean on native cosines: an empty segment, a one-row one, boundaries at T - 1, T and
    T + 1, seg_query picking different queries.  Each mean lies within one float32 ulp of the float64 mean
    of the per-row cosines."""
    n = 2 * T + 40
    ws, bs, rows, q = vc.case(TALL, n, 3, 500)
    dec = decoder_of(ws, bs, device="cuda")
    cos = vq.row_cosines(t(rows, device="cuda"), dec, t(q, device="cuda"))
    offs = [0, 0, 1, T - 1, T, T + 1, n]
    sq = [0, 1, 2, 0, 1, 2]
    mean = torch.full((len(sq) + 2,), -77.0, device="cuda")
    lib = _lib.load()
    # named, so that both arrays stay allocated until the kernel has read them
    offs_d = torch.tensor(offs, dtype=torch.int64, device="cuda")
    sq_d = torch.tensor(sq, dtype=torch.int32, device="cuda")
    assert offs_d.numel() == len(sq) + 1 and int(offs_d.max()) <= cos.shape[1] and int(sq_d.max()) < cos.shape[0]
    _lib.check(lib.lsr_video_segment_mean(n, 3, cos.data_ptr(), len(sq), offs_d.data_ptr(), sq_d.data_ptr(),
                                          mean[1:].data_ptr(), torch.cuda.current_stream().cuda_stream), "segment mean")
    torch.cuda.synchronize()
    got = mean.cpu()
    assert got[0] == -77.0 and got[-1] == -77.0                # the neighbours of the output are intact
    assert bool(got[1].isnan())
    host = cos.cpu().double()
    for s in range(1, len(sq)):
        want = float(host[sq[s], offs[s]:offs[s + 1]].mean())
        assert abs(float(got[1 + s]) - want) <= ulp32(want), (s, float(got[1 + s]), want)
    assert float(got[2]) == float(cos[1, 0])                   # a one-row segment is that row's cosine


def test_masked_similarity_segments_and_labels():
    """Through the Python surface: masks whose rows end at T - 1, T and T + 1 of the gathered rows, an empty
    mask (NaN, count 0), repeated and distinct queries; labels 0 / 1 / 2 where only == 1 counts."""
    H, W = 20, 20
    ws, bs, rows, q = vc.case(NARROW, H * W, 3, 600)
    dec = decoder_of(ws, bs, device="cuda")
    lat = t(rows, device="cuda").reshape(H, W, 6)
    flat = torch.zeros(5, H * W, dtype=torch.uint8, device="cuda")
    flat[0, :T - 1] = 1
    flat[1, T - 1] = 1
    flat[2, T] = 1
    flat[4, T + 1:] = 1                                         # mask 3 stays empty
    flat[0, T + 5:T + 50] = 2                                   # other labels do not count
    flat[3, 7:90] = 2
    masks = flat.reshape(5, H, W)
    qs = t(q, device="cuda")[[0, 1, 0, 1, 2]]
    sims, counts = vq.masked_similarity(lat, masks, dec, qs)
    assert counts.tolist() == [T - 1, 1, 1, 0, H * W - T - 1]
    assert bool(sims[3].isnan())
    cos = vq.row_cosines(lat.reshape(-1, 6), dec, t(q, device="cuda")).cpu().double()
    for k, lo, hi, j in [(0, 0, T - 1, 0), (1, T - 1, T, 1), (2, T, T + 1, 0), (4, T + 1, H * W, 2)]:
        want = float(cos[j, lo:hi].mean())
        assert abs(float(sims[k]) - want) <= ulp32(want), (k, float(sims[k]), want)
    as_bool, c2 = vq.masked_similarity(lat, masks == 1, dec, qs)
    assert torch.equal(c2, counts) and torch.equal(as_bool[[0, 1, 2, 4]], sims[[0, 1, 2, 4]])
    # against the float64 fallback on the CPU, within the rule
    d64 = decoder_of(ws, bs, torch.float64)
    s64, _ = vq.masked_similarity(lat.cpu().double(), masks.cpu(), d64, qs.cpu().double())
    s32, _ = vq.masked_similarity(lat.cpu(), masks.cpu(), decoder_of(ws, bs), qs.cpu())
    keep = [0, 1, 2, 4]
    ref, e = err(s32[keep], s64[keep]), err(sims[keep], s64[keep])
    print(f"masked means: error {e:.3g} (float32 reference {ref:.3g})")
    assert e <= TOL * ref


def test_more_than_16_distinct_queries_take_several_launches():
    H, W, K = 12, 10, 20
    ws, bs, rows, q = vc.case(TALL, H * W, K, 700)
    dec = decoder_of(ws, bs, device="cuda")
    lat = t(rows, device="cuda").reshape(H, W, 3)
    masks = (torch.arange(H * W, device="cuda")[None] % K == torch.arange(K, device="cuda")[:, None]).reshape(K, H, W)
    qs = t(q, device="cuda")
    sims, counts = vq.masked_similarity(lat, masks, dec, qs)
    assert counts.tolist() == [H * W // K] * K
    for k in (0, 15, 16, 19):
        one, _ = vq.masked_similarity(lat, masks[k:k + 1], dec, qs[k:k + 1])
        assert torch.equal(one[0], sims[k])


def test_bits_repeat_rows_alone_and_chunks():
    ws, bs, rows, q = vc.case(NARROW, 2 * T + 1, 4, 800)
    dec = decoder_of(ws, bs, device="cuda")
    x, qs = t(rows, device="cuda"), t(q, device="cuda")
    a = vq.row_cosines(x, dec, qs)
    assert torch.equal(a, vq.row_cosines(x, dec, qs))
    assert torch.equal(a, vq.row_cosines(x, dec, qs, chunk_rows=64))
    assert torch.equal(a, vq.row_cosines(x, dec, qs, chunk_rows=T + 1))
    for r in (0, 17, T - 1, T, 2 * T):
        assert torch.equal(vq.row_cosines(x[r:r + 1].contiguous(), dec, qs), a[:, r:r + 1])
    lat = x[:16 * 16].reshape(16, 16, 6)
    masks = torch.zeros(2, 16, 16, dtype=torch.bool, device="cuda")
    masks[0, 2:14, 1:15] = True
    masks[1, ::2] = True
    s, _ = vq.masked_similarity(lat, masks, dec, qs[:2])
    s64, _ = vq.masked_similarity(lat, masks, dec, qs[:2], chunk_rows=64)
    assert torch.equal(s, s64) and torch.equal(s, vq.masked_similarity(lat, masks, dec, qs[:2])[0])


def test_outputs_and_workspace_stay_inside_their_buffers():
    """cosine and the workspace are views into larger buffers pre-filled with a sentinel, at n_rows = T + 1
    and n_q = 3: every sentinel outside them is intact, and the inside is what the Python surface returns."""
    n, n_q, PAD, SENT = T + 1, 3, 4096, -77.0
    ws_, bs, rows, q = vc.case(NARROW, n, n_q, 900)
    dec = decoder_of(ws_, bs, device="cuda")
    x, qs = t(rows, device="cuda"), t(q, device="cuda")
    qn = (qs.double() / qs.double().norm(dim=-1, keepdim=True)).float().contiguous()
    lib, s = _lib.load(), dec._struct()
    need = lib.lsr_video_workspace_bytes(ctypes.byref(s), n)
    assert need > 0 and need % 16 == 0
    out = torch.full((PAD + n_q * n + PAD,), SENT, dtype=torch.float32, device="cuda")
    work = torch.full((PAD + need // 4 + PAD,), SENT, dtype=torch.float32, device="cuda")
    _lib.check(lib.lsr_video_cosine(ctypes.byref(s), n, x.data_ptr(), n_q, qn.data_ptr(), out[PAD:].data_ptr(),
                                    work[PAD:].data_ptr(), need, torch.cuda.current_stream().cuda_stream), "cosine")
    torch.cuda.synchronize()
    assert bool((out[:PAD] == SENT).all()) and bool((out[PAD + n_q * n:] == SENT).all())
    assert bool((work[:PAD] == SENT).all()) and bool((work[PAD + need // 4:] == SENT).all())
    assert torch.equal(out[PAD:PAD + n_q * n].view(n_q, n), vq.row_cosines(x, dec, qs))


def test_zero_vector_gives_nan_as_the_reference():
    """No epsilon: a row that decodes to the zero vector is 0 / 0."""
    w, b = np.zeros((16, 3), np.float32), np.zeros(16, np.float32)
    w[:, 0] = 1.0
    dec = decoder_of([w], [b], device="cuda")
    x = torch.tensor([[0.0, 1.0, 1.0], [0.5, 0.0, 0.0]], device="cuda")
    cos = vq.row_cosines(x, dec, torch.ones(1, 16, device="cuda"))
    assert bool(cos[0, 0].isnan()) and float(cos[0, 1]) == 1.0


def test_fallback_dispatch_and_zero_rows(monkeypatch):
    """CPU or float64 inputs and a width-24 decoder take the torch fallback and agree with it; all-empty
    masks launch nothing and give NaN; none of these reaches the library."""
    ws, bs, rows, q = vc.case(NARROW, 8 * 8, 2, 1000)
    dg = decoder_of(ws, bs, device="cuda")
    lat = t(rows).reshape(8, 8, 6)
    masks = torch.zeros(2, 8, 8, dtype=torch.uint8)
    masks[0, 1:6, 2:7] = 1
    masks[1, 4:, :] = 1
    d64 = decoder_of(ws, bs, torch.float64)
    ref, counts = vq.masked_similarity(lat.double(), masks, d64, t(q, torch.float64))
    native, c_native = vq.masked_similarity(lat.cuda(), masks.cuda(), dg, t(q, device="cuda"))
    assert torch.equal(c_native.cpu(), counts) and err(native, ref) <= 1e-5

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(vq._lib, "load", no_library)
    # float64 on the GPU: the fallback in float64 (float32 weights upcast)
    s, c = vq.masked_similarity(lat.double().cuda(), masks.cuda(), dg, t(q, torch.float64, "cuda"))
    assert s.dtype == torch.float64 and s.is_cuda and torch.equal(c.cpu(), counts) and err(s, ref) <= 1e-5
    # everything on the CPU
    s, _ = vq.masked_similarity(lat, masks, decoder_of(ws, bs), t(q))
    assert s.dtype == torch.float32 and not s.is_cuda and err(s, ref) <= 1e-5
    # a CPU latent with CUDA weights
    with pytest.raises(ValueError, match="the decoder's weights are on cuda"):
        vq.masked_similarity(lat, masks, dg, t(q))
    # a width the kernel does not take: torch ops in float32 on the GPU
    ws2, bs2, rows2, q2 = vc.case([6, 24, 512], 8 * 8, 2, 1001)
    d2 = decoder_of(ws2, bs2, device="cuda")
    assert not vq.native_ok(d2) and vq.native_ok(dg)
    s2, _ = vq.masked_similarity(t(rows2, device="cuda").reshape(8, 8, 6), masks.cuda(), d2, t(q2, device="cuda"))
    ref2, _ = vq.masked_similarity(t(rows2, torch.float64).reshape(8, 8, 6), masks, decoder_of(ws2, bs2, torch.float64),
                                   t(q2, torch.float64))
    assert s2.dtype == torch.float32 and s2.is_cuda and err(s2, ref2) <= 1e-4
    # zero rows on the native path: nothing is launched, the means are NaN
    s0, c0 = vq.masked_similarity(lat.cuda(), torch.zeros(2, 8, 8, dtype=torch.uint8, device="cuda"), dg,
                                  t(q, device="cuda"))
    assert s0.dtype == torch.float32 and bool(s0.isnan().all()) and c0.tolist() == [0, 0]
    # and the native path does reach the library
    with pytest.raises(AssertionError, match="the library was reached"):
        vq.masked_similarity(lat.cuda(), masks.cuda(), dg, t(q, device="cuda"))


def test_time_sensitive_query_on_the_gpu():
    """The whole phrase on the device: the per-frame similarities are the native ones, the metrics those of
    evaluate_sequence on them."""
    ws, bs, rows, q = vc.case(NARROW, 6 * 10 * 8, 1, 1100)
    dec = decoder_of(ws, bs, device="cuda")
    frames = t(rows, device="cuda").reshape(6, 10, 8, 6)
    masks = torch.zeros(6, 10, 8, dtype=torch.uint8, device="cuda")
    masks[:, 2:9, 1:7] = 1
    ids, ious = [4, 2, 9, 3, 7, 5], [0.5, 0.6, 0.7, 0.8, 0.9, 0.4]
    res = vq.time_sensitive_query(list(frames), list(masks), ious, dec, t(q, device="cuda")[0], [[3, 5]],
                                  coeffs=vc.COEFFS[0], frame_ids=ids)
    sims = [float(vq.masked_similarity(frames[i], masks[i:i + 1], dec, t(q, device="cuda"))[0][0]) for i in range(6)]
    want = vq.evaluate_sequence(ids, sims, ious, [[3, 5]], coeffs=vc.COEFFS[0])
    assert res["frame_ids"] == [2, 3, 4, 5, 7, 9] and res["similarity"] == want["similarity"]
    assert res["video"] == want["video"] and res["counts"] == [42] * 6
