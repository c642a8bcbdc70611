"""GPU checks of the fused open-vocabulary query (csrc/query.hip through language_query.py).

Tolerance rule: against the float64 value the native result's max abs error may be at most 8x the
float32 reference's error, for features and relevancy separately: the f32 MFMA is a k-ordered fmaf
chain and torch's CPU GEMM sums in blocks, so a few-fold difference is legitimate, while a lost term
or a wrong lane map is orders of magnitude larger.  For the fixture the float32 error is the one
its generator measured on the reference's own code; for other shapes it is measured here the same
way, the torch fallback in float32 against the fallback in float64."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import query_cases as qc
import language_query
from diff_gaussian_rasterization import _lib
from language_query import LanguageDecoder, relevancy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 8.0


def decoder_of(ws, bs, dtype=torch.float32, device="cpu"):
    return LanguageDecoder.from_state_dict(qc.state_dict(ws, bs, torch)).to(dtype).to(device)


def t(a, dtype=torch.float32, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)


def err(a, ref):
    return float((a.detach().cpu().double() - ref).abs().max())


def check_case(ws, bs, lat, pos, neg, what):
    """Native relevancy and decode of [N, c_in] latents against the float64 fallback, within the rule."""
    d64, d32 = decoder_of(ws, bs, torch.float64), decoder_of(ws, bs)
    x64 = t(lat, torch.float64)[:, None, :]                    # [N, 1, C]: an H x 1 image
    rel64 = relevancy(x64, d64, t(pos, torch.float64), t(neg, torch.float64))
    f64 = d64.decode(x64)
    rel_ref = err(relevancy(x64.float(), d32, t(pos), t(neg)), rel64)
    f_ref = err(d32.decode(x64.float()), f64)
    dg = d32.to("cuda")
    xg = x64.float().cuda()
    rel = relevancy(xg, dg, t(pos, device="cuda"), t(neg, device="cuda"))
    f = dg.decode(xg)
    assert rel.shape == rel64.shape and rel.dtype == torch.float32 and rel.is_cuda
    assert f.shape == f64.shape and f.dtype == torch.float32
    e_rel, e_f = err(rel, rel64), err(f, f64)
    print(f"{what}: relevancy error {e_rel:.3g} (float32 reference {rel_ref:.3g}), "
          f"features {e_f:.3g} (float32 reference {f_ref:.3g})")
    assert e_rel <= TOL * rel_ref and e_f <= TOL * f_ref
    assert float((f.norm(dim=-1) - 1).abs().max()) <= 1e-6


def test_mfma_f32_lane_maps(tmp_path):
    """v_mfma_f32_16x16x4_f32 operand and accumulator lane maps, the kernel's k-block order and the
    accumulator-as-operand step, on exact integers."""
    src = os.path.join(ROOT, "tests", "kernels", "t_mfma_f32.hip")
    exe = str(tmp_path / "t_mfma_f32")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-o", exe, src], check=True)
    r = subprocess.run(["timeout", "-k", "5", "60", exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "query_golden.npz")))
    inp = qc.fixture_inputs()
    assert str(g["weights_sha256"]) == qc.checksum(inp["ws"] + inp["bs"])
    assert str(g["inputs_sha256"]) == qc.checksum([inp["latent"], inp["pos"], inp["neg"]])
    return g, inp


@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_fixture_parity(golden, layout):
    g, inp = golden
    dec = decoder_of(inp["ws"], inp["bs"], device="cuda")
    lat = t(inp["latent"], device="cuda")                      # [L, H, W, 3] as loaded from npy
    x = lat if layout == "hwc" else lat.permute(0, 3, 1, 2).contiguous()   # [L, 3, H, W]
    rel = relevancy(x, dec, t(inp["pos"], device="cuda"), t(inp["neg"], device="cuda"), layout=layout)
    assert rel.shape == (3, 5, 37, 29)
    e_rel = err(rel, torch.from_numpy(g["relevancy"]))
    f = dec.decode(lat)
    assert f.shape == (3, 37, 29, 512)
    e_f = err(f.reshape(-1, 512)[torch.from_numpy(inp["samples"]).cuda()], torch.from_numpy(g["features"]))
    print(f"{layout}: relevancy error {e_rel:.3g} (float32 reference {float(g['relevancy_f32_err']):.3g}), "
          f"features {e_f:.3g} (float32 reference {float(g['features_f32_err']):.3g})")
    assert e_rel <= TOL * float(g["relevancy_f32_err"]) and e_f <= TOL * float(g["features_f32_err"])
    assert float((f.norm(dim=-1) - 1).abs().max()) <= 1e-6
    # a permuted view (no copy) and one level alone give the same bits
    if layout == "chw":
        view = relevancy(lat.permute(0, 3, 1, 2), dec, t(inp["pos"], device="cuda"), t(inp["neg"], device="cuda"),
                         layout="chw")
        assert torch.equal(view, rel)
    one = relevancy(x[2], dec, t(inp["pos"], device="cuda"), t(inp["neg"], device="cuda"), layout=layout)
    assert one.shape == (5, 37, 29) and torch.equal(one, rel[2])


@pytest.mark.parametrize("n_pix", [1, 15, 16, 17, 63, 64, 65, 127, 129, 1073])
def test_sweep_pixel_counts(n_pix):
    check_case(*qc.case(qc.FIXTURE_DIMS, n_pix, 6, 4, 100 + n_pix), f"n_pix {n_pix}")


@pytest.mark.parametrize("n_pos,n_neg", [(1, 1), (1, 4), (12, 4), (13, 4), (60, 4)])
def test_sweep_phrase_counts(n_pos, n_neg):
    check_case(*qc.case(qc.FIXTURE_DIMS, 129, n_pos, n_neg, 200 + n_pos + n_neg), f"phrases {n_pos}+{n_neg}")


@pytest.mark.parametrize("c_in", [1, 3, 6, 32])
def test_sweep_input_channels(c_in):
    check_case(*qc.case([c_in] + qc.DEFAULT_DECODER, 129, 6, 4, 300 + c_in), f"c_in {c_in}")


@pytest.mark.parametrize("widths", [[512], [64, 512], qc.DEFAULT_DECODER, [32, 32, 32, 32, 32, 32, 32, 64], [512, 512]],
                         ids=lambda w: "-".join(map(str, w)))
def test_sweep_decoders(widths):
    check_case(*qc.case([3] + widths, 129, 6, 4, 400 + len(widths) + widths[0]), f"decoder {widths}")


def test_more_than_60_positives_are_chunked():
    ws, bs, lat, pos, neg = qc.case(qc.FIXTURE_DIMS, 129, 75, 4, 500)
    d64 = decoder_of(ws, bs, torch.float64)
    x64 = t(lat, torch.float64)[None]                          # [1, 129, 3]
    rel64 = relevancy(x64, d64, t(pos, torch.float64), t(neg, torch.float64))
    ref = err(relevancy(x64.float(), decoder_of(ws, bs), t(pos), t(neg)), rel64)
    rel = relevancy(x64.float().cuda(), decoder_of(ws, bs, device="cuda"), t(pos, device="cuda"), t(neg, device="cuda"))
    assert rel.shape == (75, 1, 129)
    e = err(rel, rel64)
    print(f"75 positives: relevancy error {e:.3g} (float32 reference {ref:.3g})")
    assert e <= TOL * ref


def test_outputs_stay_inside_their_buffers():
    """The outputs are views into larger buffers pre-filled with a sentinel, at n_pix = 65 and
    n_pos = 13: every sentinel outside [n_pos, n_pix] (and decode's [n_pix, d_out]) is intact, and the
    inside is what the Python surface returns."""
    n_pix, n_pos, n_neg, PAD, SENT = 65, 13, 4, 1024, -77.0
    ws, bs, lat, pos, neg = qc.case(qc.FIXTURE_DIMS, n_pix, n_pos, n_neg, 600)
    dec = decoder_of(ws, bs, device="cuda")
    x, pg, ng = t(lat, device="cuda"), t(pos, device="cuda"), t(neg, device="cuda")
    lib, s = _lib.load(), dec._struct()
    stream = torch.cuda.current_stream().cuda_stream
    for n, call, want in (
            (n_pos * n_pix,
             lambda out: lib.lsr_query_relevancy(ctypes.byref(s), n_pix, x.data_ptr(), 3, 1, n_pos, pg.data_ptr(), n_neg,
                                                 ng.data_ptr(), 10.0, out, stream),
             relevancy(x[:, None, :], dec, pg, ng).reshape(-1)),
            (n_pix * 512,
             lambda out: lib.lsr_query_decode(ctypes.byref(s), n_pix, x.data_ptr(), 3, 1, out, stream),
             dec.decode(x).reshape(-1))):
        buf = torch.full((PAD + n + PAD,), SENT, dtype=torch.float32, device="cuda")
        _lib.check(call(buf[PAD:].data_ptr()), "query")
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all())
        assert torch.equal(buf[PAD:PAD + n], want)


def test_repeats_bit_for_bit():
    ws, bs, lat, pos, neg = qc.case(qc.FIXTURE_DIMS, 1073, 13, 4, 700)
    dec = decoder_of(ws, bs, device="cuda")
    x, pg, ng = t(lat, device="cuda")[None], t(pos, device="cuda"), t(neg, device="cuda")
    assert torch.equal(relevancy(x, dec, pg, ng), relevancy(x, dec, pg, ng))
    assert torch.equal(dec.decode(x), dec.decode(x))


def test_decode_indexes_past_2_31():
    """2^22 + 65 pixels x 512 features is more than 2^31 output elements (8.6 GB): the last block's rows
    land where they belong.  A pixel's arithmetic does not depend on its place in the image, so the
    first and last rows equal, bit for bit, the decode of those pixels alone."""
    n_pix = (1 << 22) + 65
    ws, bs = qc.decoder_arrays(qc.FIXTURE_DIMS, 950)
    dec = decoder_of(ws, bs, device="cuda")
    x = t(qc.latents((n_pix, 3), 951), device="cuda")
    f = dec.decode(x)
    assert f.shape == (n_pix, 512) and f.numel() > 2**31
    for rows in (slice(0, 70), slice(n_pix - 70, n_pix)):
        assert torch.equal(f[rows], dec.decode(x[rows].contiguous()))
    mid = slice((1 << 21) - 3, (1 << 21) + 67)
    assert torch.equal(f[mid], dec.decode(x[mid].contiguous()))


def test_zero_vector_gives_nan_as_the_reference():
    """No epsilon in the normalisation: a pixel that decodes to the zero vector is 0 / 0."""
    w, b = np.zeros((16, 3), np.float32), np.zeros(16, np.float32)
    w[:, 0] = 1.0
    dec = decoder_of([w], [b], device="cuda")
    x = torch.tensor([[0.0, 1.0, 1.0], [0.5, 0.0, 0.0]], device="cuda")[None]
    e = torch.full((2, 16), 0.25, device="cuda")
    rel, f = relevancy(x, dec, e[:1], e[1:]), dec.decode(x)
    assert bool(rel[0, 0, 0].isnan()) and bool(f[0, 0].isnan().all())
    assert float(rel[0, 0, 1]) == 0.5 and bool((f[0, 1] == 0.25).all())


def test_peak_memory_is_the_output():
    """At 128 x 128 pixels the full feature tensor would be 32 MiB; the fused call allocates its output."""
    ws, bs, lat, pos, neg = qc.case(qc.FIXTURE_DIMS, 128 * 128, 4, 4, 800)
    dec = decoder_of(ws, bs, device="cuda")
    x, pg, ng = t(lat, device="cuda").reshape(128, 128, 3), t(pos, device="cuda"), t(neg, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rel = relevancy(x, dec, pg, ng)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rel.shape == (4, 128, 128)
    assert rise <= rel.numel() * 4 + 64 * 1024, rise


def test_fallback_dispatch(monkeypatch):
    """Inputs the native path does not take fall back to torch ops or raise a clear error; none of
    them hands a pointer to the library."""
    ws, bs, lat, pos, neg = qc.case(qc.FIXTURE_DIMS, 33, 3, 2, 900)

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(language_query._lib, "load", no_library)
    dg = decoder_of(ws, bs, device="cuda")
    ref = relevancy(t(lat, torch.float64)[None], decoder_of(ws, bs, torch.float64), t(pos, torch.float64),
                    t(neg, torch.float64))
    # a float64 CUDA latent: the fallback, in float64 on the GPU
    rel = relevancy(t(lat, torch.float64, "cuda")[None], dg, t(pos, torch.float64, "cuda"), t(neg, torch.float64, "cuda"))
    assert rel.dtype == torch.float64 and rel.is_cuda and err(rel, ref) <= 1e-5   # float32 weights upcast
    f = dg.decode(t(lat, torch.float64, "cuda"))
    assert f.dtype == torch.float64 and f.shape == (33, 512)
    # a CPU latent with CUDA weights
    with pytest.raises(ValueError, match="the decoder's weights are on cuda"):
        relevancy(t(lat)[None], dg, t(pos), t(neg))
    with pytest.raises(ValueError, match="the decoder's weights are on cuda"):
        dg.decode(t(lat))
    with pytest.raises(ValueError, match="embeddings must be on the latent's device"):
        relevancy(t(lat, device="cuda")[None], dg, t(pos), t(neg))
    # a width the kernel does not take: torch ops in float32 on the GPU
    ws2, bs2, lat2, pos2, neg2 = qc.case([3, 24, 512], 33, 3, 2, 901)
    d2 = decoder_of(ws2, bs2, device="cuda")
    assert not d2.native_ok() and dg.native_ok()
    rel2 = relevancy(t(lat2, device="cuda")[None], d2, t(pos2, device="cuda"), t(neg2, device="cuda"))
    ref2 = relevancy(t(lat2, torch.float64)[None], decoder_of(ws2, bs2, torch.float64), t(pos2, torch.float64),
                     t(neg2, torch.float64))
    assert rel2.dtype == torch.float32 and err(rel2, ref2) <= 1e-4
    # and the native path does reach it
    with pytest.raises(AssertionError, match="the library was reached"):
        relevancy(t(lat, device="cuda")[None], dg, t(pos, device="cuda"), t(neg, device="cuda"))


def test_end_to_end_from_the_renderer():
    """render() -> language_feature_image [3, H, W] on the GPU -> relevancy(layout="chw"), no host
    round trip, against the float64 fallback on the same image copied to the host."""
    from helpers import small_case
    from lsr_testutil import run_native
    sc, cam = small_case(P=1500, W=64, H=48, C=3, seed=3)
    _, lang, _, _, _ = run_native(sc, cam)
    assert lang.shape == (3, 48, 64) and lang.is_cuda and lang.dtype == torch.float32
    ws, bs = qc.decoder_arrays(qc.FIXTURE_DIMS, 1000)
    host = lang.detach().cpu()
    pix = host.permute(1, 2, 0).reshape(-1, 3).numpy()
    e = qc.phrase_embeddings(ws, bs, pix, 9, 1001)
    pos, neg = e[:5], e[5:]
    rel = relevancy(lang, decoder_of(ws, bs, device="cuda"), t(pos, device="cuda"), t(neg, device="cuda"), layout="chw")
    rel64 = relevancy(host.double(), decoder_of(ws, bs, torch.float64), t(pos, torch.float64), t(neg, torch.float64),
                      layout="chw")
    ref = err(relevancy(host, decoder_of(ws, bs), t(pos), t(neg), layout="chw"), rel64)
    assert rel.shape == (5, 48, 64)
    e_rel = err(rel, rel64)
    print(f"end to end: relevancy error {e_rel:.3g} (float32 reference {ref:.3g}); range "
          f"[{float(rel64.min()):.3f}, {float(rel64.max()):.3f}]")
    assert e_rel <= TOL * ref
