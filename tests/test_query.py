"""CPU checks of the open-vocabulary query (language_query.py, include/lsr_query.h): the torch
fallback against the reference fixture (tests/golden/query_golden.npz, made by the reference's own
Autoencoder.decode and OpenCLIPNetwork.get_max_across), state-dict loading, the ABI's refusals
(decided before anything touches a device), the ctypes mirror of lsr_decoder, and query_frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import query_cases as qc
from diff_gaussian_rasterization import _lib
from language_query import LanguageDecoder, query_frames, relevancy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "query_golden.npz")))
    inp = qc.fixture_inputs()
    assert int(g["seed"]) == qc.FIXTURE_SEED and list(g["dims"]) == qc.FIXTURE_DIMS
    assert str(g["weights_sha256"]) == qc.checksum(inp["ws"] + inp["bs"]), "the regenerated weights differ"
    assert str(g["inputs_sha256"]) == qc.checksum([inp["latent"], inp["pos"], inp["neg"]])
    assert np.array_equal(g["samples"], inp["samples"])
    return g, inp


def decoder_of(inp, dtype):
    return LanguageDecoder.from_state_dict(qc.state_dict(inp["ws"], inp["bs"], torch)).to(dtype)


def test_fixture_spans_a_useful_range(golden):
    g, _ = golden
    assert g["relevancy"].shape == (3, 5, 37, 29) and g["features"].shape == (64, 512)
    assert g["relevancy"].min() < 0.1 and g["relevancy"].max() > 0.9
    assert 0 < g["features_f32_err"] < 1e-6 and 0 < g["relevancy_f32_err"] < 1e-5


def test_fallback_float64_reproduces_the_reference(golden):
    g, inp = golden
    dec = decoder_of(inp, torch.float64)
    lat = torch.from_numpy(inp["latent"]).double()
    rel = relevancy(lat, dec, torch.from_numpy(inp["pos"]).double(), torch.from_numpy(inp["neg"]).double())
    assert rel.dtype == torch.float64 and rel.shape == (3, 5, 37, 29)
    assert np.abs(rel.numpy() - g["relevancy"]).max() <= 1e-12
    f = dec.decode(lat).reshape(-1, 512)[torch.from_numpy(inp["samples"])]
    assert np.abs(f.numpy() - g["features"]).max() <= 1e-12
    # the same data channel-first, and one level alone
    rel_chw = relevancy(lat.permute(0, 3, 1, 2), dec, torch.from_numpy(inp["pos"]).double(),
                        torch.from_numpy(inp["neg"]).double(), layout="chw")
    assert torch.equal(rel_chw, rel)
    one = relevancy(lat[1], dec, torch.from_numpy(inp["pos"]).double(), torch.from_numpy(inp["neg"]).double())
    assert one.shape == (5, 37, 29) and torch.equal(one, rel[1])


def test_fallback_float32_within_twice_the_reference_float32_error(golden):
    g, inp = golden
    dec = decoder_of(inp, torch.float32)
    lat = torch.from_numpy(inp["latent"])
    rel = relevancy(lat, dec, torch.from_numpy(inp["pos"]), torch.from_numpy(inp["neg"]))
    assert rel.dtype == torch.float32
    e_rel = np.abs(rel.numpy().astype(np.float64) - g["relevancy"]).max()
    f = dec.decode(lat).reshape(-1, 512)[torch.from_numpy(inp["samples"])]
    e_feat = np.abs(f.numpy().astype(np.float64) - g["features"]).max()
    print(f"float32 fallback error: relevancy {e_rel:.3g} (reference {float(g['relevancy_f32_err']):.3g}), "
          f"features {e_feat:.3g} (reference {float(g['features_f32_err']):.3g})")
    assert e_rel <= 2 * float(g["relevancy_f32_err"]) and e_feat <= 2 * float(g["features_f32_err"])


def test_state_dict_loading():
    ws, bs = qc.decoder_arrays([3, 16, 32, 64], 5)
    sd = qc.state_dict(ws, bs, torch)
    full = dict(sd)
    full.update({"encoder.0.weight": torch.zeros(256, 512), "encoder.0.bias": torch.zeros(256),
                 "encoder.1.weight": torch.ones(256), "encoder.1.bias": torch.zeros(256),
                 "encoder.1.running_mean": torch.zeros(256), "encoder.1.running_var": torch.ones(256),
                 "encoder.1.num_batches_tracked": torch.tensor(3), "encoder.3.weight": torch.zeros(3, 256),
                 "encoder.3.bias": torch.zeros(3)})
    for d in (LanguageDecoder.from_state_dict(full), LanguageDecoder.from_state_dict(sd)):
        assert d.dims == [3, 16, 32, 64] and d.c_in == 3 and d.d_out == 64
        assert all(torch.equal(w, torch.from_numpy(x)) for w, x in zip(d.weights, ws))
        assert all(torch.equal(b, torch.from_numpy(x)) for b, x in zip(d.biases, bs))
    x = torch.from_numpy(qc.latents((7, 5, 3), 9)).double()
    got = LanguageDecoder.from_state_dict(sd).decode(x)
    assert got.shape == (7, 5, 64) and np.abs(got.numpy() - qc.decode_np(ws, bs, x.numpy())).max() < 1e-12

    missing = {k: v for k, v in sd.items() if not k.startswith("decoder.2.")}
    with pytest.raises(KeyError, match="missing"):
        LanguageDecoder.from_state_dict(missing)
    no_bias = {k: v for k, v in sd.items() if k != "decoder.4.bias"}
    with pytest.raises(KeyError, match="decoder.4.bias is missing"):
        LanguageDecoder.from_state_dict(no_bias)
    with pytest.raises(KeyError, match="no decoder"):
        LanguageDecoder.from_state_dict({"encoder.0.weight": torch.zeros(4, 4)})
    bad_shape = dict(sd)
    bad_shape["decoder.2.bias"] = torch.zeros(31)
    with pytest.raises(ValueError, match="bias .* does not match"):
        LanguageDecoder.from_state_dict(bad_shape)
    no_chain = dict(sd)
    no_chain["decoder.2.weight"] = torch.zeros(32, 24)
    with pytest.raises(ValueError, match="do not chain"):
        LanguageDecoder.from_state_dict(no_chain)


def test_load_reads_a_checkpoint_file(tmp_path):
    ws, bs = qc.decoder_arrays([3, 16, 32], 6)
    path = tmp_path / "best_ckpt.pth"
    torch.save(qc.state_dict(ws, bs, torch), path)
    d = LanguageDecoder.load(str(path))
    assert d.dims == [3, 16, 32] and torch.equal(d.weights[1], torch.from_numpy(ws[1]))


def test_argument_errors():
    ws, bs = qc.decoder_arrays([3, 16, 32], 6)
    d = LanguageDecoder.from_state_dict(qc.state_dict(ws, bs, torch))
    e = torch.zeros(2, 32)
    with pytest.raises(ValueError, match="layout"):
        relevancy(torch.zeros(4, 4, 3), d, e, e, layout="nhwc")
    with pytest.raises(ValueError, match="channels"):
        relevancy(torch.zeros(4, 4, 5), d, e, e)
    with pytest.raises(ValueError, match="pos_embeds and neg_embeds"):
        relevancy(torch.zeros(4, 4, 3), d, torch.zeros(2, 16), e)
    with pytest.raises(ValueError, match="pos_embeds and neg_embeds"):
        relevancy(torch.zeros(4, 4, 3), d, e, torch.zeros(0, 32))
    with pytest.raises(ValueError, match="channels"):
        d.decode(torch.zeros(4, 5))


def test_abi_refusals():
    """Every unsupported shape and every NULL pointer is LSR_EINVAL with a message, decided before
    the device is touched (this host has none); n_pix = 0 is no work."""
    lib = _lib.load()
    err = lambda: lib.lsr_last_error().decode()
    FAKE = 64                                                 # never dereferenced: every call returns early

    def decoder(dims, holes=()):
        d = _lib.Decoder()
        d.n_layers = len(dims) - 1
        for i, x in enumerate(dims[:9]):
            d.dims[i] = x
        for i in range(min(d.n_layers, 8)):
            d.weight[i] = None if ("w", i) in holes else FAKE
            d.bias[i] = None if ("b", i) in holes else FAKE
        return d

    good = decoder(qc.FIXTURE_DIMS)

    def rel(dec=good, n_pix=100, latent=FAKE, n_pos=5, pos=FAKE, n_neg=4, neg=FAKE, out=FAKE):
        return lib.lsr_query_relevancy(ctypes.byref(dec) if dec is not None else None, n_pix, latent, 3, 1, n_pos, pos,
                                       n_neg, neg, 10.0, out, None)

    def dec_(dec=good, n_pix=100, latent=FAKE, out=FAKE):
        return lib.lsr_query_decode(ctypes.byref(dec) if dec is not None else None, n_pix, latent, 3, 1, out, None)

    def refused(rc, text):
        assert rc == 1 and text in err() and err(), (rc, err())   # LSR_EINVAL

    refused(rel(dec=None), "null decoder")
    refused(dec_(dec=None), "null decoder")
    for kw in ({"latent": None}, {"pos": None}, {"neg": None}, {"out": None}):
        refused(rel(**kw), "are required")
    for kw in ({"latent": None}, {"out": None}):
        refused(dec_(**kw), "are required")
    refused(rel(dec=decoder(qc.FIXTURE_DIMS, holes=[("w", 2)])), "missing weight or bias")
    refused(dec_(dec=decoder(qc.FIXTURE_DIMS, holes=[("b", 5)])), "missing weight or bias")
    refused(rel(n_pos=0), "n_pos >= 1")
    refused(rel(n_neg=0), "n_neg >= 1")
    refused(rel(n_pos=61, n_neg=4), "n_pos + n_neg <= 64")
    refused(rel(n_pos=2**31 - 1, n_neg=2**31 - 1), "n_pos + n_neg <= 64")
    for f in (rel, dec_):
        refused(f(dec=decoder([3, 16, 24, 512])), "layer width 24")
        refused(f(dec=decoder([3, 16, 528])), "layer width 528")
        refused(f(dec=decoder([3, 0])), "layer width 0")
        refused(f(dec=decoder([33, 16, 512])), "c_in")
        refused(f(dec=decoder([0, 16, 512])), "c_in")
        nine = decoder([3] + [16] * 8)
        nine.n_layers = 9
        refused(f(dec=nine), "n_layers")
        refused(f(dec=decoder([3])), "n_layers")
        refused(f(n_pix=-1), "n_pix must be >= 0")
        assert f(n_pix=0) == 0
    assert rel(n_pos=60, n_neg=4, n_pix=0) == 0 and rel(n_pos=1, n_neg=1, n_pix=0) == 0
    assert dec_(dec=decoder([32, 512]), n_pix=0) == 0 and dec_(dec=decoder([1] + [512] * 8), n_pix=0) == 0


def test_query_header_handshake():
    """Until the caller has declared its lsr_query.h version every entry point refuses; a mismatch is
    refused too.  Fresh process: the handshake is per process."""
    import sys
    code = f"""
import ctypes
L = ctypes.CDLL({_lib.LIB_PATH!r})
L.lsr_last_error.restype = ctypes.c_char_p
assert L.lsr_query_decode(None, ctypes.c_int64(0), None, ctypes.c_int64(1), ctypes.c_int64(1), None, None) == 1
assert b"lsr_query_require_api" in L.lsr_last_error()
assert L.lsr_query_require_api(2) == 1 and b"mismatch" in L.lsr_last_error()
assert L.lsr_query_require_api(1) == 0
assert L.lsr_query_decode(None, ctypes.c_int64(0), None, ctypes.c_int64(1), ctypes.c_int64(1), None, None) == 1
assert b"null decoder" in L.lsr_last_error()
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_decoder_struct_matches_the_header(tmp_path):
    """The ctypes mirror of lsr_decoder has the C compiler's size and field offsets, and the limits
    the Python side dispatches on are the header's."""
    hdr = os.path.join(ROOT, "include", "lsr_query.h")
    cls = _lib.Decoder
    names = [f[0] for f in cls._fields_]
    assert len(names) == len(set(names))
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{hdr}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(lsr_decoder));']
    lines += [f'printf("{n} %zu\\n", offsetof(lsr_decoder, {n}));' for n in names]
    lines += [f'printf("{m} %d\\n", {m});' for m in ("LSR_QUERY_API_VERSION", "LSR_QUERY_MAX_LAYERS",
                                                      "LSR_QUERY_MAX_PHRASES", "LSR_QUERY_MAX_WIDTH",
                                                      "LSR_QUERY_MAX_INPUT")]
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()))
    want = {"size": ctypes.sizeof(cls), **{n: getattr(cls, n).offset for n in names},
            "LSR_QUERY_API_VERSION": _lib.QUERY_API_VERSION, "LSR_QUERY_MAX_LAYERS": _lib.QUERY_MAX_LAYERS,
            "LSR_QUERY_MAX_PHRASES": _lib.QUERY_MAX_PHRASES, "LSR_QUERY_MAX_WIDTH": _lib.QUERY_MAX_WIDTH,
            "LSR_QUERY_MAX_INPUT": _lib.QUERY_MAX_INPUT}
    assert got == want
    assert len(cls().dims) == _lib.QUERY_MAX_LAYERS + 1 and len(cls().weight) == _lib.QUERY_MAX_LAYERS


def test_query_frames(tmp_path):
    """Three tiny level folders, two frames: frame 0 has every value > 0 (saved in (0, 1): mapped back
    by x * 2 - 1 under rescale="auto"), frame 1 has a non-positive value (left as it is)."""
    dims, H, W = [3, 16, 32], 5, 4
    ws, bs = qc.decoder_arrays(dims, 11)
    dec = LanguageDecoder.from_state_dict(qc.state_dict(ws, bs, torch))
    frames = [np.abs(qc.latents((3, H, W, 3), 12)) * 0.9 + 0.05, qc.latents((3, H, W, 3), 13)]
    assert frames[0].min() > 0 and frames[1].min() <= 0
    frames[1][0] = np.abs(frames[1][0]) + 0.01                # one level all positive: the rule is per frame
    levels = []
    for l in range(3):
        d = tmp_path / f"level_{l + 1}"
        (d / "renders_npy").mkdir(parents=True)
        for i, fr in enumerate(frames):
            np.save(d / "renders_npy" / f"{i:05d}.npy", fr[l].astype(np.float32))
        levels.append(str(d))
    e = torch.from_numpy(qc.phrase_embeddings(ws, bs, frames[1].reshape(-1, 3), 3, 14))
    pos, neg = e[:2], e[2:]

    out = tmp_path / "auto"
    paths = query_frames(levels, dec, pos, neg, str(out))
    assert [os.path.relpath(p, out) for p in paths] == ["relevancy_npy/00000.npy", "relevancy_npy/00001.npy"]
    assert sorted(os.listdir(out / "relevancy_npy")) == ["00000.npy", "00001.npy"]
    got = [np.load(p) for p in paths]
    assert all(g.shape == (3, 2, H, W) and g.dtype == np.float32 for g in got)
    want0 = relevancy(torch.from_numpy(frames[0]) * 2.0 - 1, dec, pos, neg).numpy()
    want1 = relevancy(torch.from_numpy(frames[1]), dec, pos, neg).numpy()
    assert np.array_equal(got[0], want0) and np.array_equal(got[1], want1)

    off = [np.load(p) for p in query_frames(levels, dec, pos, neg, str(tmp_path / "off"), rescale=False)]
    raw0 = relevancy(torch.from_numpy(frames[0]), dec, pos, neg).numpy()
    assert np.array_equal(off[0], raw0) and np.array_equal(off[1], want1)
    assert np.abs(raw0 - want0).max() > 1e-3                  # the rule changes the answer

    with pytest.raises(FileNotFoundError):
        query_frames([str(tmp_path / "nothing")], dec, pos, neg, str(tmp_path / "x"))
    with pytest.raises(ValueError, match="rescale"):
        query_frames(levels, dec, pos, neg, str(tmp_path / "x"), rescale="always")
