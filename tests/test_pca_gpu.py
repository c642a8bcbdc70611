"""The PCA colouring on the GPU (include/lsr_pca.h, csrc/pca.hip; language_query.pca_image and
LanguagePCA; gaussian_scene.render_set(pca=...)) against the float64 restatement of tests/pca_cases.py.

The bound on [0, 1] outputs is the 1e-5 tests/test_query_gpu.py uses for the f32 MFMA against
float64: a CPU simulation of this pipeline (float32 centred block Grams finished in float64, float32
projection) stays below 2.2e-7 on these inputs, so 1e-5 leaves about 50x for another summation tree.
"""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # CPU container: the driver only runs these on the MI355X box
    pytest.skip("needs a GPU", allow_module_level=True)

import gaussian_scene as gs  # noqa: E402
import language_query as lq  # noqa: E402
import pca_cases  # noqa: E402
import synthetic  # noqa: E402

TOL = 1e-5


def _frame(img, layout):
    """The case's [H, W, C] image on the device in the layout asked for, contiguous."""
    t = torch.from_numpy(np.array(img)).cuda()
    return t.permute(2, 0, 1).contiguous() if layout == "chw" else t


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("name", list(pca_cases.CASES))
def test_pca_image_matches_the_restatement(name, layout):
    img, ref = pca_cases.case(name)
    H, W, C = img.shape
    out = lq.pca_image(_frame(img, layout), layout=layout)
    assert out.shape == (H, W, 3) and out.dtype == torch.float32 and out.is_cuda
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref["out"].reshape(H, W, 3)).max())
    print(f"{name} {layout}: max |out - ref| = {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("name", list(pca_cases.CASES))
def test_basis_matches_the_restatement(name):
    img, ref = pca_cases.case(name)
    pca = lq.LanguagePCA().fit([_frame(img, "chw")])
    mean, comps = pca.mean.cpu().numpy().astype(np.float64), pca.components.cpu().numpy().astype(np.float64)
    ev = pca.explained_variance.cpu().numpy().astype(np.float64)
    e_mean, e_comp = np.abs(mean - ref["mean"]).max(), np.abs(comps - ref["components"]).max()
    e_ev = np.abs(ev / ref["explained_variance"] - 1).max()
    print(f"{name}: mean {e_mean:.3e}, components {e_comp:.3e}, eigenvalues (relative) {e_ev:.3e}")
    assert pca.n_samples == img.shape[0] * img.shape[1] and pca.n_channels == img.shape[2]
    assert e_mean <= TOL and e_comp <= TOL and e_ev <= TOL
    lo, hi = pca.range.cpu().numpy()
    assert abs(lo - ref["lo"]) <= TOL and abs(hi - ref["hi"]) <= TOL


@pytest.mark.parametrize("name", ["17x23x32", "blocks"])
def test_uint8_output_is_the_references_to8b(name):
    img, ref = pca_cases.case(name)
    H, W, C = img.shape
    got = lq.pca_image(_frame(img, "chw"), out="uint8")
    assert got.shape == (H, W, 3) and got.dtype == torch.uint8 and got.is_cuda
    got = got.cpu().numpy().astype(np.int64).reshape(-1, 3)
    scaled = 255.0 * ref["out"]
    want = np.floor(scaled).astype(np.int64)
    assert np.abs(got - want).max() <= 1
    exact = np.abs(scaled - np.round(scaled)) > 255 * TOL      # farther from a boundary than the float bound
    print(f"{name}: {exact.mean():.4f} of the values are away from a boundary")
    assert exact.mean() >= 0.95
    assert np.array_equal(got[exact], want[exact])


@pytest.mark.parametrize("name", ["blocks", "fan-in"])
def test_two_calls_give_the_same_bits(name):
    img, _ = pca_cases.case(name)
    f = _frame(img, "chw")
    a, b = lq.pca_image(f), lq.pca_image(f)
    assert torch.equal(a, b)
    p, q = lq.LanguagePCA().fit([f]), lq.LanguagePCA().fit([f])
    assert torch.equal(p.components, q.components) and torch.equal(p.mean, q.mean)
    assert torch.equal(p.explained_variance, q.explained_variance) and torch.equal(p.range, q.range)
    assert torch.equal(lq.pca_image(f, out="uint8"), lq.pca_image(f, out="uint8"))


def test_a_view_two_strides_describe_needs_no_copy():
    """[H, W, C] memory seen as [C, H, W] (pix_stride = C, chan_stride = 1) is the same call as layout
    "hwc"; a frame whose rows are padded is refused."""
    img, _ = pca_cases.case("33x65x16")
    t = _frame(img, "hwc")
    assert torch.equal(lq.pca_image(t.permute(2, 0, 1)), lq.pca_image(t, layout="hwc"))
    wide = torch.zeros(16, 33, 70, device="cuda")
    with pytest.raises(ValueError, match="two strides cannot describe"):
        lq.pca_image(wide[:, :, :65])
    with pytest.raises(ValueError, match="float32"):
        lq.pca_image(t.double(), layout="hwc")


def test_sequence_fit_is_one_pca_over_all_frames():
    frames, ref = pca_cases.sequence_case()
    dev = [_frame(f, "chw") for f in frames]
    pca = lq.LanguagePCA().fit(iter(dev))
    n = 17 * 23
    assert pca.n_samples == 3 * n
    assert np.abs(pca.mean.cpu().numpy() - ref["mean"]).max() <= TOL
    assert np.abs(pca.components.cpu().numpy() - ref["components"]).max() <= TOL
    assert np.abs(pca.explained_variance.cpu().numpy() / ref["explained_variance"] - 1).max() <= TOL
    lo, hi = pca.range.cpu().numpy()
    assert abs(lo - ref["lo"]) <= TOL and abs(hi - ref["hi"]) <= TOL
    for i, f in enumerate(dev):
        want = ref["out"][i * n:(i + 1) * n].reshape(17, 23, 3)
        err = np.abs(pca.transform(f).cpu().numpy() - want).max()
        print(f"frame {i}: max |out - ref| = {err:.3e}")
        assert err <= TOL
        got8 = pca.transform(f, out="uint8").cpu().numpy().astype(np.int64)
        assert np.abs(got8 - np.floor(255 * want)).max() <= 1
    # the fitted range is not touched by transform()
    assert np.array_equal(pca.range.cpu().numpy(), np.array([lo, hi], dtype=np.float32))


def test_fit_walks_a_reiterable_without_holding_its_frames():
    """A list, an object whose __iter__ makes each frame afresh (what render_set's sequence mode passes: it
    is walked once per sweep) and a one-shot generator give the same bits; transform() takes no range."""
    frames, _ = pca_cases.sequence_case()
    dev = [_frame(f, "chw") for f in frames]
    walks = []

    class Fresh:
        def __iter__(self):
            walks.append(1)
            return (d.clone() for d in dev)

    a, b, c = lq.LanguagePCA().fit(dev), lq.LanguagePCA().fit(Fresh()), lq.LanguagePCA().fit(d for d in dev)
    assert len(walks) == 3                                 # sums, Gram, range
    for q in (b, c):
        assert torch.equal(a.components, q.components) and torch.equal(a.mean, q.mean)
        assert torch.equal(a.explained_variance, q.explained_variance) and torch.equal(a.range, q.range)
        assert q.n_samples == a.n_samples
    assert torch.equal(a.transform(dev[1]), b.transform(dev[1]))


def test_constant_image_gives_zeros_and_leaves_the_next_frame_alone():
    """max y == min y, where the reference divides 0 by 0: zeros, the one departure."""
    const = (0.25 + 0.01 * torch.arange(32, device="cuda", dtype=torch.float32))[:, None, None].expand(32, 17, 23)
    const = const.contiguous()
    out = lq.pca_image(const)
    assert out.shape == (17, 23, 3) and torch.count_nonzero(out) == 0
    assert torch.count_nonzero(lq.pca_image(const, out="uint8")) == 0
    img, ref = pca_cases.case("17x23x32")
    nxt = lq.pca_image(_frame(img, "chw"))
    assert np.abs(nxt.cpu().numpy() - ref["out"].reshape(17, 23, 3)).max() <= TOL


# ---- render_set -------------------------------------------------------------------------------------
W, H = 96, 72


def _scene(P=3000, C=8, seed=0):
    """The tiny scene of tests/test_gaussian_scene_gpu.py."""
    sc = synthetic.make_scene(P, C=C, tanfovx=0.6, tanfovy=0.6 * H / W, seed=seed, logscale_mean=-4.0)
    g = torch.Generator().manual_seed(seed)
    q = sc.rotations * (0.5 + torch.rand(P, 1, generator=g))
    s = gs.GaussianScene(xyz=sc.means3D, features_dc=sc.shs[:, :1].clone(), features_rest=sc.shs[:, 1:].clone(),
                         language_feature=sc.lang * 3.0, opacity=torch.logit(sc.opacities),
                         scaling=torch.log(sc.scales), rotation=q)
    return s.to("cuda")


def _cam(t):
    cam = synthetic.origin_camera(W, H, 0.6)
    cam.time = t
    return cam


def _read_png(path):
    """[H, W, 3] uint8 of a file gaussian_scene.write_png wrote (8-bit RGB, filter 0 on every row)."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            size = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h = size
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3)


def _check_pictures(pngs, pixels, per_frame_pixels):
    """pngs within 1 of the restatement over `pixels` ([N, C] float32, the fitted set).  Where the
    image's spectrum leaves the restatement's basis ill-defined, the basis the device fitted is
    checked to be an eigenbasis of the top three eigenvalues and the pictures are rebuilt from it."""
    ref = pca_cases.pca_reference(pixels)
    gap, lead = pca_cases.well_defined(ref)
    out = ref["out"]
    fallback = gap < pca_cases.EIGEN_GAP or lead < pca_cases.SIGN_MARGIN
    print(f"{len(pngs)} picture(s): eigenvalue ratio {gap:.3f}, sign margin {lead:.4f}: compared with "
          + ("the picture rebuilt from the device's basis (checked to be the top eigenbasis)" if fallback
             else "the restatement's own picture"))
    if fallback:
        C = pixels.shape[1]
        n_frames = len(pixels) // per_frame_pixels
        dev = [torch.from_numpy(pixels[i * per_frame_pixels:(i + 1) * per_frame_pixels].reshape(H, W, C)).cuda()
               for i in range(n_frames)]
        comps = lq.LanguagePCA().fit(dev, layout="hwc").components.cpu().numpy().astype(np.float64)
        xc = pixels.astype(np.float64) - ref["mean"]
        cov = xc.T @ xc / (len(xc) - 1)
        lam = np.einsum("kc,cd,kd->k", comps, cov, comps)
        assert np.abs(comps @ comps.T - np.eye(3)).max() <= TOL
        assert np.abs(lam / ref["explained_variance"] - 1).max() <= TOL
        y = xc @ comps.T
        out = (y - y.min()) / (y.max() - y.min())
    want = np.floor(255 * out).astype(np.int64)
    for i, png in enumerate(pngs):
        got = png.astype(np.int64).reshape(-1, 3)
        assert np.abs(got - want[i * per_frame_pixels:(i + 1) * per_frame_pixels]).max() <= 1


def test_render_set_pca_modes(tmp_path, monkeypatch):
    s = _scene(C=8)
    views = [_cam(t) for t in (0.0, 0.5, 1.0)]
    bg = torch.ones(3, device="cuda")
    calls = []

    def recorder(feature_map):
        calls.append(tuple(feature_map.shape))
        return torch.zeros(feature_map.shape[1], feature_map.shape[2], 3)

    monkeypatch.setattr(gs, "pca_compress", recorder)
    for mode in ("native", "sequence"):
        gs.render_set(str(tmp_path), mode, 7, views, s, bg, output_channel="lang", stage="coarse-lang", pca=mode)
        base = tmp_path / f"{mode}_lang" / "ours_7"
        frames = [np.load(base / "renders_npy" / f"{i:05d}.npy") for i in range(3)]
        assert all(f.shape == (H, W, 8) and f.dtype == np.float32 for f in frames)
        pixels = [((f + np.float32(1.0)) / np.float32(2)).reshape(-1, 8) for f in frames]   # render_set's (r + 1) / 2
        pngs = [_read_png(base / "renders" / f"{i:05d}.png") for i in range(3)]
        assert all(p.shape == (H, W, 3) for p in pngs)
        if mode == "native":
            for png, pix in zip(pngs, pixels):
                _check_pictures([png], pix, H * W)
        else:
            _check_pictures(pngs, np.concatenate(pixels), H * W)
    assert not calls                                       # neither device mode went through pca_compress
    # the default is today's path: every frame through pca_compress, unchanged
    gs.render_set(str(tmp_path), "default", 7, views, s, bg, output_channel="lang", stage="coarse-lang")
    assert calls == [(8, H, W)] * 3
    assert not _read_png(tmp_path / "default_lang" / "ours_7" / "renders" / "00000.png").any()
    with pytest.raises(ValueError, match='pca must be'):
        gs.render_set(str(tmp_path), "bad", 7, views, s, bg, output_channel="lang", stage="coarse-lang", pca="torch")
