"""CPU checks of language_tiles (the frame's tiles and segment maps, and the `_s.npy` / `_f.npy`
files) against tests/tiles_cases.py's plain-numpy restatement of the reference's per-label loop, plus
the argument checks of include/lsr_tiles.h, which run before a device is touched.  The arithmetic is
integer, so everything is compared for equality."""
import ctypes

import numpy as np
import pytest
import torch

import tiles_cases as tc


def frame(name):
    image, m, want = tc.case(name)
    return torch.from_numpy(image.copy()), torch.from_numpy(m.copy()), want


@pytest.mark.parametrize("name", list(tc.CASES))
def test_fallback_equals_the_restatement(name):
    import language_tiles as lt
    image, m, want = frame(name)
    ft = lt.prepare_frame(image, m)
    tc.assert_equals_restatement(ft, want)
    assert ft.seg_maps.dtype == torch.int32 and ft.labels.dtype == torch.int32 and ft.boxes.dtype == torch.int32
    assert ft.tiles.shape[0] == sum(ft.lengths) == int(ft.seg_maps.max()) + 1


def test_case_a_filters_and_marks():
    """The one-pixel-wide and the one-row labels have no tile and their pixels are -1, as are label 0
    and the negative label; the tiles come in ascending label order with the ids' gaps closed."""
    import language_tiles as lt
    image, m, want = frame("A")
    ft = lt.prepare_frame(image, m)
    assert ft.labels[:ft.lengths[0]].tolist() == [1, 2, 5, 9, 12]
    seg0, m0 = ft.seg_maps[0].numpy(), m[0].numpy()
    for lab in (7, 4, 0, -3):
        assert (seg0[m0 == lab] == -1).all()
    for k, lab in enumerate([1, 2, 5, 9, 12]):
        assert (seg0[m0 == lab] == k).all()
    assert int(ft.seg_maps[1][ft.seg_maps[1] >= 0].min()) == ft.lengths[0]       # create's renumbering


def test_other_dtypes_and_bgr():
    import language_tiles as lt
    image, m, want = frame("A")
    tc.assert_equals_restatement(lt.prepare_frame(image.numpy(), m.to(torch.int64).numpy()), want)
    tc.assert_equals_restatement(lt.prepare_frame(image.to(torch.int16), m.to(torch.float32)), want)
    tc.assert_equals_restatement(lt.prepare_frame(image.flip(-1), m, bgr=True), want)
    flipped = lt.prepare_frame(image, m, bgr=True)
    assert torch.equal(flipped.tiles, lt.prepare_frame(image, m).tiles.flip(1))
    with pytest.raises(ValueError, match="whole numbers"):
        lt.prepare_frame(image, m.to(torch.float32) + 0.5)
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        lt.prepare_frame(image.permute(2, 0, 1), m)
    with pytest.raises(ValueError, match=r"\[4, H, W\]"):
        lt.prepare_frame(image, m[:3])


@pytest.mark.parametrize("level", range(4))
def test_an_empty_level_is_named(level):
    import language_tiles as lt
    image, m = tc.case_empty_level(level)
    with pytest.raises(ValueError, match=rf"level {level} \('{lt.LEVELS[level]}'\)"):
        lt.prepare_frame(torch.from_numpy(image), torch.from_numpy(m))


def test_files_round_trip_through_the_supervision_loader(tmp_path):
    import language_tiles as lt
    (ia, ma, wa), (ib, mb, wb) = tc.case("A"), tc.case("B")
    np.save(tmp_path / "labels_b.npy", mb)
    out = str(tmp_path / "language_features")
    totals = lt.build_language_features([ia.copy(), ib.copy()], [ma.copy(), str(tmp_path / "labels_b.npy")],
                                        tc.fake_embed, out, ["frame_a.png", "00001.jpg"])
    assert totals == [sum(wa["lengths"]), sum(wb["lengths"])]
    tc.check_round_trip(out, ["frame_a", "00001"], [(ma, wa), (mb, wb)])
    with pytest.raises(ValueError, match=r"expected \[n, D\]"):
        lt.build_language_features([ia.copy()], [ma.copy()], lambda t: tc.fake_embed(t)[:-1], out, ["x.png"])
    with pytest.raises(ValueError, match="1 images, 2 label maps"):
        lt.build_language_features([ia], [ma, ma], tc.fake_embed, out, ["x.png"])


def test_write_language_features(tmp_path):
    import language_tiles as lt
    seg = -np.ones((4, 3, 5), dtype=np.int32)
    seg[0, 0, 0], seg[3, 2, 4] = 0, 1
    lt.write_language_features(str(tmp_path / "f"), torch.from_numpy(seg), np.eye(2, 7, dtype=np.float64))
    s, f = np.load(tmp_path / "f_s.npy"), np.load(tmp_path / "f_f.npy")
    assert s.dtype == np.float32 and np.array_equal(s, seg) and f.dtype == np.float32 and f.shape == (2, 7)
    with pytest.raises(ValueError, match="index 2 segments, features has 3 rows"):
        lt.write_language_features(str(tmp_path / "g"), seg, np.zeros((3, 7)))
    with pytest.raises(ValueError, match=r"\[4, H, W\]"):
        lt.write_language_features(str(tmp_path / "g"), seg[:2], np.zeros((2, 7)))


def test_abi_refusals():
    """include/lsr_tiles.h: LSR_EINVAL with its message, decided before a device is touched (the
    pointers here are never dereferenced)."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    err = lambda: lib.lsr_last_error().decode()
    need = lib.lsr_tiles_workspace_size(4)
    assert need >= 4 * 1024 * 6 * 4
    assert lib.lsr_tiles_workspace_size(3) == -1 and "L must be 4" in err()
    p = ctypes.c_void_p(256)
    lengths = (ctypes.c_int32 * 4)(2, 1, 1, 1)

    def refused(rc, text):
        assert rc == 1 and text in err(), (rc, err())          # LSR_EINVAL

    census = lambda L=4, H=8, W=8, labels=p, nbytes=need, ws=p: lib.lsr_tiles_census(L, H, W, labels, nbytes, ws, None)
    plan = lambda L=4, H=8, W=8, nbytes=need, ws=p, desc=p, counts=p: lib.lsr_tiles_plan(L, H, W, nbytes, ws, desc,
                                                                                       counts, None)
    render = lambda L=4, H=8, W=8, labels=p, image=p, nbytes=need, ws=p, desc=p, lens=lengths, n=5, seg=p, tiles=p: \
        lib.lsr_tiles_render(L, H, W, labels, image, nbytes, ws, desc, lens, n, seg, tiles, None)
    for step in (census, plan, render):
        refused(step(L=3), "L must be 4")
        refused(step(L=5), "L must be 4")
        refused(step(H=0), "1 <= H, W")
        refused(step(W=0), "1 <= H, W")
        refused(step(W=16385), "1 <= H, W")
        refused(step(ws=None), "workspace required")
        refused(step(nbytes=need - 1), "smaller than lsr_tiles_workspace_size")
        refused(step(ws=ctypes.c_void_p(264)), "16-byte aligned")
    refused(census(labels=None), "null labels")
    refused(plan(desc=None), "null desc or counts")
    refused(plan(counts=None), "null desc or counts")
    for name in ("labels", "image", "desc", "lens", "seg"):
        refused(render(**{name: None}), "null labels, image, desc, lengths or seg_maps")
    refused(render(tiles=None), "null tiles")
    refused(render(n=4), "n = 4 tiles, but the plan's lengths sum to 5")
    refused(render(n=6), "n = 6 tiles, but the plan's lengths sum to 5")
    refused(render(lens=(ctypes.c_int32 * 4)(2, -1, 3, 1)), "lengths[1] = -1")
    refused(render(lens=(ctypes.c_int32 * 4)(1024, 1, 1, 1), n=1027), "lengths[0] = 1024")
