"""GPU checks of language_tiles' native path (lsr_tiles_census / _plan / _render) against
tests/tiles_cases.py's numpy restatement and against the torch-ops fallback on the same device:
equality throughout, the arithmetic being integer."""
import numpy as np
import pytest
import torch

import tiles_cases as tc

pytestmark = pytest.mark.gpu


def frame(name):
    image, m, want = tc.case(name)
    return torch.from_numpy(image.copy()).cuda(), torch.from_numpy(m.copy()).cuda(), want


@pytest.fixture
def native_only(monkeypatch):
    """prepare_frame must not reach the fallback."""
    import language_tiles as lt

    def refuse(*a, **k):
        raise AssertionError("the torch-ops fallback ran")
    monkeypatch.setattr(lt, "_prepare_torch", refuse)
    return lt


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_native_equals_the_restatement(native_only, name):
    image, m, want = frame(name)
    ft = native_only.prepare_frame(image, m)
    assert ft.tiles.is_cuda and ft.seg_maps.is_cuda
    tc.assert_equals_restatement(ft, want)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_fallback_on_the_gpu_equals_native(name):
    import language_tiles as lt
    image, m, _ = frame(name)
    nat = lt.prepare_frame(image, m)
    fb = lt._prepare_torch(image, m.long())
    assert nat.lengths == fb.lengths
    for a, b in ((nat.seg_maps, fb.seg_maps), (nat.labels, fb.labels), (nat.boxes, fb.boxes)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # the tile bytes are equal; the floats are byte / 255 by the kernel's correctly rounded division in
    # one and by a torch op (a product with 1 / 255 on the device: two roundings) in the other, so they
    # may differ by two float32 ulps of a value below 1, 2^-24 each
    assert nat.tiles.dtype == fb.tiles.dtype == torch.float32
    assert torch.equal(torch.round(nat.tiles * 255.0).to(torch.int32), torch.round(fb.tiles * 255.0).to(torch.int32))
    assert float((nat.tiles - fb.tiles).abs().max()) <= 2.0 ** -23


def test_a_label_past_the_table_takes_the_fallback(monkeypatch):
    import language_tiles as lt
    image, m, want = frame("C1024")
    ran = []
    fallback = lt._prepare_torch
    monkeypatch.setattr(lt, "_prepare_torch", lambda *a: ran.append(1) or fallback(*a))
    ft = lt.prepare_frame(image, m)
    assert ran == [1] and ft.tiles.is_cuda
    tc.assert_equals_restatement(ft, want)


def test_bgr_and_strided_inputs(native_only):
    image, m, want = frame("A")
    tc.assert_equals_restatement(native_only.prepare_frame(image.flip(-1), m, bgr=True), want)
    wide = torch.zeros((4, 37, 60), dtype=torch.int32, device="cuda")
    wide[:, :, :53] = m
    tc.assert_equals_restatement(native_only.prepare_frame(image, wide[:, :, :53]), want)


@pytest.mark.parametrize("level", [0, 2])
def test_an_empty_level_is_named(native_only, level):
    image, m = tc.case_empty_level(level)
    with pytest.raises(ValueError, match=rf"level {level} \('{native_only.LEVELS[level]}'\)"):
        native_only.prepare_frame(torch.from_numpy(image).cuda(), torch.from_numpy(m).cuda())


def test_two_calls_give_the_same_bits(native_only):
    image, m, _ = frame("C")
    a, b = native_only.prepare_frame(image, m), native_only.prepare_frame(image, m)
    assert a.lengths == b.lengths and torch.equal(a.seg_maps, b.seg_maps) and torch.equal(a.boxes, b.boxes)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.tiles.view(torch.int32), b.tiles.view(torch.int32))


def test_files_round_trip_through_the_supervision_loader(native_only, tmp_path):
    (ia, ma, wa), (ib, mb, wb) = tc.case("A"), tc.case("B")
    np.save(tmp_path / "labels_b.npy", mb.astype(np.int64))
    out = str(tmp_path / "language_features")
    totals = native_only.build_language_features([ia.copy(), ib.copy()], [ma.copy(), str(tmp_path / "labels_b.npy")],
                                                 tc.fake_embed, out, ["frame_a.png", "00001.jpg"], device="cuda")
    assert totals == [sum(wa["lengths"]), sum(wb["lengths"])]
    tc.check_round_trip(out, ["frame_a", "00001"], [(ma, wa), (mb, wb)])
