"""Frames for the language-feature tiles (language_tiles, include/lsr_tiles.h) and the yardstick they
are held to: a plain-numpy restatement of the reference's per-label loop
(preprocess/generate_clip_features.py: sam_encoder's np.where and bbox, mask2segmap's filter,
get_seg_img's black-out and crop, pad_img, seg_map[mask] = i, create's renumbering), with cv2.resize
replaced by the integer bilinear resize that lsr_tiles.h states.  Every case builder asserts the
properties it exists for, so a case cannot silently stop covering its branch."""
import functools

import numpy as np
import torch

SIDE = 224
CENSUS_ROWS = 4           # LSR_TILES_CENSUS_ROWS: image rows of one census workgroup


# ---- the yardstick ----------------------------------------------------------------------------------

def taps(l):
    """Per output index d of a side-l source: first tap s, second tap s1, weight a (of 448) of the second."""
    s, s1, a = [], [], []
    for d in range(SIDE):
        t = (2 * d + 1) * l - SIDE
        si, ai = (0, 0) if t < 0 else (t // (2 * SIDE), t % (2 * SIDE))
        if si >= l - 1:
            si, ai = l - 1, 0
        s.append(si)
        s1.append(min(si + 1, l - 1))
        a.append(ai)
    return np.array(s), np.array(s1), np.array(a)


def resize(pad):
    """[l, l, 3] uint8 -> [224, 224, 3] uint8: bilinear, half-pixel centres, replicated edge, exact."""
    l = pad.shape[0]
    assert pad.shape == (l, l, 3)
    s, s1, a = taps(l)
    p = pad.astype(np.int32)
    w0, w1 = (2 * SIDE - a).astype(np.int32), a.astype(np.int32)
    # the sum over the four taps of wx wy byte, columns first (integers: the order does not matter)
    cols = w0[None, :, None] * p[:, s] + w1[None, :, None] * p[:, s1]               # [l, 224, 3]
    S = w0[:, None, None] * cols[s] + w1[:, None, None] * cols[s1]
    assert S.dtype == np.int32 and 0 <= S.min() and S.max() <= 255 * 448 * 448      # fits
    return ((S + 100352) // 200704).astype(np.uint8)


def restate(image, label_maps):
    """image [H, W, 3] uint8 (RGB), label_maps [4, H, W] integers ->
    dict(seg_maps [4, H, W] int32, lengths [4], labels [n], boxes [n, 4] (x, y, w, h), tile_bytes [n, 3, 224, 224])."""
    seg_maps, lengths, labels, boxes, tiles = [], [], [], [], []
    for i in range(4):
        m = label_maps[i]
        masks = []
        present = set(np.unique(m).tolist())
        for j in range(1, int(m.max()) + 1):
            if j not in present:                      # (the reference finds this out from an empty np.where)
                continue
            ys, xs = np.where(m == j)
            masks.append((m == j, j, [xs.min(), ys.min(), xs.max() - xs.min(), ys.max() - ys.min()]))
        masks = [k for k in masks if k[2][2] != 0 and k[2][3] != 0]
        seg_map = -np.ones(image.shape[:2], dtype=np.int32)
        for idx, (segm, j, (x, y, w, h)) in enumerate(masks):
            img = image.copy()
            img[segm == 0] = 0
            crop = img[y:y + h, x:x + w]
            l = max(w, h)
            pad = np.zeros((l, l, 3), dtype=np.uint8)
            if h > w:
                pad[:, (h - w) // 2:(h - w) // 2 + w] = crop
            else:
                pad[(w - h) // 2:(w - h) // 2 + h] = crop
            tiles.append(resize(pad).transpose(2, 0, 1))
            labels.append(j)
            boxes.append([x, y, w, h])
            seg_map[segm] = idx
        seg_maps.append(seg_map)
        lengths.append(len(masks))
    for j in range(1, 4):
        v = seg_maps[j]
        v[v != -1] += sum(lengths[:j])
    return dict(seg_maps=np.stack(seg_maps), lengths=lengths, labels=np.array(labels, dtype=np.int32),
                boxes=np.array(boxes, dtype=np.int32).reshape(-1, 4),
                tile_bytes=np.stack(tiles) if tiles else np.zeros((0, 3, SIDE, SIDE), np.uint8))


def stats(level_map):
    """{label >= 1: (x, y, w, h, pixels)} of one level."""
    out = {}
    for j in np.unique(level_map):
        if j >= 1:
            ys, xs = np.where(level_map == j)
            out[int(j)] = (xs.min(), ys.min(), xs.max() - xs.min(), ys.max() - ys.min(), len(ys))
    return out


def kept(st):
    return {j: b for j, b in st.items() if b[2] != 0 and b[3] != 0}


def _image(H, W, seed):
    return np.random.default_rng(seed).integers(1, 256, size=(H, W, 3), dtype=np.uint8)     # no black pixel of its own


# ---- case A: 37 x 53, hand-placed ---------------------------------------------------------------------

def case_a():
    H, W = 37, 53
    m = np.zeros((4, H, W), dtype=np.int32)
    a = m[0]
    a[2:12, 3:9] = 1            # h > w
    a[2:7, 12:31] = 2           # w > h
    a[14:23, 3:12] = 5          # h == w
    a[14:31, 20:40:2] = 9       # 9 and 12 interleaved, column by column, inside one bbox
    a[14:31, 21:40:2] = 12
    a[5:16, 50] = 7             # one pixel wide: filtered
    a[34, 5:26] = 4             # a single row: filtered
    a[32:34, 40:46] = -3        # negative: background
    b = m[1]
    b[0, :] = b[H - 1, :] = 1   # touches all four frame edges
    b[:, 0] = b[:, W - 1] = 1
    b[5:21, 5:31] = 2
    b[24:33, 35:50] = 6
    c = m[2]
    c[:, :20] = 3
    c[10:30, 25:45] = 8
    c[3, 30] = 11               # one pixel: filtered
    d = m[3]
    d[1:36, 1:26] = 2
    d[1:36, 27:52] = 5
    image = _image(H, W, 1)

    s0 = stats(m[0])
    assert set(s0) == {1, 2, 4, 5, 7, 9, 12} and (m[0] == 0).any() and (m[0] < 0).any()
    assert s0[1][3] > s0[1][2] and s0[2][2] > s0[2][3] and s0[5][2] == s0[5][3]
    assert s0[7][2] == 0 and s0[7][3] != 0 and s0[4][3] == 0 and s0[4][2] != 0           # filtered each way
    assert s0[9][:2] == (20, 14) and s0[12][:2] == (21, 14) and s0[9][2] == s0[12][2] == 18  # overlapping boxes
    assert stats(m[1])[1][:4] == (0, 0, W - 1, H - 1)
    assert stats(m[2])[11][2:4] == (0, 0)
    assert all(kept(stats(m[i])) for i in range(4))
    assert all(max(bx[2], bx[3]) < SIDE for i in range(4) for bx in kept(stats(m[i])).values())   # all upscales
    return image, m


# ---- case B: 300 x 470, the resize's regimes ----------------------------------------------------------

def case_b():
    H, W = 300, 470
    m = np.zeros((4, H, W), dtype=np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    holes = (xx + 2 * yy) % 7 == 0

    def block(level, label, y0, y1, x0, x1):
        """rows y0..y1 and columns x0..x1 inclusive, with holes but its four corners"""
        r = np.zeros((H, W), bool)
        r[y0:y1 + 1, x0:x1 + 1] = True
        r &= ~holes
        for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
            r[y, x] = True
        m[level][r] = label

    block(0, 1, 10, 40, 5, 465)          # extent 460: downscale
    block(0, 2, 50, 150, 10, 458)        # extent 448: the 2x case
    block(0, 3, 160, 290, 20, 244)       # l == 224: the identity
    block(1, 4, 20, 280, 100, 200)       # h > w, downscale
    block(1, 2, 30, 90, 250, 400)
    block(2, 7, 5, 295, 3, 467)          # nearly the frame
    block(3, 1, 100, 200, 100, 200)
    block(3, 9, 100, 200, 210, 440)
    image = _image(H, W, 2)

    s0 = kept(stats(m[0]))
    assert max(s0[1][2:4]) == 460 and max(s0[2][2:4]) == 448 and max(s0[3][2:4]) == 224
    assert set(taps(448)[2]) == {224}                                   # every weight a is one half
    s, s1, a = taps(224)
    assert np.array_equal(s, np.arange(224)) and not a.any()            # the identity
    b = stats(m[1])[4]
    assert b[3] > b[2] and b[3] > SIDE
    assert (m[0][10:41, 5:466] == 0).any()                              # the holes are there: the black-out matters
    return image, m


# ---- case C: 270 x 360, Voronoi-style maps with about 200 labels per level ---------------------------

def case_c():
    H, W, sites = 270, 360, 200
    rng = np.random.default_rng(3)
    m = np.zeros((4, H, W), dtype=np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(4):
        sy, sx = rng.integers(0, H, sites), rng.integers(0, W, sites)
        ids = rng.choice(np.arange(1, 1023), size=sites, replace=False)
        if i == 0:
            ids[0] = 1023
        for y0 in range(0, H, 30):                                        # (row bands: a band's distances fit the cache)
            band = slice(y0, y0 + 30)
            d = (yy[band, :, None] - sy) ** 2 + (xx[band, :, None] - sx) ** 2
            m[i][band] = ids[np.argmin(d, axis=-1)]
        m[i][rng.random((H, W)) < 0.02] = 0                               # background speckle
    image = _image(H, W, 4)

    for i in range(4):
        st = stats(m[i])
        assert 150 <= len(st) <= sites and len(kept(st)) >= 150
        crossing = [j for j, b in st.items() if b[1] // CENSUS_ROWS != (b[1] + b[3]) // CENSUS_ROWS]
        assert 2 * len(crossing) > len(st)                                # most labels span census workgroups
    k0 = kept(stats(m[0]))
    assert 1023 in k0 and m.max() == 1023
    return image, m


def case_c_1024():
    """case C with its label 1023 renamed 1024: past the native table."""
    image, m = case_c()
    m = m.copy()
    m[0][m[0] == 1023] = 1024
    assert m.max() == 1024 and 1024 in kept(stats(m[0]))
    return image, m


def case_empty_level(level):
    """case A with `level` left without a kept label (one filtered label remains)."""
    image, m = case_a()
    m = m.copy()
    m[level] = 0
    m[level][4, 7:20] = 3
    assert stats(m[level]) and not kept(stats(m[level]))
    return image, m


CASES = {"A": case_a, "B": case_b, "C": case_c, "C1024": case_c_1024}


@functools.lru_cache(maxsize=None)
def case(name):
    """(image, label_maps, the restatement's result) of a named case, built once."""
    image, m = CASES[name]()
    image.setflags(write=False)
    m.setflags(write=False)
    return image, m, restate(image, m)


def assert_equals_restatement(ft, want):
    """A FrameTiles against restate()'s dict: everything exactly."""
    assert list(ft.lengths) == list(want["lengths"])
    assert np.array_equal(ft.seg_maps.cpu().numpy(), want["seg_maps"])
    assert np.array_equal(ft.labels.cpu().numpy(), want["labels"])
    assert np.array_equal(ft.boxes.cpu().numpy(), want["boxes"])
    tiles = ft.tiles.cpu().numpy()
    assert tiles.dtype == np.float32 and tiles.shape == want["tile_bytes"].shape
    got = np.rint(tiles * 255.0).astype(np.int32)
    assert np.array_equal(got, want["tile_bytes"].astype(np.int32))
    assert np.abs(tiles * 255.0 - got).max() < 1e-3                      # a byte / 255, nothing in between


# ---- the files -------------------------------------------------------------------------------------

def fake_embed(tiles):
    """A fixed stand-in for CLIP: [n, 24] from the tiles' channel means and a few pixels."""
    n = tiles.shape[0]
    g = torch.Generator().manual_seed(5)
    proj = torch.randn(3 * 16, 24, generator=g).to(tiles.device)
    feats = torch.nn.functional.adaptive_avg_pool2d(tiles, 4).reshape(n, -1)
    return feats @ proj + 0.1


def check_round_trip(folder, stems, frames):
    """The written files through language_supervision's loader, at each level."""
    import language_supervision as ls
    for stem, (m, want) in zip(stems, frames):
        seg_file, feat_file = np.load(f"{folder}/{stem}_s.npy"), np.load(f"{folder}/{stem}_f.npy")
        assert seg_file.dtype == np.float32 and seg_file.shape == want["seg_maps"].shape
        assert feat_file.dtype == np.float32 and feat_file.shape == (sum(want["lengths"]), 24)
        assert np.array_equal(feat_file, feat_file.astype(np.float16).astype(np.float32))    # rounded through float16
        assert np.abs(np.linalg.norm(feat_file.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -10
        start = 0
        for level in range(4):
            sup = ls.load_language_supervision(folder, stem, level)
            keep = {j for j, b in kept(stats(m[level])).items()}
            assert np.array_equal(sup.labelled().numpy(), np.isin(m[level], sorted(keep)))
            rows = sup.seg[sup.labelled()]
            assert int(rows.min()) == start and int(rows.max()) == start + want["lengths"][level] - 1
            start += want["lengths"][level]
