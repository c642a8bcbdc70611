"""The per-pixel image check (lsr_testutil.image_check) and the scenes of
tests/test_forward_branches_gpu.py (fwd_cases), on the oracle alone.

(a) the float oracle passes image_check's per-element part against the double oracle on every
    scene and view at coefficient 1e-4 throughout, with the same radii and n_contrib: the bound is
    one the reference meets without any kernel.  Largest |f32 - f64| / A over the 28 scenes (the
    23 of fwd_cases and the other 5 of bwd_cases, whose forwards the backward module checks the
    same way): colour 9.1e-5 (W5, view 0), language 3.6e-5 (W32, view 0), depth 3.2e-5 (HE).
    The float oracle rounds the projection (centres, conics, hence the weights) as well as the
    sums, so these are upper limits for a kernel that shares the float oracle's weights bit for
    bit; image_check grants the kernels' fp32 sums only (2 k + 8) 2^-24 (lsr_testutil.image_coef).
(b) every scene's preconditions hold (fwd_cases.check_preconditions).
(c) the check has teeth, on scenes G, H, L7 and L32, with image_check's exact checks left on (the
    oracle's own state stands in for the native one).  A language image that lost the bf16 lo half
    of the language operand -- the double oracle run on language rows rounded to bf16 -- passes the
    tensor-wide max |language - ref| <= 1e-3 and fails image_check on at least half of its
    elements.  The last channel zeroed on the pixels with the smallest A -- in ascending order of
    A as many as the tensor-wide tolerance lets through, at least 1 in 100 -- passes it too and
    fails image_check on at least 95 % of the doctored elements.  Measured: bf16 rows, max abs
    error 8.9e-4 / 9.1e-4 / 2.1e-4 / 1.1e-4 (G / H / L7 / L32) with 0.99 / 0.99 / 0.64 / 0.63 of the
    elements over the bound; zeroed channel, 48 / 126 / 11 / 87 pixels doctored, every one caught.
    The 1 in 100 holds over the four scenes together (272 of 11451 pixels) and in H, L7 and L32
    singly; in scene G only 48 of the 5063 pixels (0.95 %) have |language[47]| <= 1e-3, so there
    no doctoring that the tensor-wide tolerance lets through can reach it -- a property of the
    scene, not of the check, hence the floor is asserted on the scenes' sum.
(d) the exact checks have teeth too: one tile_max_contrib off by one, the preset (~0, 0) left in an
    empty tile's range, final_T or an uncovered pixel's colour moved by one bit each fail.
"""
import numpy as np
import pytest
import torch

import fwd_cases
from lsr_testutil import image_check, oracle_as_native, run_oracle

LANG_TOL = 1e-3           # the tensor-wide contract (tests/test_parity_gpu.py)
TEETH = ["G", "H", "L7", "L32"]


def _standing_in(r32, lang=None):
    """The float oracle's images and state in the native ones' place."""
    return r32.color, r32.lang if lang is None else lang, r32.depth, oracle_as_native(r32)


@pytest.mark.parametrize("name", list(fwd_cases.CASES) + fwd_cases.BWD_ONLY)
def test_f32_oracle_passes_against_f64(name):
    for v, (a, b, A) in enumerate(zip(fwd_cases.reference(name, False), fwd_cases.reference(name, True),
                                      fwd_cases.lang_scale(name))):
        np.testing.assert_array_equal(a.radii, b.radii)
        np.testing.assert_array_equal(a.state()["n_contrib"], b.state()["n_contrib"])
        bad, stats = image_check(_standing_in(a), b, A, coef=1e-4, exact=False)
        print(name, v, {k: float(f"{s['max_err_over_A']:.2e}") for k, s in stats.items()})
        assert not bad, (name, v, bad, stats)


@pytest.mark.parametrize("name", list(fwd_cases.CASES))
def test_scene_preconditions(name):
    print(name, fwd_cases.check_preconditions(name))


@pytest.mark.parametrize("name", list(fwd_cases.CASES) + fwd_cases.BWD_ONLY)
def test_oracle_state_passes_exact_checks(name):
    """The float oracle standing in for the kernels passes image_check whole: the exact checks ask
    nothing the reference's own state does not have."""
    for r, A in zip(fwd_cases.reference(name), fwd_cases.lang_scale(name)):
        bad, stats = image_check(_standing_in(r), r, A)
        assert not bad, (name, bad)


@pytest.mark.parametrize("name", TEETH)
def test_image_check_rejects_lost_bf16_lo_half(name):
    c, r32, A = fwd_cases.case(name), fwd_cases.reference(name)[0], fwd_cases.lang_scale(name)[0]
    rows = c.scene.lang.to(torch.bfloat16).to(torch.float32).numpy()
    lost = run_oracle(c.scene, c.cams[0], double=True, lang=rows, **c.run_kw()).lang.astype(np.float32)
    true = fwd_cases.reference(name, True)[0].lang
    old = float(np.abs(lost - true).max())
    assert old <= LANG_TOL and np.abs(lost - r32.lang).max() <= LANG_TOL, old   # today's check accepts it
    bad, stats = image_check(_standing_in(r32, lost), r32, A)
    assert set(bad) == {"lang"}, bad
    frac = bad["lang"]["elements"] / lost.size
    print(name, "max abs", f"{old:.2e}", "fraction over the bound", f"{frac:.3f}", stats["lang"])
    assert frac >= 0.5, (name, frac)


def _zeroed_last_channel(name):
    """(doctored language image, doctored pixels, pixels with A > 0) of the scene: the last channel
    zeroed on the pixels, in ascending order of A, whose loss the tensor-wide tolerance cannot see
    (a pixel's value does not grow with its A as a Gaussian's gradient does, so they are no prefix
    of the order: every such pixel is taken, none is left that could be added)."""
    c, r32, A = fwd_cases.case(name), fwd_cases.reference(name)[0], fwd_cases.lang_scale(name)[0]
    ch = c.C - 1
    true, a = np.abs(r32.lang[ch]).ravel(), A[ch].ravel()
    pix = np.nonzero(a > 0)[0]
    pix = pix[np.argsort(a[pix], kind="stable")]
    pix = pix[true[pix] <= LANG_TOL]
    assert len(pix) >= 1 and true[pix].min() > 0                 # something was there to lose
    lang = r32.lang.copy()
    lang[ch].reshape(-1)[pix] = 0.0
    return lang, len(pix), int((a > 0).sum())


@pytest.mark.parametrize("name", TEETH)
def test_image_check_rejects_zeroed_last_channel(name):
    r32, A = fwd_cases.reference(name)[0], fwd_cases.lang_scale(name)[0]
    lang, n, covered = _zeroed_last_channel(name)
    assert np.abs(lang - r32.lang).max() <= LANG_TOL             # today's check accepts it
    bad, stats = image_check(_standing_in(r32, lang), r32, A)
    assert set(bad) == {"lang"}, bad
    print(name, "doctored", n, "of", covered, "caught", bad["lang"]["elements"])
    # every doctored element is caught, bar those whose terms cancel to under 1e-4 of their size
    assert bad["lang"]["elements"] >= 0.95 * n, (name, bad["lang"]["elements"], n)


def test_zeroed_last_channel_doctors_one_pixel_in_100():
    """The doctoring above is no token one: at least 1 pixel in 100, over the scenes together (see
    the module docstring for scene G)."""
    counts = {name: _zeroed_last_channel(name)[1:] for name in TEETH}
    print(counts)
    n, covered = (sum(x[i] for x in counts.values()) for i in (0, 1))
    assert n * 100 >= covered, counts


@pytest.mark.parametrize("doctor", ["tile_max", "preset_range", "final_T", "uncovered_colour", "radii"])
def test_image_check_exact_parts_reject(doctor):
    r = fwd_cases.reference("HE")[0]
    A = fwd_cases.lang_scale("HE")[0]
    color, lang, depth, st = _standing_in(r)
    color, st.ranges, st.tile_max, st.final_T, st.radii = (x.copy() for x in (color, st.ranges, st.tile_max,
                                                                               st.final_T, st.radii))
    empty = np.nonzero(st.ranges[:, 0] == st.ranges[:, 1])[0]
    y, x = np.argwhere(st.n_contrib == 0)[0]
    if doctor == "tile_max":
        st.tile_max[np.argmax(st.tile_max)] += 1
    elif doctor == "preset_range":
        st.ranges[empty[0]] = (0xFFFFFFFF, 0)
    elif doctor == "final_T":
        st.final_T[st.n_contrib > 0] = np.nextafter(st.final_T[st.n_contrib > 0], np.float32(0))
    elif doctor == "uncovered_colour":
        color[1, y, x] = np.nextafter(color[1, y, x], np.float32(0))
    else:
        st.radii[np.argmax(st.radii)] += 1
    bad, _ = image_check((color, lang, depth, st), r, A)
    want = dict(tile_max="tile_max_contrib", preset_range="empty_tile_range", final_T="binning",
                uncovered_colour="uncovered_pixels", radii="radii")[doctor]
    assert want in bad, (doctor, bad)
