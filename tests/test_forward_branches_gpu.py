"""Every instantiation of the forward compositor against the oracle, pixel by pixel.

The forward composite is k_render_fwd_wave (render_fwd_wave.hip) at pads 0, 4, 8, 16 and 64 and
k_render_fwd_wave_mfma (render_fwd_mfma_wave.hip: 17..32 channels, the language sums on matrix
cores) with and without pre-split language operands; launch_render_fwd_wave_views chooses by the
channel count.  Each pad stages its language rows as whole float4 rows (C == pad) or scalar by
scalar (c < C).  The cases (scenes: fwd_cases) reach every instantiation and both stagings, on the
ragged 83 x 61 base scene unless noted:

    case   C    kernel                          staging         scene
    A      0    k_render_fwd_wave<0>            none
    N6     6    k_render_fwd_wave<0>            none            include_feature=False: language exactly 0
    C4     4    k_render_fwd_wave<4>            float4
    C1     1    k_render_fwd_wave<4>            scalar
    P      8    k_render_fwd_wave<8>            float4          cov3D + colors precomputed
    B      5    k_render_fwd_wave<8>            scalar
    C16    16   k_render_fwd_wave<16>           float4
    C12    12   k_render_fwd_wave<16>           scalar
    C64    64   k_render_fwd_wave<64>           float4
    C33    33   k_render_fwd_wave<64>           scalar
    G      48   k_render_fwd_wave<64>           scalar
    C63    63   k_render_fwd_wave<64>           scalar
    F      32   k_render_fwd_wave_mfma<false>   float4
    E      17   k_render_fwd_wave_mfma<false>   masked scalar   scale_modifier 1.6
    C24    24   k_render_fwd_wave_mfma<false>   masked scalar
    C31    31   k_render_fwd_wave_mfma<false>   masked scalar
    F PRE  32   k_render_fwd_wave_mfma<true>    pre-split       preprocess_views_native(split_language=True)
    S7     7    k_render_fwd_wave<8>            scalar          long and saturating, 35 x 19
    S32    32   k_render_fwd_wave_mfma<false>   float4          long and saturating, 35 x 19
    HE     5    k_render_fwd_wave<8>            scalar          half empty: 12 of 24 tiles without entries
    W5     5    k_render_fwd_wave<8>            scalar          3 views in one launch, the middle one empty
    W32    32   k_render_fwd_wave_mfma<true>    pre-split       3 views in one launch, the middle one empty

(bwd_cases' scenes C, D, H, L7, L32, V16 and V64 go through the same check from
tests/test_backward_branches_gpu.py.)

Asserted per case and view: the scene's preconditions on the oracle's state
(fwd_cases.check_preconditions), then lsr_testutil.image_check against the float oracle: radii,
final_T bit for bit, every pixel's last contributor, tile_max_contrib, the (0, 0) range of every
tile without entries, uncovered pixels exactly (bg, 0, 0, T = 1); and per element
|native - ref| <= coef A with coef = min(1e-4, (2 n_contrib + 8) 2^-24) (1e-4 for the language image
of the matrix-core kernel), exactly 0 where A = 0.

Measured on an MI355X, against the float oracle (recorded, not used to set any bound): the largest
err / A per case, view and output and, in brackets, the largest err / (coef A).  The fp32 sums sit
at about 4 units of 2^-24 whatever the list length, a fifth of the derived bound at the most (W5:
a pixel with 4 contributors); the matrix-core language sums at 2.1e-5 A, as the backward's bf16
hi / lo sums do (tests/test_backward_branches_gpu.py: 2.3e-5).  The float oracle against the double
one on the same scenes (tests/test_forward_check.py) is at most 9.1e-5 A (colour), 3.6e-5 A
(language) and 3.2e-5 A (depth).

    case    view  colour              language            depth
    A       0     2.2e-07 (0.091)     0                   2.2e-07 (0.072)
    N6      0     2.3e-07 (0.051)     0                   2.5e-07 (0.044)
    C4      0     2.3e-07 (0.076)     2.2e-07 (0.072)     2.2e-07 (0.072)
    C1      0     2.4e-07 (0.062)     1.1e-07 (0.030)     2.2e-07 (0.072)
    P       0     2.3e-07 (0.071)     2.1e-07 (0.113)     2.2e-07 (0.072)
    B       0     2.3e-07 (0.051)     2.5e-07 (0.042)     2.5e-07 (0.044)
    C16     0     2.3e-07 (0.051)     2.3e-07 (0.048)     2.5e-07 (0.044)
    C12     0     2.3e-07 (0.051)     2.7e-07 (0.051)     2.5e-07 (0.044)
    C64     0     2.3e-07 (0.072)     2.9e-07 (0.111)     2.2e-07 (0.072)
    C33     0     2.3e-07 (0.076)     2.4e-07 (0.124)     2.2e-07 (0.072)
    G       0     2.3e-07 (0.051)     2.5e-07 (0.061)     2.5e-07 (0.044)
    C63     0     2.3e-07 (0.048)     2.4e-07 (0.075)     2.5e-07 (0.044)
    F       0     2.3e-07 (0.076)     1.9e-05 (0.188)     2.2e-07 (0.072)
    E       0     2.5e-07 (0.042)     1.9e-05 (0.191)     2.1e-07 (0.040)
    C24     0     2.3e-07 (0.076)     1.8e-05 (0.178)     2.2e-07 (0.072)
    C31     0     2.2e-07 (0.044)     1.9e-05 (0.194)     2.5e-07 (0.044)
    F PRE   0     2.3e-07 (0.076)     1.9e-05 (0.188)     2.2e-07 (0.072)
    S7      0     2.4e-07 (0.006)     1.5e-07 (0.002)     2.2e-07 (0.007)
    S32     0     2.4e-07 (0.006)     5.6e-06 (0.056)     2.2e-07 (0.007)
    HE      0     1.7e-07 (0.095)     2.2e-07 (0.120)     1.8e-07 (0.082)
    W5      0     2.3e-07 (0.164)     2.8e-07 (0.214)     2.2e-07 (0.174)
    W5      1     0                   0                   0
    W5      2     2.1e-07 (0.099)     2.2e-07 (0.097)     2.2e-07 (0.061)
    W32     0     2.2e-07 (0.141)     2.1e-05 (0.206)     2.2e-07 (0.148)
    W32     1     0                   0                   0
    W32     2     2.4e-07 (0.099)     2.1e-05 (0.210)     2.2e-07 (0.084)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # CPU container: the driver only runs these on the MI355X box
    pytest.skip("needs a GPU", allow_module_level=True)

import diff_gaussian_rasterization as dgr  # noqa: E402
import fwd_cases  # noqa: E402
from lsr_testutil import image_check, raster_settings, run_native  # noqa: E402


def _check(name, nats, label=None):
    """Preconditions, then every view's native (color, lang, radii, depth, state) through
    image_check against its own oracle run."""
    c = fwd_cases.case(name)
    print(label or name, "preconditions", fwd_cases.check_preconditions(name))
    assert len(nats) == len(c.cams)
    for v, (nat, ref, A) in enumerate(zip(nats, fwd_cases.reference(name), fwd_cases.lang_scale(name))):
        color, lang, radii, depth, st = nat
        assert radii is st.radii or torch.equal(radii, st.radii)
        assert lang.shape == (c.C, c.H, c.W)
        bad, stats = image_check((color, lang, depth, st), ref, A)
        print(label or name, "view", v, {k: {n: float(f"{x:.2e}") for n, x in s.items()} for k, s in stats.items()})
        assert not bad, (label or name, v, bad, stats)
    return c


def _views(c, split):
    """The case's cameras through the batched entry points: one compositor launch for all."""
    dev = c.scene.to("cuda")
    rss = [raster_settings(cam, bg=fwd_cases.BG, sh_degree=c.sh_degree, scale_modifier=c.scale_modifier)
           for cam in c.cams]
    pfs = dgr.preprocess_views_native(rss, dev.means3D, dev.opacities, shs=dev.shs, language_feature=dev.lang,
                                      scales=dev.scales, rotations=dev.rotations, split_language=split)
    if split:
        assert pfs[0].inputs.get("language_feature_split") is not None and pfs[0].fin.language_feature_split
    else:
        assert pfs[0].inputs.get("language_feature_split") is None and not pfs[0].fin.language_feature_split
    dgr.binning_views_native(pfs)
    return pfs


@pytest.mark.parametrize("name", ["A", "N6", "C4", "C1", "P", "B", "C16", "C12", "C64", "C33", "G", "C63",
                                  "F", "E", "C24", "C31"])
def test_kernel_and_staging(name):
    c = fwd_cases.case(name)
    nat = run_native(c.scene, c.cams[0], **c.run_kw())
    _check(name, [nat])
    if not c.include_feature:    # the language image is written, as zeros
        assert c.C > 0 and float(nat[1].abs().max()) == 0.0


def test_presplit_operands_case_f():
    """Case F with the language rows' bf16 hi / lo operands made once by the batched preprocess:
    k_render_fwd_wave_mfma<true>."""
    c = fwd_cases.case("F")
    pfs = _views(c, split=True)
    _check("F", [dgr.render_native(pfs[0])], label="F PRE")


@pytest.mark.parametrize("name", ["S7", "S32"])
def test_long_saturating_scene(name):
    c = fwd_cases.case(name)
    _check(name, [run_native(c.scene, c.cams[0], **c.run_kw())])


def test_half_empty_scene():
    c = fwd_cases.case("HE")
    _check("HE", [run_native(c.scene, c.cams[0], **c.run_kw())])


@pytest.mark.parametrize("name", ["W5", "W32"])
def test_views_in_one_launch(name):
    """3 cameras composited by one launch (grid row = view); the middle one sees nothing and must be
    exactly background, zero language and zero depth."""
    c = fwd_cases.case(name)
    nats = dgr.render_views_native(_views(c, split=c.split))
    _check(name, nats)
    color, lang, radii, depth, st = nats[c.empty_view]
    assert st.num_rendered == 0 and int(radii.abs().max()) == 0
    bg = torch.tensor(fwd_cases.BG, device=color.device)
    assert torch.equal(color, bg[:, None, None].expand_as(color))
    assert float(lang.abs().max()) == 0.0 and float(depth.abs().max()) == 0.0
