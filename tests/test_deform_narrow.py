"""The deformation field's second shape, net_width 64 / output_coordinate_dim 32 (the reference's D-NeRF
configs and its ModelHiddenParams defaults), without a GPU: the float64 oracle against the reference
module's outputs and autograd (tests/golden/deform_narrow_{variant}.npz, made by
tests/golden/make_deform_narrow_golden.py), and what DeformationField accepts and refuses."""
import ast
import json
import os

import numpy as np
import pytest
import torch

from deform_oracle import DeformConfig, DeformOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VARIANTS = ("dnerf", "defaults", "full")
OUTS = ("means3D", "scales", "rotations", "opacity", "shs", "lang", "coff")
PRE = "deformation_net."


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


_cache = {}


def load_variant(name):
    """One variant: (golden config, DeformConfig, params, parameter gradients, every array).  An array
    the file stores once under another key ("aliases": the output of a head that is off, the input
    gradient of an identity residual) is restored under its own."""
    if name not in _cache:
        z = np.load(os.path.join(GOLDEN, f"deform_narrow_{name}.npz"))
        pre = name + "/"
        d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        for k, twin in ast.literal_eval(str(z["aliases"])).items():
            d[k[len(pre):]] = d[twin[len(pre):]]
        cfg = ast.literal_eval(str(d["config"]))
        params = {k[len("param/"):]: v for k, v in d.items() if k.startswith("param/")}
        grads = {k[len("grad/"):]: v for k, v in d.items() if k.startswith("grad/")}
        _cache[name] = (cfg, DeformConfig.from_golden(cfg), params, grads, d)
    return _cache[name]


def test_variants_have_the_narrow_shape_and_cover_border_and_time():
    want = {"dnerf": ([1, 2], 0, 3, False), "defaults": ([1, 2, 4, 8], 1, 3, False), "full": ([1, 2], 2, 5, True)}
    for name in VARIANTS:
        cfg, _, params, _, d = load_variant(name)
        multires, depth, heads, rot = want[name]
        assert (cfg["multires"], cfg["depth"], cfg["apply_rotation"], cfg["no_dlang"]) == (multires, depth, rot, 1)
        assert params["feature_out.0.weight"].shape == (64, 32 * len(multires))
        assert params["grid.grids.0.0"].shape[:2] == (1, 32)
        assert sum(k.endswith(".3.weight") for k in params) == heads
        assert len(set(cfg["res"])) == 4 and d["means3D"].shape[0] == 300
        a0, a1 = d["aabb"]
        pn = (d["means3D"] - a0) * (2.0 / (a1 - a0)) - 1.0
        assert (np.abs(pn) > 1).any(axis=1).sum() > 20
        assert len(np.unique(d["time"])) > 10 and (np.abs(d["time"]) > 1).any()


@pytest.mark.parametrize("name", VARIANTS)
def test_oracle_matches_reference_at_the_narrow_shape(name):
    """The unchanged oracle at 32 channels / width 64: outputs, input gradients and parameter
    gradients of the reference's autograd (the bounds of test_oracle_matches_reference_variant)."""
    cfg, dc, params, grads, d = load_variant(name)
    o = DeformOracle(params, d["aabb"], cfg=dc)
    f64 = lambda k: d[k].astype(np.float64)   # noqa: E731
    out = o.forward(f64("means3D"), f64("scales"), f64("rotations"), f64("opacity"), f64("shs"), f64("lang"),
                    f64("time"))
    for k in OUTS:
        if "out_" + k in d:
            assert _rel(out[k], d["out_" + k]) < 1e-6, k
    g_in, g = o.backward(*[f64("up_" + k) for k in OUTS[:5]], up_lang=f64("up_lang"), up_coff=None)
    for k in ("means3D", "scales", "rotations", "opacity", "shs", "lang"):
        assert _rel(g_in[k].reshape(d["grad_" + k].shape), d["grad_" + k]) < 1e-5, k
    assert set(g) == set(grads), set(g) ^ set(grads)
    for k, v in grads.items():
        assert _rel(g[k].reshape(v.shape), v) < 1e-5, k


# ---- what DeformationField accepts and refuses ---------------------------------------------------
DNERF = dict(kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32,
                             "resolution": [64, 64, 64, 75]},
             multires=[1, 2], defor_depth=0, net_width=64, plane_tv_weight=0.0002)   # arguments/dnerf/*.py
# the ModelHiddenParams defaults with net_width / output_coordinate_dim left to the code's defaults
DEFAULTS = dict(kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "resolution": [64, 64, 64, 25]})
ENV = {"language_feature_hiddendim": "3"}


@pytest.fixture(scope="module")
def layout():
    with open(os.path.join(GOLDEN, "deform_narrow_state_dict_layout.json")) as f:
        return json.load(f)


def _zeros(layout, name):
    return {k: torch.zeros(s) for k, s in layout[name].items()}


def _heads(params):
    return sorted({k.split(".")[0] for k in params if not k.startswith(("grid", "feature_out"))})


def test_config_from_reference_accepts_dnerf_and_the_defaults(layout):
    from deformation import DeformationField, LANG_PASS
    for name, hidden, scales, depth in (("dnerf", DNERF, 2, 0), ("defaults", DEFAULTS, 4, 1)):
        sd = _zeros(layout, name)
        params, cfg = DeformationField.config_from_reference(sd, hidden, env=ENV)
        assert params["feature_out.0.weight"].shape == (64, 32 * scales)           # width 64, 32 channels
        assert params["grid.grids.0.0"].shape[1] == 32
        assert len(cfg["multires"]) == scales and cfg["depth"] == depth and cfg["lang_mode"] == LANG_PASS
        assert _heads(params) == ["pos_deform", "rotations_deform", "scales_deform"]   # no_do, no_dshs default
        assert len([k for k in params if k.startswith("grid.grids")]) == 6 * scales and "grid.aabb" in params
        assert set(PRE + k for k in params) <= set(sd)
    # an object with attributes, as the reference passes its ModelHiddenParams
    from argparse import Namespace
    _, cfg = DeformationField.config_from_reference(_zeros(layout, "dnerf"), Namespace(**DNERF), env=ENV)
    assert cfg["multires"] == [1, 2] and cfg["resolution"] == [64, 64, 64, 75]


def test_config_from_reference_stays_strict(layout):
    from deformation import DeformationField
    sd = _zeros(layout, "dnerf")
    cfr = DeformationField.config_from_reference
    kp = DNERF["kplanes_config"]
    with pytest.raises(ValueError, match="net_width"):          # (16, 64)
        cfr(sd, dict(DNERF, kplanes_config=dict(kp, output_coordinate_dim=16)), env=ENV)
    with pytest.raises(ValueError, match="net_width"):          # (32, 128)
        cfr(sd, dict(DNERF, net_width=128), env=ENV)
    # a 128-wide state dict declared as 64, and 16-channel planes declared as 32
    wide = dict(sd, **{PRE + "feature_out.0.weight": torch.zeros(128, 64)})
    with pytest.raises(ValueError, match="feature_out.0.weight"):
        cfr(wide, DNERF, env=ENV)
    thin = dict(sd, **{PRE + "grid.grids.0.0": torch.zeros(1, 16, 64, 64)})
    with pytest.raises(ValueError, match="grid.grids.0.0"):
        cfr(thin, DNERF, env=ENV)
    for bad in ("static_mlp", "empty_voxel", "no_grid"):
        with pytest.raises(ValueError, match=bad):
            cfr(sd, dict(DNERF, **{bad: True}), env=ENV)
    with pytest.raises(ValueError, match="grid_pe"):
        cfr(sd, dict(DNERF, grid_pe=2), env=ENV)
    with pytest.raises(ValueError, match="use_tribute_dlang"):
        cfr(sd, DNERF, env=dict(ENV, use_tribute_dlang="t"))
    with pytest.raises(ValueError, match="outside"):
        cfr(dict(sd, stray=torch.zeros(1)), DNERF, env=ENV)
    with pytest.raises(ValueError, match="feature_out.2"):      # deeper than the config says
        cfr(dict(sd, **{PRE + "feature_out.2.weight": torch.zeros(64, 64)}), DNERF, env=ENV)


def test_unsupported_language_modes_are_refused_by_name(layout):
    """RESIDUAL, NORESNET and DISCRETE have no kernels at 32 / 64: the message names the mode and the shape."""
    from deformation import DeformationField
    sd = _zeros(layout, "dnerf")
    cfr = DeformationField.config_from_reference
    for hidden, env, mode in ((dict(DNERF, no_dlang=0), ENV, "RESIDUAL"),
                              (dict(DNERF, no_dlang=0), dict(ENV, no_resnet="t"), "NORESNET"),
                              (DNERF, dict(ENV, use_discrete_lang_f="t", centers_num="3"), "DISCRETE")):
        with pytest.raises(ValueError, match=f"{mode}.*32.*64"):
            cfr(sd, hidden, env=env)


def test_init_params_has_the_layouts_computed_path(layout):
    """init_params(channels=32, width=64): the names and shapes of the state dict's computed path (the
    defaults' planes at 1/8 of their base resolution here: 512 x 512 x 32 planes are 100 MB of noise)."""
    from deformation import DeformationField
    heads = ("pos_deform", "scales_deform", "rotations_deform")
    for name, hidden, res, multires, depth in (("dnerf", DNERF, [64, 64, 64, 75], [1, 2], 0),
                                               ("defaults", DEFAULTS, [8, 8, 8, 25], [1, 2, 4, 8], 1)):
        p = DeformationField.init_params(res, multires, [[1, 1, 1], [-1, -1, -1]], channels=32, width=64, depth=depth,
                                         heads=heads)
        want, _ = DeformationField.config_from_reference(_zeros(layout, name), hidden, env=ENV)
        assert set(p) == set(want)
        for k, v in p.items():
            shape = tuple(want[k].shape)
            if name == "defaults" and ".grids." in k:
                shape = shape[:2] + tuple(n if n == 25 else n // 8 for n in shape[2:])
            assert tuple(v.shape) == shape, k
        assert float(p["grid.grids.0.2"].min()) == 1.0 and float(p["grid.grids.0.0"].max()) <= 0.5


def test_hidden_params_round_trip(monkeypatch):
    """hidden_params() of a 32 / 64 field writes its own net_width / output_coordinate_dim, and
    config_from_reference reads them back to the same configuration."""
    from deformation import DeformationField
    p = DeformationField.init_params([4, 3, 2, 5], [1, 2], [[1, 1, 1], [-1, -1, -1]], channels=32, width=64,
                                     heads=("pos_deform", "scales_deform", "rotations_deform"))
    f = DeformationField.__new__(DeformationField)     # the configuration without the device
    f.resolution, f.multires, f.depth, f.apply_rotation, f.lang_mode = [4, 3, 2, 5], [1, 2], 0, False, 0
    f.lang_dim, f.centers, f.time_pe, f.head_on, f.discrete = 3, 0, 4, (True, True, True, False, False), False
    f.channels, f.width = p["grid.grids.0.0"].shape[1], p["feature_out.0.weight"].shape[0]
    h = f.hidden_params()
    assert h["net_width"] == 64 and h["kplanes_config"]["output_coordinate_dim"] == 32
    params, cfg = DeformationField.config_from_reference({PRE + k: v for k, v in p.items()}, h, env=f.env_params())
    assert set(params) == set(p)
    assert (cfg["resolution"], cfg["multires"], cfg["depth"], cfg["no_do"], cfg["no_dshs"], cfg["lang_mode"]) == \
        ([4, 3, 2, 5], [1, 2], 0, True, True, 0)
