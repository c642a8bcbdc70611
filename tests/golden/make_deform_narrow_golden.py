"""Generate tests/golden/deform_narrow_{variant}.npz from the REFERENCE deformation network at its
second shape, net_width 64 / output_coordinate_dim 32 (run in the build container only, as
make_deform_variants_golden.py: it imports the reference).  Same contents per variant as make_deform_variants_golden.py, whose
make_variant builds them (net_width and kplanes_config overridden through the variant's args):

  dnerf     arguments/dnerf/*.py: multires [1, 2], defor_depth 0, no_do = no_dshs = True
  defaults  the ModelHiddenParams defaults (arguments/__init__.py:84-113, train.py without --configs):
            multires [1, 2, 4, 8], defor_depth 1, three heads
  full      multires [1, 2], defor_depth 2, all five heads, apply_rotation

The language passes through in all three (no_dlang 1).  One file per variant, and an array that
repeats another bit for bit (the output of a head that is off is its input, the input gradient of an
identity residual is its upstream) is stored once: "aliases" maps its key to the stored one
(load_variant resolves them).  Both keep every file under the repository's 1 MiB limit.  The generator
asserts, with the float64 oracle, that fewer than half of each variant's Gaussians have a ReLU input
within 1e-4 of zero (the cap test_deform_narrow_gpu.py puts on its kink masking).

    python tests/golden/make_deform_narrow_golden.py            # deform_narrow_{dnerf,defaults,full}.npz
    python tests/golden/make_deform_narrow_golden.py --layout   # deform_narrow_state_dict_layout.json
"""
import ast
import json
import os
import sys
from argparse import Namespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_deform_variants_golden as base   # noqa: E402

OUT = os.path.join(HERE, "deform_narrow_{}.npz")
RES = [4, 3, 2, 5]            # x, y, z, t plane resolution: distinct per axis, small
NARROW = dict(net_width=64, kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4,
                                            "output_coordinate_dim": 32, "resolution": list(RES)})
VARIANTS = {
    "dnerf": dict(args=dict(NARROW, multires=[1, 2], defor_depth=0, no_do=True, no_dshs=True, no_dlang=1),
                  env=dict(language_feature_hiddendim="3")),
    "defaults": dict(args=dict(NARROW, multires=[1, 2, 4, 8], defor_depth=1, no_do=True, no_dshs=True, no_dlang=1),
                     env=dict(language_feature_hiddendim="3")),
    "full": dict(args=dict(NARROW, multires=[1, 2], defor_depth=2, no_do=False, no_dshs=False, no_dlang=1,
                           apply_rotation=True),
                 env=dict(language_feature_hiddendim="3")),
}
SEEDS = {"dnerf": 100, "defaults": 110, "full": 120}


def kink_share(d, name):
    """Share of the variant's Gaussians with a ReLU input within 1e-4 of zero (the float64 oracle)."""
    from deform_oracle import DeformConfig, DeformOracle
    pre = name + "/"
    cfg = ast.literal_eval(str(d[pre + "config"]))
    params = {k[len(pre + "param/"):]: v for k, v in d.items() if k.startswith(pre + "param/")}
    o = DeformOracle(params, d[pre + "aabb"], cfg=DeformConfig.from_golden(cfg))
    f64 = lambda k: d[pre + k].astype(np.float64)   # noqa: E731
    o.forward(*[f64(k) for k in ("means3D", "scales", "rotations", "opacity", "shs", "lang", "time")])
    amb = np.zeros(d[pre + "means3D"].shape[0], bool)
    for v in o.preactivations():
        amb |= (np.abs(v) < 1e-4).any(axis=1)
    return float(amb.mean())


def dedupe(d):
    """d without the arrays that repeat an earlier one bit for bit, plus "aliases" (repr of a dict)."""
    kept, aliases = {}, {}
    for k, v in d.items():
        twin = next((k2 for k2, v2 in kept.items() if v2.dtype == v.dtype and v2.shape == v.shape and v.size > 64 and
                     np.array_equal(v2, v)), None)
        if twin is None:
            kept[k] = v
        else:
            aliases[k] = twin
    kept["aliases"] = np.array(repr(aliases))
    return kept


def load_variant(name, folder=HERE):
    """The variant's arrays under their names without the variant prefix, aliases resolved."""
    z = np.load(OUT.format(name).replace(HERE, folder))
    pre = name + "/"
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    for k, twin in ast.literal_eval(str(z["aliases"])).items():
        d[k[len(pre):]] = d[twin[len(pre):]]
    return d


def state_dict_layout(deform_network):
    """Keys and shapes of deform_network(...).state_dict() for a D-NeRF config and for the
    ModelHiddenParams defaults (every module the reference builds, computed or not)."""
    out = {}
    common = dict(net_width=64, timebase_pe=4, posebase_pe=10, scale_rotation_pe=2, opacity_pe=2, timenet_width=64,
                  timenet_output=32, bounds=1.6, no_dx=False, no_grid=False, no_ds=False, no_dr=False, no_do=True,
                  no_dshs=True, no_dlang=1, empty_voxel=False, grid_pe=0, static_mlp=False, apply_rotation=False)
    kp = lambda res: {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32,   # noqa: E731
                      "resolution": res}
    for name, args in (("dnerf", dict(multires=[1, 2], defor_depth=0, kplanes_config=kp([64, 64, 64, 75]))),
                       ("defaults", dict(multires=[1, 2, 4, 8], defor_depth=1, kplanes_config=kp([64, 64, 64, 25])))):
        os.environ["language_feature_hiddendim"] = "3"
        net = deform_network(Namespace(**dict(common, **args)))
        out[name] = {k: list(v.shape) for k, v in net.state_dict().items()}
    path = os.path.join(HERE, "deform_narrow_state_dict_layout.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", path)


def main():
    deform_network = base._import_reference()
    if "--layout" in sys.argv:
        state_dict_layout(deform_network)
        return
    base.RES = list(RES)      # make_variant records it as the variant's config["res"]
    for name, spec in VARIANTS.items():
        d, used = base.make_variant(deform_network, name, spec, seed=SEEDS[name])
        assert d[name + "/param/feature_out.0.weight"].shape == (64, 32 * len(spec["args"]["multires"]))
        share = kink_share(d, name)
        print(f"{name}: {used} parameter tensors on the path, kink share {share:.3f}")
        assert share < 0.5, (name, share)
        np.savez_compressed(OUT.format(name), **dedupe(d))
        size = os.path.getsize(OUT.format(name))
        print("wrote", OUT.format(name), size, "bytes")
        assert size < 1 << 20
        back = load_variant(name)
        assert all(np.array_equal(back[k[len(name) + 1:]], v) for k, v in d.items())


if __name__ == "__main__":
    main()
