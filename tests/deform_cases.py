"""The cases of tests/test_deform_branches_gpu.py and tests/test_deform_check.py: which instantiation
of the deformation field's kernels each one reaches, its seeded inputs, and its reference (the
oracle with the kernels' float32 coordinate decisions, and the term scales of deform_check).

Every case: tiny planes (RES, times the scale's multires), seeded random parameters (the golden
variants: their fixture's), train_aabb on.  Of the points, every fourth lies exactly on grid lines
of one scale (each coordinate on a line of its own), every 16th on faces of the box, the others
uniformly in the box grown by 15 % (so some outside); of the times a third is +1, a third -1, the
rest uniform in [-1.2, 1.2] (the time-row case has its own).  No 1e-3-cell exclusion: the reference
shares the kernels' cells.

Tile regimes.  launch_head_wgrad (csrc/deform_wgrad.hip) gives a block of k_head_wgrad3 / k_head_wgrad2
    rows_per_block = max(64, ceil(ceil(P / nb) / 64) * 64),   T = rows_per_block / 64 tiles
with nb = 256 / ns / 8 * 8 for ns <= 4 small heads (64 for four, 256 for one) and nb = max(8,
256 / nbig / 8 * 8) = 256 for the one SH head; lsr_deform_backward gives k_atb
    rows_per_block = max(64, ceil(ceil(P / 1024) / 64) * 64).
The tile cases state T3 / T2 / atb (tiles of k_head_wgrad3, of k_head_wgrad2, rows of k_atb);
test_deform_check.py recomputes them from these formulas.  They run with row-window upstreams
(nonzero only in the first tile of every k_head_wgrad3 block, only in its last tile, only in the
array's last row), so that a tile dropped or read twice changes a gradient by its whole value; the
reference is computed on the window's rows alone (a row with zero upstream adds exactly nothing);
up to FULL_MAX_P rows they also run with the full upstream, which reaches the middle tiles.

Cases with more than one feature_out layer: _bound_the_chain keeps the term scale near the value
through the layers after the first, so that the check bites there too."""
import ast
import functools
import os

import numpy as np

from deform_oracle import DeformConfig, DeformOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = [6, 5, 4, 7]
COMBOS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
HEADS = ("pos_deform", "scales_deform", "rotations_deform", "opacity_deform", "shs_deform")
HEAD_OUT = (3, 3, 4, 1, 48)
KEYS = ("means3D", "scales", "rotations", "opacity", "shs")
ALL, SMALL, SH_ONLY, ONE_SMALL = (1, 1, 1, 1, 1), (1, 1, 1, 1, 0), (0, 0, 0, 0, 1), (0, 0, 1, 0, 0)
WINDOWS = ("first_tile", "last_tile", "last_row")
FULL_MAX_P = 12300   # tile cases up to this size also run with the full upstream (the middle tiles)
KINK = 1e-4          # |pre-activation| below which a Gaussian's upstream is zeroed in both runs
KINK_CAP = 0.5       # at most this share of a case's Gaussians (what the existing tests assert)


def _case(S, P, depth=0, heads=ALL, rot=False, shape=(16, 128), calls=1, times="thirds", variant=None, seed=0,
          T3=1, T2=1, atb=64, runs=""):
    return dict(S=S, P=P, depth=depth, heads=tuple(bool(h) for h in heads), rot=rot, shape=shape, calls=calls,
                times=times, variant=variant, seed=seed, T3=T3, T2=T2, atb=atb, runs=runs)


CASES = {}
# k_deform_fwd<S, GRAD = false> and k_deform_bwd_a<S, DEEP = false> for S = 1..4, at one Gaussian, a full
# block of 64 rows, one row past it and a ragged tail
for _S in (1, 2, 3, 4):
    for _P in (1, 64, 65, 300):
        CASES[f"S{_S}_P{_P}"] = _case(_S, _P, seed=10 * _S + _P + 1, calls=2 if _P == 65 else 1,
                                      runs=f"k_deform_fwd<{_S},false>, k_deform_bwd_a<{_S},false>")
# k_deform_bwd_a<S, DEEP = true> (more than one feature_out layer) at every scale count, and the depths the
# ABI allows beside 2; depth 1 is depth 0's instantiation (one layer)
CASES["depth1_S2"] = _case(2, 130, depth=1, seed=21, runs="k_deform_bwd_a<2,false>, depth 1")
CASES["depth3_S1"] = _case(1, 130, depth=3, seed=23, runs="k_deform_bwd_a<1,true>, depth 3")
CASES["depth4_S2"] = _case(2, 130, depth=4, seed=24, calls=2,
                           runs="k_deform_bwd_a<2,true>, depth 4; k_atb with 4 feature_out jobs")
CASES["depth3_S3"] = _case(3, 67, depth=3, seed=25, runs="k_deform_bwd_a<3,true>")
CASES["depth4_S4"] = _case(4, 67, depth=4, seed=26, runs="k_deform_bwd_a<4,true>")
# launch_head_wgrad's runs
CASES["small_heads_only"] = _case(2, 300, heads=SMALL, seed=31, runs="nbig = 0: k_head_wgrad3 alone")
CASES["sh_head_only"] = _case(2, 300, heads=SH_ONLY, seed=32, runs="ns = 0: k_head_wgrad2 alone")
CASES["one_small_head"] = _case(1, 300, heads=ONE_SMALL, seed=33, runs="ns = 1: nb = 256")
# apply_rotation: the backward sends the upstream through k_deform_fwd<S, GRAD = true> (quat_grad writes the
# rotation head's upstream sG_rot); S = 3 with GRAD also by variant_discrete (discrete_grad)
CASES["apply_rotation"] = _case(2, 300, heads=ALL, rot=True, seed=34, calls=2, runs="k_deform_fwd<2,true>")
CASES["apply_rotation_deep"] = _case(1, 130, depth=3, heads=(1, 0, 1, 0, 1), rot=True, seed=35,
                                     runs="k_deform_fwd<1,true>, k_deform_bwd_a<1,true>")
CASES["apply_rotation_S3"] = _case(3, 65, heads=(0, 1, 1, 0, 0), rot=True, seed=36, runs="k_deform_fwd<3,true>; ns = 2")
CASES["apply_rotation_S4"] = _case(4, 130, heads=(1, 1, 1, 0, 0), rot=True, seed=37, runs="k_deform_fwd<4,true>; ns = 3")
# the golden variants' parameters: k_lang_deform_*, the coff head, k_atb with lang_dim rows
for _v in ("lang", "noresnet", "discrete"):
    CASES["variant_" + _v] = _case(0, 300, variant=_v, seed=40, runs="k_lang_deform_* / coff head / k_atb M = lang_dim")
# time rows: 70 blocks (blockIdx % 2, % 32 and % 64 all wrap); waves of 16 Gaussians all at time[0]
# (the x-row branch), mixed, elsewhere, back at time[0], and a ragged last wave at time[0]
CASES["time_rows"] = _case(2, 70 * 64 - 7, heads=SMALL, times="waves", seed=50, T3=2,
                           runs="x-row and four-tap scatters, plane replicas, time-row copies, box slots")
# tile regimes (four small heads + SH)
CASES["tiles_T2"] = _case(2, 4097, seed=61, T3=2, runs="k_head_wgrad3 T = 2, a last block of one row")
CASES["tiles_T3"] = _case(2, 8200, seed=62, T3=3, runs="k_head_wgrad3 T = 3, ragged")
CASES["tiles_T4"] = _case(2, 12300, seed=63, T3=4, runs="k_head_wgrad3 T = 4")
# (a seed whose last row has no ReLU input within KINK of zero: the last-row window keeps its row)
CASES["tiles_wgrad2_T3"] = _case(1, 33000, seed=66, T3=9, T2=3, runs="k_head_wgrad2 T = 3")
CASES["tiles_atb128"] = _case(1, 65700, depth=2, seed=65, T3=17, T2=5, atb=128,
                              runs="k_atb at 128 rows per block, K = 16 and K = 128 jobs")
TILE_CASES = tuple(k for k in CASES if k.startswith("tiles_"))
# the 32 / 64 shape with on-line and on-face points
CASES["narrow_on_lines"] = _case(2, 130, depth=1, shape=(32, 64), seed=70, calls=2, runs="deform_narrow.hip")
PLAIN_CASES = tuple(k for k in CASES if k not in TILE_CASES)
CPU_CASES = tuple(k for k in CASES if CASES[k]["P"] <= 12300)     # the emulation runs these


def tiles(P, ns, nbig):
    """(T of k_head_wgrad3, T of k_head_wgrad2, k_atb rows per block) of a call with ns heads of at
    most 4 outputs and nbig wider ones, by the launchers' formulas (the module docstring quotes them)."""
    ceil = lambda a, b: (a + b - 1) // b   # noqa: E731
    rpb = lambda nb: max(64, ceil(ceil(P, nb), 64) * 64)   # noqa: E731
    t3 = rpb(256 // ns // 8 * 8 if ns <= 4 else 32) // 64 if ns else 0
    t2 = rpb(max(8, 256 // nbig // 8 * 8)) // 64 if nbig else 0
    return t3, t2, max(64, ceil(ceil(P, 1024), 64) * 64)


def _variant(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "deform_variants.npz"))
    pre = name + "/"
    cfg = ast.literal_eval(str(z[pre + "config"]))
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    return cfg, d


def _f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


def _bound_the_chain(params, cfg, aabb, means3D, times):
    """The feature_out layers after the first of a deep case, rewritten in place so that the term scale
    stays within a small factor of the value through the chain (layers of mixed signs widen it about
    tenfold each, and at depth 4 the check then sees nothing): the drawn weights as magnitudes, scaled
    so that a layer keeps the mean activation; every eighth unit's bias set to minus the median of its
    pre-activation over the case's Gaussians, so that the ReLU masks still cut (about half of those
    units per Gaussian).  The first layer and the heads stay of mixed sign, as at depth 0."""
    o = DeformOracle(params, aabb, cfg=cfg, coords="float32")
    a = np.maximum(o._lin("feature_out.0", o.features(means3D, times)[0]), 0.0)
    for k in range(1, cfg.depth):
        w = np.abs(params[f"feature_out.{2 * k}.weight"])
        w = _f32(w * (a.mean() / (a.mean(0) @ w.T).mean()))
        b = params[f"feature_out.{2 * k}.bias"].copy()
        b[::8] = -np.median(a @ w.T, axis=0)[::8]
        params[f"feature_out.{2 * k}.weight"], params[f"feature_out.{2 * k}.bias"] = w, _f32(b)
        a = np.maximum(a @ w.T + params[f"feature_out.{2 * k}.bias"], 0.0)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(cfg, res, multires, params, aabb, inp, lang, times, ups): float64 arrays holding float32 values."""
    c = CASES[name]
    rng = np.random.default_rng(1000 + c["seed"])
    P = c["P"]
    C, Wd = c["shape"]
    if c["variant"]:
        gc, d = _variant(c["variant"])
        res, multires = list(gc["res"]), list(gc["multires"])
        cfg = DeformConfig.from_golden(gc)
        params = {k[len("param/"):]: v.astype(np.float64) for k, v in d.items() if k.startswith("param/")}
        aabb = d["aabb"].astype(np.float64)
    else:
        res, multires = RES, [1, 2, 4, 8][:c["S"]]
        cfg = DeformConfig(n_scales=c["S"], depth=c["depth"], heads=c["heads"], apply_rotation=c["rot"])
        params = {}
        for s, m in enumerate(multires):
            rs = [r * m for r in res[:3]] + [res[3]]
            for ci, (c0, c1) in enumerate(COMBOS):
                params[f"grid.grids.{s}.{ci}"] = rng.uniform(0.1, 1.5, size=(1, C, rs[c1], rs[c0]))
        wsc = 0.1 if Wd == 128 else 0.15
        for k in range(max(c["depth"], 1)):
            params[f"feature_out.{2 * k}.weight"] = rng.normal(scale=0.2 if k == 0 else wsc,
                                                               size=(Wd, C * c["S"] if k == 0 else Wd))
            params[f"feature_out.{2 * k}.bias"] = rng.normal(scale=0.05, size=Wd)
        for hname, n, on in zip(HEADS, HEAD_OUT, c["heads"]):
            if on:
                params[hname + ".1.weight"] = rng.normal(scale=wsc, size=(Wd, Wd))
                params[hname + ".1.bias"] = rng.normal(scale=0.05, size=Wd)
                params[hname + ".3.weight"] = rng.normal(scale=wsc, size=(n, Wd))
                params[hname + ".3.bias"] = rng.normal(scale=0.05, size=n)
        params = {k: _f32(v) for k, v in params.items()}
        aabb = _f32([[1.5, 1.2, 3.0], [-1.4, -1.1, 0.5]])
    a0, a1 = aabb[0], aabb[1]                                    # [max, min]
    lo, hi = a1, a0
    ext = 0.15 * (hi - lo)
    pts = rng.uniform(lo - ext, hi + ext, size=(P, 3))
    r3 = np.array(res[:3])
    for g in range(0, P, 4):                                     # on grid lines of one scale
        m = multires[(g // 4) % len(multires)]
        k = rng.integers(0, r3 * m)                              # a line index per coordinate
        pts[g] = a0 + (2.0 * k / (r3 * m - 1)) * (a1 - a0) / 2.0
    for g in range(2, P, 16):                                    # on faces of the box
        face = rng.integers(0, 2, size=3)
        on = rng.integers(0, 2, size=3).astype(bool) | (np.arange(3) == (g // 16) % 3)
        pts[g] = np.where(on, np.where(face, a0, a1), pts[g])
    if P == 1:
        pts[0, 0] = a1[0]                                        # the one Gaussian: on a line and on a face
    times = rng.uniform(-1.2, 1.2, size=P)
    if c["times"] == "thirds":
        times[::3] = 1.0
        times[1::3] = -1.0
    else:                                                        # "waves": by the wave's index (16 Gaussians)
        t0 = -1.0 / 3.0                                          # time[0]: on a time line of RES[3] = 7
        w = np.arange(P) // 16
        kind = w % 4                                             # 0, 3: at time[0]; 1: mixed; 2: elsewhere
        times[(kind == 0) | (kind == 3)] = t0
        times[(kind == 1) & (np.arange(P) % 2 == 0)] = t0
        times[(kind == 2) & (np.arange(P) % 3 == 0)] = 1.0
        times[(kind == 2) & (np.arange(P) % 3 == 1)] = -1.0
        times[w == w[-1]] = t0                                   # the ragged last wave
    if not c["variant"] and c["depth"] >= 2:
        _bound_the_chain(params, cfg, aabb, _f32(pts), _f32(times).reshape(P, 1))
    inp = dict(means3D=pts, scales=rng.normal(-4, 0.5, size=(P, 3)), rotations=rng.normal(size=(P, 4)),
               opacity=rng.normal(size=(P, 1)), shs=rng.normal(scale=0.3, size=(P, 16, 3)))
    ups = dict(means3D=rng.normal(size=(P, 3)), scales=rng.normal(size=(P, 3)), rotations=rng.normal(size=(P, 4)),
               opacity=rng.normal(size=(P, 1)), shs=rng.normal(size=(P, 16, 3)) * 0.1)
    lang = None
    if c["variant"]:
        lang = d["lang"].astype(np.float64)
        ups["lang"] = d["up_lang"].astype(np.float64)
        if "up_coff" in d:
            ups["coff"] = d["up_coff"].astype(np.float64)
    return dict(cfg=cfg, res=res, multires=multires, params=params, aabb=aabb, inp={k: _f32(v) for k, v in inp.items()},
                lang=lang, times=_f32(times).reshape(P, 1), ups={k: _f32(v) for k, v in ups.items()})


def windows(name):
    """The upstream windows a case runs with: the whole array (None), and for a tile case the three
    windows; a tile case above FULL_MAX_P rows runs the windows alone."""
    if name not in TILE_CASES:
        return (None,)
    return WINDOWS + ((None,) if CASES[name]["P"] <= FULL_MAX_P else ())


def window_rows(name, window):
    """The rows with a nonzero upstream: all of them (window None), or of every k_head_wgrad3 block
    its first tile / its last tile, or the array's last row."""
    c = CASES[name]
    P = c["P"]
    if window is None:
        return np.arange(P)
    if window == "last_row":
        return np.array([P - 1])
    rpb = 64 * c["T3"]
    g = np.arange(P)
    row0 = g // rpb * rpb
    if window == "first_tile":
        return g[g - row0 < 64]
    n = np.minimum(P, row0 + rpb) - row0                         # rows of the block
    return g[(g - row0) // 64 == (n - 1) // 64]


@functools.lru_cache(maxsize=None)
def reference(name, window=None, products="float64", coords="float32", drop_lo_hi=None):
    """The oracle on the case's window rows, kink-masked: dict(rows, amb, ups (the masked upstream of
    those rows), out, A_out, g_in, g, A_in, A_g); gradients and scales of ONE call.  Cached: the
    tests share it and leave it unchanged."""
    x = inputs(name)
    rows = window_rows(name, window)
    o = DeformOracle(x["params"], x["aabb"], cfg=x["cfg"], coords=coords, products=products, drop_lo_hi=drop_lo_hi,
                     train_aabb=True)
    inp = [x["inp"][k][rows] for k in KEYS]
    lang = None if x["lang"] is None else x["lang"][rows]
    out, A_out = o.forward(*inp, lang, x["times"][rows], abs_terms=True)
    amb = kink_rows(name, window)
    ups = {k: v[rows].copy() for k, v in x["ups"].items()}
    for v in ups.values():
        v[amb] = 0.0
    g_in, g, A_in, A_g = o.backward(*[ups[k] for k in KEYS], up_lang=ups.get("lang"), up_coff=ups.get("coff"),
                                    abs_terms=True)
    return dict(rows=rows, amb=amb, ups=ups, out=out, A_out=A_out, g_in=g_in, g=g, A_in=A_in, A_g=A_g)


@functools.lru_cache(maxsize=None)
def kink_rows(name, window=None):
    """Of the window's rows, those with a ReLU input within KINK of zero in the float32-coordinate
    float64 oracle (the language columns of the lang_deform input reach the kernels exactly and are
    left out, as test_deform_gpu._kink_masked_oracle)."""
    x = inputs(name)
    rows = window_rows(name, window)
    o = DeformOracle(x["params"], x["aabb"], cfg=x["cfg"], coords="float32")
    o.forward(*[x["inp"][k][rows] for k in KEYS], None if x["lang"] is None else x["lang"][rows], x["times"][rows])
    zs = o.preactivations()
    if x["cfg"].lang_mode in ("residual", "noresnet"):
        zs[-3] = zs[-3][:, x["lang"].shape[1]:]
    amb = np.zeros(len(rows), bool)
    for v in zs:
        amb |= (np.abs(v) < KINK).any(axis=1)
    return amb


def offsets(name, out, rows):
    """What the kernels compute of forward outputs `out` (a dict under the oracle's names, the rows
    `rows` of the case): the residual outputs minus their inputs; the rotations under apply_rotation,
    the language and coff as they are; an absent output is left out."""
    x = inputs(name)
    res = {}
    for k, v in out.items():
        if v is None:
            continue
        v = np.asarray(v, np.float64)
        if k in ("lang", "coff") or (k == "rotations" and x["cfg"].apply_rotation and x["cfg"].heads[2]):
            res[k] = v
        else:
            res[k] = v.reshape(x["inp"][k][rows].shape) - x["inp"][k][rows]
    return res
