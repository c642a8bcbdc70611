"""The deformation field's workspace and backward-scratch sizes, without a GPU: lsr_deform_workspace_bytes
and lsr_deform_backward_scratch_bytes read only the net's integers and check its pointers for null, so
dummy non-null pointers do.  The sizes are the host-side layout both shapes share (csrc/deform_host.h:
plane pairs, plane sizes, 256-byte alignment, layers, head mask); every expected number below is what a
build of commit 07a276d (the last with one layout per shape) returned, written down, not recomputed."""
import ctypes

import pytest

from diff_gaussian_rasterization import _lib

PS = (0, 1, 64, 65, 100000)
PASS, RESIDUAL, DISCRETE = 0, 1, 3
SMALL, LARGE = (6, 5, 4, 7), (64, 64, 64, 150)
GEOMETRY = 0b11111   # pos, scales, rotations, opacity, shs


def _net(channels, width, n_scales, depth, res=SMALL, heads=GEOMETRY, apply_rotation=0, lang_mode=PASS, lang_dim=3,
         centers=0, time_pe=4):
    return dict(channels=channels, width=width, n_scales=n_scales, depth=depth, res=res, heads=heads,
                apply_rotation=apply_rotation, lang_mode=lang_mode, lang_dim=lang_dim, centers=centers, time_pe=time_pe)


NETS = {
    **{f"wide-s{s}-d{d}": _net(16, 128, s, d) for s in (1, 2, 4) for d in (0, 2)},
    "wide-pass": _net(16, 128, 2, 1, lang_mode=PASS),
    "wide-residual": _net(16, 128, 2, 1, lang_mode=RESIDUAL),
    "wide-discrete3": _net(16, 128, 2, 1, lang_mode=DISCRETE, centers=3, heads=GEOMETRY | 1 << 5),
    "wide-rot-off": _net(16, 128, 3, 1, apply_rotation=0),
    "wide-rot-on": _net(16, 128, 3, 1, apply_rotation=1),
    "wide-large": _net(16, 128, 2, 1, res=LARGE),
    **{f"narrow-s{s}-d{d}": _net(32, 64, s, d, heads=0b00111) for s in (1, 2, 4) for d in (1, 2)},
    "narrow-rot-on": _net(32, 64, 2, 1, apply_rotation=1),
    "narrow-large": _net(32, 64, 2, 0, res=LARGE, heads=0b00111),
}

# name: (workspace bytes, backward scratch bytes at each P of PS); from a build of commit 07a276d
EXPECTED = {
    "wide-s1-d0": (1019392, (60160, 60160, 128512, 129792, 108858880)),
    "wide-s1-d2": (1150464, (61184, 61184, 194048, 196352, 211258880)),
    "wide-s2-d0": (1060096, (186624, 186624, 259072, 260352, 115385344)),
    "wide-s2-d2": (1191168, (187648, 187648, 324608, 326912, 217785344)),
    "wide-s4-d0": (1552384, (1474304, 1474304, 1554944, 1556224, 129473024)),
    "wide-s4-d2": (1683456, (1475328, 1475328, 1620480, 1622784, 231873024)),
    "wide-pass": (1060096, (186624, 186624, 259072, 260352, 115385344)),
    "wide-residual": (1248512, (189184, 189184, 393984, 397824, 326185472)),
    "wide-discrete3": (1256704, (186624, 186624, 259584, 261120, 116585216)),
    "wide-rot-off": (1187328, (514816, 514816, 591360, 592640, 122113536)),
    "wide-rot-on": (1187328, (514816, 514816, 592128, 593664, 123713280)),
    "wide-large": (10477568, (20109056, 20109056, 20181504, 20182784, 135307776)),
    "narrow-s1-d1": (129536, (29696, 29696, 166656, 168960, 217627392)),
    "narrow-s1-d2": (145920, (30208, 30208, 199424, 202240, 268827392)),
    "narrow-s2-d1": (202496, (94464, 94464, 239616, 241920, 230492160)),
    "narrow-s2-d2": (218880, (94976, 94976, 272384, 275200, 281692160)),
    "narrow-s4-d1": (1137920, (1013760, 1013760, 1175040, 1177600, 257011200)),
    "narrow-s4-d2": (1154304, (1014272, 1014272, 1207808, 1210880, 308211200)),
    "narrow-rot-on": (268032, (95488, 95488, 305920, 309504, 334491904)),
    "narrow-large": (19038208, (18930176, 18930176, 19075328, 19077632, 249327872)),
}


def sizes(cfg):
    """(workspace bytes, [scratch bytes at P for P in PS]) of the net `cfg` describes"""
    lib = _lib.load()
    net = _lib.DeformNet()
    for k in ("channels", "width", "n_scales", "depth", "heads", "apply_rotation", "lang_mode", "lang_dim", "centers",
              "time_pe"):
        setattr(net, k, cfg[k])
    net.res = (ctypes.c_int32 * 4)(*cfg["res"])
    net.multires = (ctypes.c_int32 * 4)(1, 2, 4, 8)
    dummy = 256   # never dereferenced
    net.aabb = dummy
    for s in range(4):
        for ci in range(6):
            net.planes[s][ci] = dummy
    for name, n in (("w_feat", 4), ("b_feat", 4), ("w1", 6), ("b1", 6), ("w2", 6), ("b2", 6), ("w_lang", 3), ("b_lang", 3)):
        for i in range(n):
            getattr(net, name)[i] = dummy
    ref = ctypes.byref(net)
    return int(lib.lsr_deform_workspace_bytes(ref)), [int(lib.lsr_deform_backward_scratch_bytes(ref, P)) for P in PS]


def test_every_listed_net_has_its_numbers():
    assert set(EXPECTED) == set(NETS)
    assert all(len(v[1]) == len(PS) and v[0] > 0 and min(v[1]) > 0 for v in EXPECTED.values())


@pytest.mark.parametrize("name", sorted(NETS))
def test_workspace_and_scratch_bytes_are_the_recorded_ones(name):
    workspace, scratch = sizes(NETS[name])
    assert (workspace, tuple(scratch)) == EXPECTED[name]
