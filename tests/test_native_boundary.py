"""_lib.Boundary: the one place a tensor becomes an address for liblsr.so, and the policy that no other module of the
package takes one.  The refusals are tested on CPU tensors against torch.device("cuda", 0), which needs no GPU."""
import ast
import ctypes
import glob
import os

import pytest
import torch

from diff_gaussian_rasterization import _lib

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "4dlangsplat_amd")
CPU, GPU0 = torch.device("cpu"), torch.device("cuda", 0)
GOOD = torch.arange(12, dtype=torch.float32).reshape(3, 4)
COPIES = ("contiguous", "to", "clone", "float", "double", "half", "int", "long", "cuda", "cpu", "reshape", "flatten")

# (what, tensor or object, dtype the C side reads, device of the call): everything the boundary refuses
REFUSED = [
    ("wrong dtype", GOOD.double(), torch.float32, CPU),
    ("wrong dtype for int32", GOOD, torch.int32, CPU),
    ("non-contiguous", GOOD.t(), torch.float32, CPU),
    ("column slice", GOOD[:, :2], torch.float32, CPU),
    ("another device", GOOD, torch.float32, GPU0),
    ("a list", [1.0, 2.0], torch.float32, CPU),
    ("an address", GOOD.data_ptr(), torch.float32, CPU),
    ("None", None, torch.float32, CPU),
]


@pytest.mark.parametrize("what,t,dtype,device", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals(what, t, dtype, device):
    B = _lib.Boundary(device)
    assert B.ok(t, dtype) is False                     # the predicate is False exactly where ptr() raises
    with pytest.raises(ValueError, match="^gts: contiguous"):
        B.ptr(t, "gts", dtype)
    if t is not None:
        with pytest.raises(ValueError, match="^gts: "):
            B.opt(t, "gts", dtype)


def test_accepts_and_message():
    B = _lib.Boundary(CPU)
    assert B.ok(GOOD) is True and B.ptr(GOOD, "x") == GOOD.data_ptr() == B.opt(GOOD, "x")
    row = GOOD[1:]                                     # the address of a slice, not integer arithmetic
    assert B.ptr(row) == GOOD.data_ptr() + 16
    i32 = torch.zeros(3, dtype=torch.int32)
    assert B.ok(i32, torch.int32) and B.ptr(i32, "seg", torch.int32) == i32.data_ptr()
    assert B.opt(None, "x") is None                    # NULL for an optional argument
    assert _lib.Boundary("cpu").ok(GOOD) and _lib.Boundary("cuda:0").device == GPU0   # a device may be spelled out
    with pytest.raises(ValueError) as e:
        _lib.Boundary(GPU0).ptr(GOOD.double(), "gts")
    assert str(e.value) == "gts: contiguous float32 tensor on cuda:0 required, got float64 on cpu"
    with pytest.raises(ValueError, match="got non-contiguous float32 on cpu"):
        B.ptr(GOOD.t(), "x")
    with pytest.raises(ValueError, match="got NoneType"):
        B.ptr(None, "x")


def test_strided_is_an_opt_in():
    """Entry points that take the strides as arguments of their own: dtype and device are still checked."""
    B = _lib.Boundary(CPU)
    cols = GOOD[:, :2]
    assert not B.ok(cols) and B.ok(cols, strided=True) and B.ptr(cols, "g", strided=True) == GOOD.data_ptr()
    for bad, dev in ((cols.double(), CPU), (cols, GPU0), (None, CPU)):
        assert not _lib.Boundary(dev).ok(bad, strided=True)
        with pytest.raises(ValueError, match="^g: float32 tensor on"):
            _lib.Boundary(dev).ptr(bad, "g", strided=True)


def test_array():
    B = _lib.Boundary(CPU)
    ts = [GOOD, GOOD[1:], GOOD[2:]]
    arr = B.array(ts, "images")
    assert isinstance(arr, ctypes.c_void_p * 3) and list(arr) == [t.data_ptr() for t in ts]
    assert len(B.array([], "images")) == 0
    for bad in (GOOD.double(), GOOD.t(), None, 7):
        with pytest.raises(ValueError, match=r"^images\[1\]: contiguous float32"):
            B.array([GOOD, bad, GOOD], "images")
    with pytest.raises(ValueError, match=r"^images\[0\]: .* on cuda:0 required, got float32 on cpu"):
        _lib.Boundary(GPU0).array(ts, "images")


class _FakeStream:
    """What Boundary.stream reads of a torch stream."""

    def __init__(self, device, handle):
        self.device, self.cuda_stream = device, handle


def test_stream_of_another_device_is_refused():
    B = _lib.Boundary(GPU0)
    st = B.stream(_FakeStream(GPU0, 0x1234))
    assert isinstance(st, ctypes.c_void_p) and st.value == 0x1234
    with pytest.raises(ValueError, match="stream: a stream of cuda:0 required, got one of cuda:1"):
        B.stream(_FakeStream(torch.device("cuda", 1), 0x1234))


def _is_compared(node, parents):
    p = parents[node]
    return isinstance(p, ast.Compare) and (node is p.left or any(node is c for c in p.comparators))


def test_only_lib_takes_addresses():
    """No module but _lib.py calls .data_ptr() (except to compare two tensors' storage) or keeps a pointer or stream
    helper of its own: what may cross the ctypes boundary is decided in one place."""
    offences = []
    files = sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))
    assert len(files) >= 18, files
    for path in files:
        if os.path.basename(path) == "_lib.py":
            continue
        tree = ast.parse(open(path).read(), path)
        parents = {c: p for p in ast.walk(tree) for c in ast.iter_child_nodes(p)}
        for node in ast.walk(tree):
            where = f"{os.path.relpath(path, PKG)}:{getattr(node, 'lineno', 0)}"
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "data_ptr" \
                    and not _is_compared(node, parents):
                offences.append(where + ": .data_ptr()")
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.args \
                    and node.func.attr in ("ptr", "opt", "array"):
                # a copy made inside the argument dies when the boundary returns: the address would dangle
                offences += [f"{where}: .{c.func.attr}() inside a boundary argument" for c in ast.walk(node.args[0])
                             if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute)
                             and c.func.attr in COPIES]
            names = []
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                names = [node.name]
            elif isinstance(node, ast.Assign):
                names = [t.id for t in node.targets if isinstance(t, ast.Name)]
            offences += [f"{where}: defines {n}" for n in names
                         if n in ("_ptr", "_vp", "_pointers", "_ptr_array", "_stream")]
    assert not offences, offences
