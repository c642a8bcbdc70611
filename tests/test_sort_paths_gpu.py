"""Every path of the device scan and radix sort (sort.hip) against host references on exact
integer data: tests/kernels/t_sort_paths.hip, one test per group of cases, and the program's
self-test of its own checkers (no device call)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sort_paths_exe(tmp_path_factory):
    """The program, compiled once per module with test_radix_sort's flags."""
    src = os.path.join(ROOT, "tests", "kernels", "t_sort_paths.hip")
    exe = str(tmp_path_factory.mktemp("sort_paths") / "t_sort_paths")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "4dlangsplat_amd", "csrc"), "-o", exe, src], check=True)
    return exe


def test_sort_paths_selftest(sort_paths_exe):
    """The checkers accept a correct simulated output and reject each single corruption (swapped
    equal-key values, scan off by one, wrong total, kept off by one, a written tail or guard word,
    wrong or spurious ranges, a rectangle from the wrong id)."""
    r = subprocess.run(["timeout", "-k", "5", "120", sort_paths_exe, "--selftest"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


def _run_group(exe, group):
    r = subprocess.run(["timeout", "-k", "5", "120", exe, group], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_scan(sort_paths_exe):
    """exclusive_scan_u32: one tile, the folded two-kernel path, the recursive path; 16-byte and
    scalar loads / stores; with and without total."""
    _run_group(sort_paths_exe, "scan")


@pytest.mark.gpu
def test_scan_batch(sort_paths_exe):
    """exclusive_scan_batch: unequal segments, host_total words and the returned mask."""
    _run_group(sort_paths_exe, "scan_batch")


@pytest.mark.gpu
def test_sort_host_plan(sort_paths_exe):
    """radix_sort_pairs, host-planned: block-edge sizes, bit windows, key patterns, dropped keys."""
    _run_group(sort_paths_exe, "host_plan")


@pytest.mark.gpu
def test_sort_ranges(sort_paths_exe):
    """The last pass's per-key ranges: runs across blocks, keys at or above nranges, unused keys."""
    _run_group(sort_paths_exe, "ranges")


@pytest.mark.gpu
def test_sort_depth_plan(sort_paths_exe):
    """The device-planned depth sort: both plans and their boundary, kept, gather, stability."""
    _run_group(sort_paths_exe, "depth_plan")


@pytest.mark.gpu
def test_sort_batch(sort_paths_exe):
    """radix_sort_batch: unequal and empty segments, both plans in one batch, the refusals."""
    _run_group(sort_paths_exe, "batch")
