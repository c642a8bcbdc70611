"""bench.py's argument handling (CPU): the --early-views batch list and the number of binning
batches (= compositor launch pairs per step) the timed-region check expects, and the defaults the
driver's plain `python bench.py` run gets."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_early_views_parsing(bench):
    assert bench._early_views("3") == 3
    assert bench._early_views("1,2") == (1, 2)
    assert bench._early_views("2, 3, 3") == (2, 3, 3)
    import argparse
    with pytest.raises(argparse.ArgumentTypeError):
        bench._early_views("-1")
    with pytest.raises(argparse.ArgumentTypeError):
        bench._early_views("")


@pytest.mark.parametrize("early,V,n", [(3, 8, 2), (0, 8, 1), (8, 8, 1), (9, 8, 1), (1, 8, 2), ((1, 2), 8, 3),
                                       ((2, 3), 8, 3), ((2, 3, 3), 8, 3), ((1, 1, 1), 5, 4), ((3, 5), 8, 2)])
def test_binning_batches(bench, early, V, n):
    """Batches: the early views, then side batches of the listed sizes while views remain, then
    the rest (native_view_renderer's cuts)."""
    assert bench._n_binning_batches(early, V) == n


def test_defaults(bench):
    a = bench.parse_args([])
    assert a.gpus == 1 and a.early_views == 2 and a.order_on_side and a.binning == "sort"
    assert a.main_priority == 0 and a.side_priority == 0
    assert not bench.parse_args(["--no-order-on-side"]).order_on_side
    assert bench.parse_args(["--order-on-side"]).order_on_side
    assert bench.parse_args(["--binning", "bucket", "--early-views", "2,3"]).early_views == (2, 3)
    assert not a.full and a.dump_outputs is None
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full and b.dump_outputs == "out"


def test_dump_sample_is_fixed(bench):
    import torch
    assert torch.equal(bench.dump_sample(5, 8, 1), torch.arange(5))
    s = bench.dump_sample(1000, 64, 1)
    assert s.shape == (64,) and bool((s[1:] > s[:-1]).all()) and 0 <= int(s[0]) and int(s[-1]) < 1000
    assert torch.equal(s, bench.dump_sample(1000, 64, 1))
    assert not torch.equal(s, bench.dump_sample(1000, 64, 2))


def test_dump_outputs_files(bench, tmp_path, monkeypatch):
    """The dump of a small bucket and two views: float32 files, the sampled rows / pixels of the
    arrays handed in, the same sample for every field and view."""
    import numpy as np
    import torch
    from view_parallel import GradBucket
    P, M, C, H, W = 300, 16, 4, 6, 10
    monkeypatch.setattr(bench, "DUMP_GRAD_BYTES", 4 * (62 + C) * 100)      # 100 of the 300 rows
    monkeypatch.setattr(bench, "DUMP_IMAGE_BYTES", 4 * (3 + C + 1) * 2 * 25)  # 25 of the 60 pixels
    bucket = GradBucket(P, M, C, "cpu", densify_stats=True)
    g = torch.Generator().manual_seed(0)
    bucket.flat.copy_(torch.randn(bucket.flat.numel(), generator=g))
    bucket.radii.copy_(torch.arange(P, dtype=torch.int32))
    images = {v: (torch.randn(3, H, W, generator=g), torch.randn(C, H, W, generator=g),
                  torch.randn(1, H, W, generator=g)) for v in (1, 0)}
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), bucket, images, 0, 1)
    names = sorted(p.name for p in out.iterdir())
    assert names == sorted(["grad_" + k + ".npy" for k in bucket.views] + ["radii_max.npy", "color.npy",
                                                                            "language.npy", "depth.npy"])
    rows = bench.dump_sample(P, 100, bench.DUMP_SEED)
    for k, view in bucket.views.items():
        a = np.load(out / ("grad_" + k + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, view[rows].numpy())
    assert np.array_equal(np.load(out / "radii_max.npy"), np.arange(P, dtype=np.float32))
    pix = bench.dump_sample(H * W, 25, bench.DUMP_SEED + 2)
    for i, name in enumerate(("color", "language", "depth")):
        a = np.load(out / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == (2, images[0][i].shape[0], 25)
        for j, v in enumerate((0, 1)):
            assert np.array_equal(a[j], images[v][i].flatten(1)[:, pix].numpy())
