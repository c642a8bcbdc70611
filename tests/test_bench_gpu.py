"""bench.py on the GPU at a reduced size (30k Gaussians, 200x120, C = 8, 4 views: two binning
batches, the product path of the headline run), in-process: what a plain run does and prints,
what --full adds, and the --dump-outputs files (the last timed step's bucket, radii MAX and
renders; the same inputs and the same samples from run to run)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

P, W, H, C, V = 30_000, 200, 120, 8, 4
SIZE = ["--gpus", "1", "--gaussians", str(P), "--width", str(W), "--height", str(H), "--channels", str(C),
        "--views", str(V)]
FIELDS = ("means3D", "scales", "rotations", "opacities", "sh", "language_feature", "means2D")


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test_gpu", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(bench, capsys, extra):
    capsys.readouterr()
    bench.run(bench.parse_args(SIZE + extra))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_steps_only(bench, capsys, monkeypatch):
    """A plain run: --steps timed steps after --warmup untimed ones, nothing profiled, no single-view
    or CPU leg, and a line whose value and ms_per_step describe the same measurement."""
    from view_parallel import ViewParallelStep
    calls = []
    real = ViewParallelStep.run
    monkeypatch.setattr(ViewParallelStep, "run", lambda self, cb: (calls.append(1), real(self, cb))[1])
    line = _run(bench, capsys, ["--steps", "3", "--warmup", "2"])
    assert len(calls) == 5
    assert line["steps"] == 3 and line["warmup"] == 2 and line["full"] is False
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - V / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    assert line["config"]["gaussians"] == P and line["config"]["views_per_gpu_per_step"] == V
    assert line["config"]["num_rendered_mean"] > 0
    assert line["roofline"] is None and line["frame_roofline"] is None and line["phases"] == {}
    assert line["single_view"] is None and line["cpu_baseline"] is None


def test_full_run_adds_the_profile(bench, capsys):
    """--full: the per-phase profile and roofline of the dominant kernel and the single-view figure
    (the CPU legs switched off here: they take seconds by design)."""
    line = _run(bench, capsys, ["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
                                "--single-view-steps", "2"])
    assert line["full"] is True and line["steps"] == 2
    assert line["roofline"]["kernel"] in line["phases"] and line["roofline"]["frac"] > 0
    assert {"preprocess", "render_fwd", "render_bwd"} <= set(line["phases"])
    assert line["frame_roofline"]["achieved"] > 0 and line["single_view"]["value"] > 0
    assert line["config"]["visible"] > 0 and line["config"]["visible_any_view"] >= line["config"]["visible"]


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_outputs(bench, capsys, tmp_path):
    """--dump-outputs: float32 files of the last timed step's results, under 64 MB; the renders and
    the radii MAX equal a direct forward of the same seeded scene and cameras; two runs agree (the
    forward exactly, the float-atomic gradient sums within 1e-5 of each field's largest entry, the
    bound tests/test_multirank_gpu.py puts on their reassociation)."""
    import diff_gaussian_rasterization as dgr
    import synthetic
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    line = _run(bench, capsys, ["--steps", "2", "--warmup", "1", "--dump-outputs", d1])
    assert line["steps"] == 2 and line["dumped_outputs"] == d1
    _run(bench, capsys, ["--steps", "3", "--warmup", "0", "--dump-outputs", d2])
    a, b = _load(d1), _load(d2)
    assert sorted(a) == sorted(["grad_" + f for f in FIELDS] + ["radii_max", "color", "language", "depth"])
    assert sorted(a) == sorted(b)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k, x in a.items():
        assert x.dtype == np.float32 and np.isfinite(x).all(), k
        assert x.shape == b[k].shape, k
        if k.startswith("grad_"):
            scale = float(np.abs(x).max())
            assert scale > 0, k
            assert float(np.abs(x - b[k]).max()) <= 1e-5 * scale, k
        else:
            assert np.array_equal(x, b[k]), k
    assert a["grad_means3D"].shape == (P, 3) and a["grad_sh"].shape == (P, 16, 3)      # all rows: P is small
    assert a["grad_language_feature"].shape == (P, C) and a["radii_max"].shape == (P,)
    assert a["color"].shape == (V, 3, H * W) and a["language"].shape == (V, C, H * W) and a["depth"].shape == (V, 1, H * W)

    dev = torch.device("cuda", torch.cuda.current_device())
    scene = synthetic.make_scene(P, C=C, tanfovx=0.6, tanfovy=0.6 * H / W).to(dev)          # bench.py's scene
    radii_max = np.zeros(P, np.float32)
    for v, c in enumerate(synthetic.camera_batch(V, W, H, tanfovx=0.6, seed=1)):              # and cameras
        rs = dgr.GaussianRasterizationSettings(H, W, c.tanfovx, c.tanfovy, torch.ones(3, device=dev), 1.0,
                                               c.world_view_transform.to(dev), c.full_proj_transform.to(dev), 3,
                                               c.camera_center.to(dev), False, False, True)
        color, lang, radii, depth, _ = dgr.forward_native(rs, scene.means3D, scene.opacities, shs=scene.shs,
                                                          language_feature=scene.lang, scales=scene.scales,
                                                          rotations=scene.rotations)
        assert np.array_equal(a["color"][v], color.flatten(1).cpu().numpy()), v
        assert np.array_equal(a["depth"][v], depth.flatten(1).cpu().numpy()), v
        assert np.array_equal(a["language"][v], lang.flatten(1).cpu().numpy()), v
        radii_max = np.maximum(radii_max, radii.cpu().numpy().astype(np.float32))
    assert np.array_equal(a["radii_max"], radii_max)
