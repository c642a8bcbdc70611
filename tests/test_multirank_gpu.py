"""configs[3]'s code path on the one-GPU box (BASELINE.json: 64-view batch, per-view data parallel,
8 x MI355X over RCCL).  The box has one GPU, so the ranks share it and the collectives run over
gloo (LSR_BENCH_BACKEND=gloo, LSR_BENCH_SHARE_DEVICE=1); everything above the collectives is the
product path: bench.py's rank spawn (view_parallel.launch_ranks), the device binding, the barrier
and MAX-over-ranks timing, the view slicing, the batched renderer, the bucket's SUM and the radii
MAX, and ShardedAdam's reduce-scatter / Adam on the row shard / all-gather.  The scaling curve
itself (RCCL over xGMI, one GPU per rank) stays unmeasured here: the driver runs it on an 8-GPU
node.  Every multi-rank run is a fresh child process (subprocess.run), never an exec of this one.
Reference semantics: train.py:242-271 (views rendered in a loop, radii MAX, visibility ANY),
:339 (one backward over the batch), :420-421 (optimizer step)."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import mp_view_parallel_gpu as mpv  # noqa: E402

pytestmark = pytest.mark.gpu


def _env():
    env = dict(os.environ)
    env.update(LSR_BENCH_BACKEND="gloo", LSR_BENCH_SHARE_DEVICE="1", MASTER_ADDR="127.0.0.1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MASTER_PORT", None)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    return env


@pytest.mark.timeout(420)
def test_bench_two_ranks_prints_one_line():
    """bench.py --gpus 2 at the headline size (2M, 1352x1014, C = 32, 8 views per rank): one JSON
    line from rank 0 with both ranks' 16 views counted and the process group's rank count."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--single-view-steps", "0"]   # --full: the line's roofline entry
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["ranks"] == 2
    assert line["config"]["global_batch"] == 16 and line["config"]["parallelism"] == "dp2"
    assert line["steps"] == 2 and line["value"] > 0
    assert abs(line["value"] - 16 * 2 / (line["ms_per_step"] * 2e-3)) <= 1e-3 * line["value"]
    # the dominant kernel is picked by event time; with both ranks on one device an event pair of one
    # rank also spans the other rank's kernels, so which phase comes out ahead here is arbitrary (the
    # one-GPU line, where it is render_bwd, is bench.py's own run)
    assert line["roofline"]["kernel"] in ("render_bwd", "render_fwd", "preprocess", "preprocess_bwd_views",
                                          "preprocess_bwd", "emit", "tile_ranges")
    assert line["roofline"]["frac"] > 0 and line["cpu_baseline"] is None


def _spawn(mode, steps, chunks=1, world=2, views=mpv.N_VIEWS, timeout=240):
    d = tempfile.mkdtemp(prefix="lsr_mp_")
    cmd = [sys.executable, os.path.join(HERE, "mp_view_parallel_gpu.py"), "--out", d, "--world", str(world),
           "--mode", mode, "--steps", str(steps), "--chunks", str(chunks), "--views", str(views)]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    outs = [torch.load(os.path.join(d, f"rank{k}.pt"), weights_only=True) for k in range(world)]
    for k in range(world):
        os.remove(os.path.join(d, f"rank{k}.pt"))
    os.rmdir(d)
    return outs


def _check_bucket(ser, outs, n_views):
    """Every rank ends the step with the same bucket, equal to one rank rendering every view up to the
    fp32 reassociation of the float-atomic view sums; radii MAX exactly; the views sliced contiguously."""
    world = len(outs)
    got_views = [v for o in outs for v in o["views"]]
    assert got_views == list(range(n_views)) and ser["views"] == list(range(n_views))
    assert all(len(o["views"]) == n_views // world for o in outs)
    for k, v in ser["grads"].items():
        if v is None:
            continue
        a = outs[0]["grads"][k]
        for o in outs[1:]:
            assert torch.equal(a, o["grads"][k]), k      # the all-reduce leaves every rank the same sum
        scale = float(v.abs().max())
        assert scale > 0, k
        assert float((a - v).abs().max()) <= 1e-5 * scale, (k, float((a - v).abs().max()), scale)
    for o in outs:
        assert torch.equal(o["radii"], ser["radii"])


@pytest.mark.timeout(300)
def test_two_rank_bucket_equals_one_rank_sum():
    """Two ranks (views 0-7 and 8-15, the batched renderer with 3 early views each) end the step
    with the same bucket on both ranks, equal to one rank rendering all 16 views up to the fp32
    reassociation of the float-atomic view sums; radii MAX exactly."""
    ser = mpv.run_rank(0, 1, None, "allreduce", 1)
    outs = _spawn("allreduce", 1)
    assert outs[0]["views"] == list(range(8)) and outs[1]["views"] == list(range(8, 16))
    _check_bucket(ser, outs, mpv.N_VIEWS)


def _assemble(outs, get):
    """[P, ...] rows from the ranks' pieces; get(o) -> (global row ids, rows).  Every row exactly once."""
    rows0 = get(outs[0])[1]
    got = torch.zeros((mpv.P,) + tuple(rows0.shape[1:]), dtype=rows0.dtype)
    seen = torch.zeros(mpv.P, dtype=torch.bool)
    for o in outs:
        idx, rows = get(o)
        assert not seen[idx].any()
        got[idx], seen[idx] = rows, True
    assert bool(seen.all())
    return got


def _adam_replay(p0, grads, lr):
    """torch.optim.Adam (eps 1e-15, the reference's optimizer: gaussian_model.py:301) over the given
    gradient sequence, on the CPU in float32."""
    p = torch.nn.Parameter(p0.clone().float())
    opt = torch.optim.Adam([p], lr=lr, eps=1e-15, foreach=False)
    for g in grads:
        p.grad = g.clone().float().reshape(p.shape)
        opt.step()
    return p.detach()


def _activate(k, x):
    """render()'s activations of a raw group (gaussian_model.py:38-47, gaussian_renderer/__init__.py)."""
    if k == "scaling":
        return torch.exp(x)
    if k == "rotation":
        return torch.nn.functional.normalize(x)
    if k == "opacity":
        return torch.sigmoid(x)
    if k == "language_feature":
        return x / (x.norm(dim=-1, keepdim=True) + 1e-9)
    return x


ACT_OF = dict(xyz="means3D", scaling="scales", rotation="rotations", opacity="opacities", language_feature="lang")


def _check_sharded(ser, outs, steps):
    """ShardedAdam over `steps` steps on len(outs) ranks against one rank doing every view and row.
    No tolerance is a free fraction of rows:
      1. the reduce-scattered gradients (recorded per piece, after the activations' backward) equal the
         serial ones per element within |d| <= 1e-4 |g| + 1e-6 max|g| (the float-atomic view sums
         reassociate; the absolute floor covers sums that cancel to near zero);
      2. Adam on the shards is exactly torch.optim.Adam on the reduced gradients: the CPU replay from
         the initial parameters matches every rank's rows within float32 rounding;
      3. every parameter element equals the serial one within 1e-6 + 1e-5 |p| + 1e-3 lr steps, except
         the elements whose gradient differed from the serial one by more than 1e-4 relative in some
         step (check 1 bounds those differences absolutely): Adam normalises the gradient, so a
         near-zero sum whose last bits moved may turn the update's sign (bounded by 2 lr per step);
      4. every rank holds the same activated scene, the activations of the gathered parameters."""
    init = mpv.raw_scene()[1]
    for k in ser["full"]:
        lr = mpv.LRS[k]
        exempt = torch.zeros_like(init[k], dtype=torch.bool)
        g_dist = []
        for st in range(1, steps + 1):
            gs = _assemble([ser], lambda o: o["grads_rec"][st][k]).double()
            gd = _assemble(outs, lambda o: o["grads_rec"][st][k]).double()
            g_dist.append(gd)
            d = (gd - gs).abs()
            bound = 1e-4 * gs.abs() + 1e-6 * float(gs.abs().max())
            assert bool((d <= bound).all()), (k, st, float((d - bound).max()))
            exempt |= (d > 1e-4 * gs.abs() + 1e-30).reshape(exempt.shape)
        got = _assemble(outs, lambda o: o["full"][k])
        want = _assemble([ser], lambda o: o["full"][k])
        assert float((want - init[k]).abs().max()) > 0, k            # the steps moved the parameters
        rep = _adam_replay(init[k], g_dist, lr)
        dr = (got - rep).abs()
        assert bool((dr <= 1e-6 * rep.abs() + 1e-6 * lr).all()), (k, float(dr.max()))
        d = (got - want).abs()
        tight = d <= 1e-6 + 1e-5 * want.abs() + 1e-3 * lr * steps
        assert bool((tight | exempt).all()), (k, int((~tight & ~exempt).sum()), float(d[~exempt].max()))
        assert float(d.max()) <= 2 * lr * steps, (k, float(d.max()))
        if k in ACT_OF:
            a = outs[0]["act"][ACT_OF[k]]
            da = (a - _activate(k, got)).abs()
            assert bool((da <= 1e-6 + 1e-6 * a.abs()).all()), (k, float(da.max()))
    for k, v in ser["act"].items():
        for o in outs[1:]:
            assert torch.equal(outs[0]["act"][k], o["act"][k]), k   # every rank renders the same scene
    assert all(torch.equal(o["radii"], ser["radii"]) for o in outs)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("chunks", [1, 4])
def test_two_rank_sharded_adam_equals_serial(chunks):
    """Two optimizer steps with ShardedAdam (reduce-scatter by Gaussian rows, lsr_adam_step on each
    rank's shard, all-gather of the activated inputs) against one rank doing every view and row.
    chunks = 4: the chunk pipeline (each flush chunk's reduce-scatter behind its launch, Adam and the
    all-gather chunk by chunk, and the second step's batched preprocess launched per row chunk as
    each chunk's gather lands: lsr_forward_preprocess_views_rows_async, ViewParallelStep(defer_gather))."""
    steps = 2
    ser = mpv.run_rank(0, 1, None, "sharded", steps)
    outs = _spawn("sharded", steps, chunks)
    if chunks == 1:
        r0, r1 = outs[0]["rows"], outs[1]["rows"]
        assert r0[0] == 0 and r0[1] == r1[0] and r1[1] == mpv.P
    _check_sharded(ser, outs, steps)


# ---- configs[3]'s shape: 8 ranks, a 64-view global batch ------------------------------------------------

@pytest.mark.timeout(900)
def test_bench_eight_ranks_configs3_shape():
    """bench.py --gpus 8 at the headline size (2M, 1352x1014, C = 32): 8 ranks x 8 views = the 64-view
    batch of BASELINE configs[3], one JSON line from rank 0 with all 64 views counted."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "1",
           "--no-cpu-baseline", "--single-view-steps", "0", "--no-profile"]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=840)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 8 and line["ranks"] == 8
    assert line["config"]["global_batch"] == 64 and line["config"]["parallelism"] == "dp8"
    assert line["config"]["views_per_gpu_per_step"] == 8
    assert line["steps"] == 1 and line["value"] > 0
    assert abs(line["value"] - 64 / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]


@pytest.mark.timeout(600)
def test_eight_rank_bucket_equals_one_rank_sum():
    """Eight ranks over a 64-view batch (8 views each: the batched renderer's 3 early + 5 side views)
    at reduced P: every rank's bucket equals one rank rendering all 64 views; radii MAX exactly."""
    ser = mpv.run_rank(0, 1, None, "allreduce", 1, n_views=64)
    outs = _spawn("allreduce", 1, world=8, views=64, timeout=540)
    assert [o["views"] for o in outs] == [list(range(8 * r, 8 * r + 8)) for r in range(8)]
    _check_bucket(ser, outs, 64)


@pytest.mark.timeout(600)
def test_eight_rank_sharded_adam_chunks4_equals_serial():
    """ShardedAdam(chunks=4) on 8 ranks over a 64-view batch: 4 chunks x 8 pieces of 768 rows
    (Pa = 24576 for P = 20000, so the last chunk's pieces are partly and wholly past P), two steps,
    the second step's preprocess waiting per row chunk; against the serial step."""
    steps = 2
    ser = mpv.run_rank(0, 1, None, "sharded", steps, n_views=64)
    outs = _spawn("sharded", steps, chunks=4, world=8, views=64, timeout=540)
    _check_sharded(ser, outs, steps)
