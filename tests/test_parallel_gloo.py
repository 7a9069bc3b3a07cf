"""gloo tests of the clip-parallel path (run on CPU): sharding + the single all-gather must reproduce the
rank-order == clip-order of the whole batch, for equal and ragged shards -- at world size 2 and, since round 6, at world
size 8 in the regimes the metric names (8 clips per rank; config 4's 16 clips over 8 ranks; strong scaling at 1 clip per
rank; a ragged 12-over-8 in which two ranks hold nothing).  The forward itself is a stand-in (the HIP engine needs a
GPU); the collective logic, bench.py's timed region and its launcher are what is under test."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_forward(clips):
    # deterministic per-clip "logits": depends only on the clip's content
    flat = clips.flatten(1)                   # (an empty shard -- 12 clips over 8 ranks -- gives [0, 4] logits)
    if flat.shape[0] == 0:
        return flat.new_zeros((0, 4))
    return torch.stack([flat.mean(1), flat.abs().max(1).values, flat[:, 0], flat.sum(1)], 1)


def _worker(rank, world, port, total, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pretorched_x_amd.parallel import clip_parallel_forward, shard_clips
    g = torch.Generator().manual_seed(123)
    clips = torch.randn(total, 3, 2, 4, 4, generator=g)          # identical on every rank
    local = shard_clips(clips)
    out = clip_parallel_forward(_fake_forward, local, total=total)
    out2 = clip_parallel_forward(_fake_forward, local, total=None)  # size-discovery path
    want = _fake_forward(clips)
    ok = torch.equal(out, want) and torch.equal(out2, want)
    q.put((rank, bool(ok), tuple(out.shape)))
    dist.barrier()
    dist.destroy_process_group()


def _bench_worker(rank, world, port, total, q, corrupt):
    """Drives bench.py's N > 1 branch itself -- timed_steps (barriers, MAX-over-ranks timing, the one
    all-gather per step) + the self-check + the rank-0 tuned-table broadcast -- under gloo with a stand-in
    forward.  `corrupt`: rank 1 returns logits that change between calls, which the check must flag."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    from pretorched_x_amd import engine
    from pretorched_x_amd.parallel import broadcast_tuned_table, shard_clips
    g = torch.Generator().manual_seed(7)
    clips = torch.randn(total, 3, 2, 4, 4, generator=g)
    local = shard_clips(clips)
    calls = [0]

    def run():
        calls[0] += 1
        out = _fake_forward(local)
        return out + calls[0] if (corrupt and rank == 1) else out

    elapsed, out, verify, rank_ms = bench.timed_steps(run, total, steps=3, warmup=1, dev=torch.device("cpu"),
                                                      sync=lambda: None)
    # every rank's own step time travels with the MAX (a straggler must be visible in the line)
    assert len(rank_ms["ms_per_step"]) == world and rank_ms["max"] >= rank_ms["min"] > 0
    assert rank_ms["ms_per_step"][rank_ms["argmax_rank"]] == rank_ms["max"] and abs(rank_ms["max"] - 1e3 * elapsed / 3) < 1e-3
    # rank 0 "tunes", everyone adopts its table
    if rank == 0:
        engine.tuned_merge({"[\"fake-problem\"]": ("64x64x16/2x2/m32/dma", 2)})
    n = broadcast_tuned_table(src=0)
    has = engine.tuned_snapshot().get("[\"fake-problem\"]")
    ok_out = corrupt or torch.equal(out, _fake_forward(clips))
    q.put((rank, dict(verify), bool(ok_out), calls[0], elapsed > 0, has, n > 0))
    dist.barrier()
    dist.destroy_process_group()


def _strong_worker(rank, world, port, total, q, workload):
    """bench.py --scaling strong under gloo: ONE global batch (identical on every rank) cut by bench.local_batch /
    parallel.shard_clips, timed_steps gathers `total` rows (ragged shards included), rank order == clip order."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    bench.GLOBAL_BATCH = dict(bench.GLOBAL_BATCH, **{workload: total})        # small stand-in batch sizes
    make = lambda n, seed: torch.randn(n, 3, 2, 4, 4, generator=torch.Generator().manual_seed(seed))     # noqa: E731
    local, tot = bench.local_batch(make, 8, workload, "strong", world, rank)
    elapsed, out, verify, _rank_ms = bench.timed_steps(lambda: _fake_forward(local), tot, steps=2, warmup=1, dev=torch.device("cpu"),
                                                       sync=lambda: None)
    want = _fake_forward(make(total, 99))
    q.put((rank, dict(verify), bool(torch.equal(out, want)), int(local.shape[0]), tot))
    dist.barrier()
    dist.destroy_process_group()


def _collect(procs, q, world, limit=240.0):
    """One result per rank -- or a failure as soon as a rank dies / the deadline passes: never a parent blocked forever on
    a queue nobody will write to (the other ranks of a dead one sit in a collective until gloo times out)."""
    import time
    res, deadline = [], time.time() + limit
    try:
        while len(res) < world:
            if not q.empty():
                res.append(q.get())
                continue
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not dead, "a rank exited with %s" % dead
            assert time.time() < deadline, "ranks did not report within %.0f s (%d of %d did)" % (limit, len(res), world)
            time.sleep(0.05)
        for p in procs:
            p.join(60)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    return res


def _run(total, world=2, target=None, extra=()):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    if target is not None:
        procs = [ctx.Process(target=target, args=(r, world, port, total, q) + tuple(extra)) for r in range(world)]
        for p in procs:
            p.start()
        return _collect(procs, q, world)
    procs = [ctx.Process(target=_worker, args=(r, world, port, total, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(procs, q, world)
    assert all(ok for _, ok, _ in res), res
    assert all(shape == (total, 4) for _, _, shape in res), res


def test_clip_parallel_equal_shards():
    _run(total=8)


def test_clip_parallel_ragged_shards():
    _run(total=5)


def test_bench_distributed_branch_is_self_verifying():
    """bench.py at N > 1: 1 warm-up + 3 timed steps + 1 verification forward per rank, gather order and
    cross-rank identity confirmed, the rank-0 tuned table reaches every rank."""
    res = _run(total=8, target=_bench_worker, extra=(False,))
    for rank, verify, ok_out, calls, timed, has, n in res:
        assert verify == {"gather_order_ok": True, "replicas_identical": True, "ranks": 2, "rows": 8,
                          "deterministic": True}, (rank, verify)
        assert ok_out and timed and calls == 5
        assert has == ("64x64x16/2x2/m32/dma", 2) and n


def test_bench_distributed_check_flags_a_bad_rank():
    res = _run(total=8, target=_bench_worker, extra=(True,))
    for rank, verify, *_ in res:
        assert verify["gather_order_ok"] and verify["replicas_identical"]      # the gather itself is fine ...
        assert verify["deterministic"] is False                                   # ... rank 1's forward is not


def test_bench_strong_scaling_shards_one_global_batch():
    """--scaling strong (cfg2: the fixed 8-clip batch; cfg4: 16 clips over the ranks), equal and ragged shards."""
    for total, workload in ((8, "cfg2"), (5, "cfg4")):
        res = _run(total=total, target=_strong_worker, extra=(workload,))
        per = sorted(n for _, _, _, n, _ in res)
        assert sum(per) == total and per == sorted([total - total // 2, total // 2]), per
        for rank, verify, ok, n, tot in res:
            assert tot == total and ok, (rank, n)
            assert verify["gather_order_ok"] and verify["replicas_identical"] and verify["deterministic"] and verify["rows"] == total


def test_bench_gpus_n_starts_its_own_ranks():
    """VERDICT r3 missing #1: `python bench.py --gpus 2` WITHOUT a launcher must become two ranks (it re-executes itself under
    torch.distributed.run, one process per GPU) instead of silently running one; `--gpus N` that disagrees with a
    launcher's WORLD_SIZE, or asks for more GPUs than the node has, fails loudly.  PTX_BENCH_LAUNCH_CHECK=1: the ranks
    rendezvous over gloo and report, nothing is measured (no GPU here)."""
    import json
    import subprocess
    env = dict(os.environ, PTX_BENCH_LAUNCH_CHECK="1", PTX_BENCH_BACKEND="gloo", PYTHONDONTWRITEBYTECODE="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    bench = os.path.join(ROOT, "bench.py")
    r = subprocess.run([sys.executable, bench, "--gpus", "2"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["ranks_seen"] == {"world_size": 2, "distinct_pids": 2, "local_ranks": [0, 1]}, line
    # --scaling both: the weak line, then the strong line, from ONE invocation; PTX_BENCH_TIMEOUT bounds every collective
    # wait (the other ranks sit in the tuned-table broadcast while rank 0 tunes)
    r = subprocess.run([sys.executable, bench, "--gpus", "2", "--scaling", "both"], env=dict(env, PTX_BENCH_TIMEOUT="77"),
                       capture_output=True, text=True, timeout=300)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and [ln["scaling"] for ln in lines] == ["weak", "strong"], (r.stderr[-800:], lines)
    assert all(ln["process_group_timeout_s"] == 77.0 and ln["ranks_seen"]["world_size"] == 2 for ln in lines)
    # N = 1: no launcher, no process group
    r = subprocess.run([sys.executable, bench, "--gpus", "1"], env=env, capture_output=True, text=True, timeout=300)
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert r.returncode == 0 and line["n_gpus"] == 1 and line["ranks_seen"]["world_size"] == 1, (r.stderr[-500:], line)
    # no --gpus under a launcher: the launcher's WORLD_SIZE is taken (`torchrun ... bench.py` must keep working)
    r = subprocess.run([sys.executable, bench], env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=300)
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert r.returncode == 0 and line["n_gpus"] == 1, r.stderr[-500:]
    # a launcher's WORLD_SIZE that disagrees with --gpus is an error, not a warning
    r = subprocess.run([sys.executable, bench, "--gpus", "8"], env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "must agree" in r.stderr
    # RCCL needs one GPU per rank: asking for more than the node has fails before anything is launched
    env_nccl = dict(env, PTX_BENCH_BACKEND="nccl")
    r = subprocess.run([sys.executable, bench, "--gpus", "2"], env=env_nccl, capture_output=True, text=True, timeout=300)
    if torch.cuda.device_count() < 2:
        assert r.returncode != 0 and "visible GPU" in r.stderr, r.stderr[-500:]


# ---- world size 8: the regimes the metric names -------------------------------------------------------------

def test_world8_gather_equal_and_ragged():
    """8 ranks: 64 clips (8 per rank, the weak-scaling shape), 16 (config 4: 2 per rank), 8 (strong: 1 per rank) and 12
    (torch.chunk semantics, as DataParallel's scatter: six ranks hold 2 clips, ranks 6 and 7 hold none)."""
    for total in (64, 16, 8, 12):
        _run(total=total, world=8)


def test_world8_bench_weak_regime_is_self_verifying():
    """bench.timed_steps at 8 ranks x 8 clips + verify_gather + the rank-0 tuned-table broadcast."""
    res = _run(total=64, world=8, target=_bench_worker, extra=(False,))
    assert sorted(r[0] for r in res) == list(range(8))
    for rank, verify, ok_out, calls, timed, has, n in res:
        assert verify == {"gather_order_ok": True, "replicas_identical": True, "ranks": 8, "rows": 64,
                          "deterministic": True}, (rank, verify)
        assert ok_out and timed and calls == 5
        assert has == ("64x64x16/2x2/m32/dma", 2) and n
    res = _run(total=64, world=8, target=_bench_worker, extra=(True,))
    assert all(v["gather_order_ok"] and v["replicas_identical"] and v["deterministic"] is False for _, v, *_ in res)


def test_world8_bench_strong_regimes():
    """--scaling strong at 8 ranks: config 4 (16 clips, 2 per rank), the headline batch (8 clips, ONE per rank) and a ragged
    12-clip batch (2,2,2,2,2,2,0,0): every rank ends with the whole batch's logits in clip order."""
    from pretorched_x_amd.parallel import shard_bounds
    for total, workload in ((16, "cfg4"), (8, "cfg2"), (12, "cfg3")):
        res = _run(total=total, world=8, target=_strong_worker, extra=(workload,))
        per = {rank: n for rank, _, _, n, _ in res}
        assert [per[r] for r in range(8)] == [shard_bounds(total, 8, r)[1] - shard_bounds(total, 8, r)[0] for r in range(8)]
        assert sum(per.values()) == total
        for rank, verify, ok, n, tot in res:
            assert tot == total and ok, (rank, n)
            assert verify["gather_order_ok"] and verify["replicas_identical"] and verify["deterministic"] and verify["rows"] == total
            assert verify["ranks"] == 8


def test_bench_gpus_8_self_launch_standin_lines():
    """`python bench.py --gpus 8 --scaling both` WITHOUT a launcher and without GPUs: PTX_BENCH_STANDIN=1 + PTX_BENCH_BACKEND=gloo
    runs the real N-rank code path of bench.py (self-launch under torch.distributed.run, local_batch, timed_steps, the
    gather, the per-rank bookkeeping) with a CPU stand-in forward.  One JSON line per scaling mode, 8 entries in
    rank_ms_per_step and ranks_seen; config 4's 16 clips leave 2 per rank."""
    import json
    import subprocess
    env = dict(os.environ, PTX_BENCH_STANDIN="1", PTX_BENCH_BACKEND="gloo", PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PTX_BENCH_LAUNCH_CHECK"):
        env.pop(k, None)
    bench = os.path.join(ROOT, "bench.py")
    r = subprocess.run([sys.executable, bench, "--gpus", "8", "--scaling", "both", "--steps", "3", "--warmup", "1"], env=env,
                       capture_output=True, text=True, timeout=600)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and [ln["scaling"] for ln in lines] == ["weak", "strong"], (r.stderr[-1500:], lines)
    weak, strong = lines
    for ln in lines:
        assert ln["standin"] is True and ln["n_gpus"] == 8 and ln["roofline"] is None
        assert "FUNCTIONAL CHECK" in ln["config"]["parallelism"]
        assert len(ln["rank_ms_per_step"]["ms_per_step"]) == 8 and ln["rank_ms_per_step"]["max"] >= ln["rank_ms_per_step"]["min"] > 0
        seen = ln["ranks_seen"]
        assert seen["world_size"] == 8 and sorted(r_["rank"] for r_ in seen["ranks"]) == list(range(8))
        assert len({r_["pid"] for r_ in seen["ranks"]}) == 8
        assert ln["distributed_check"] == {"gather_order_ok": True, "replicas_identical": True, "ranks": 8,
                                           "rows": ln["config"]["global_batch"], "deterministic": True}
    assert weak["config"]["global_batch"] == 64 and [r_["units"] for r_ in weak["ranks_seen"]["ranks"]] == [8] * 8
    assert strong["config"]["global_batch"] == 8 and [r_["units"] for r_ in strong["ranks_seen"]["ranks"]] == [1] * 8
    # config 4: 16 clips over 8 ranks, strong by construction
    r = subprocess.run([sys.executable, bench, "--gpus", "8", "--workload", "cfg4", "--scaling", "strong", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-1500:]
    assert lines[0]["config"]["global_batch"] == 16 and [r_["units"] for r_ in lines[0]["ranks_seen"]["ranks"]] == [2] * 8
    # the stand-in refuses to pose as an RCCL run
    r = subprocess.run([sys.executable, bench, "--gpus", "1"], env=dict(env, PTX_BENCH_BACKEND="nccl"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "PTX_BENCH_STANDIN" in r.stderr


def test_bench_dump_outputs_and_steps():
    """`--dump-outputs DIR` writes the last timed step's output as DIR/<name>.npy (float32), identical from run to run with
    the same arguments; `--steps` is the number of timed steps in the line; a plain run carries no secondary legs.  Driven
    through the CPU stand-in forward (PTX_BENCH_STANDIN=1), the same measure() / timed_steps path a GPU run takes."""
    import json
    import subprocess
    import tempfile

    import numpy as np
    env = dict(os.environ, PTX_BENCH_STANDIN="1", PTX_BENCH_BACKEND="gloo", PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PTX_BENCH_LAUNCH_CHECK"):
        env.pop(k, None)
    bench = os.path.join(ROOT, "bench.py")
    with tempfile.TemporaryDirectory() as tmp:
        arrays = []
        for i, steps in enumerate((3, 5)):
            d = os.path.join(tmp, "run%d" % i)
            r = subprocess.run([sys.executable, bench, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dump-outputs", d],
                               env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-1500:]
            line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            assert line["steps"] == steps and line["ms_per_step"] > 0 and line["full"] is False, line
            assert line["dumped_outputs"] == ["logits"] and os.listdir(d) == ["logits.npy"]
            a = np.load(os.path.join(d, "logits.npy"))
            assert a.dtype == np.float32 and a.shape == (8, 339) and np.isfinite(a).all()
            arrays.append(a)
        assert np.array_equal(arrays[0], arrays[1])
        r = subprocess.run([sys.executable, bench, "--gpus", "1", "--steps", "0"], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode != 0 and "--steps" in r.stderr
