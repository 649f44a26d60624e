"""Bench contract tests: the driver runs bench.py here (CPU) and on GPU
boxes at N=1..8; these tests rehearse the exact multi-rank path (gloo,
world 2) including the parallel story + all-gather join lockstep."""
import json
import multiprocessing as mp
import os
import socket
import subprocess
import sys

import pytest


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_default_single_rank():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "5", "--warmup", "1"],
        cwd=REPO,
        capture_output=True,
        text=True,
        timeout=180,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    for key in (
        "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
        "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
    ):
        assert key in line, key
    assert line["n_gpus"] == 1
    assert line["steps"] == 5
    assert line["value"] > 0


def _bench_dump(out_dir, *extra):
    env = dict(os.environ)
    env["BOBRA_BENCH_NO_CPU_FALLBACK"] = "1"  # the real parallel8 story
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
         "--dump-outputs", str(out_dir), *extra],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=180,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes what the last timed step returned, identically
    from run to run; --full leaves the headline line's fields in place."""
    import numpy as np

    plain = _bench_dump(tmp_path / "a")
    full = _bench_dump(tmp_path / "b", "--full")
    for line in (plain, full):
        assert line["steps"] == 3 and line["warmup"] == 1
        assert line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(1000.0 / line["ms_per_step"], rel=1e-2)
        assert line["config"]["bench_config"] == "parallel8"
    assert {k: type(v) for k, v in plain.items()} == {k: type(v) for k, v in full.items()}

    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert "join.joined.npy" in names and "output.rows.npy" in names
    total = 0
    for name in names:
        a = np.load(tmp_path / "a" / name)
        b = np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        assert np.array_equal(a, b), name  # seeded inputs: same arrays every run
        assert np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 * 1024 * 1024

    joined = np.load(tmp_path / "a" / "join.joined.npy")
    assert joined.shape == (8 * 32, 4096)
    assert np.load(tmp_path / "a" / "output.rows.npy").tolist() == [256.0]
    branches = [np.load(tmp_path / "a" / f"fanout.branches.b{i}.embeddings.npy")
                for i in range(8)]
    assert np.array_equal(joined, np.concatenate(branches, axis=0))
    # embed-pool output rows are L2-normalized (bf16 storage)
    assert np.allclose(np.linalg.norm(joined, axis=1), 1.0, atol=2e-2)


def test_bench_dump_sampling_cap(tmp_path):
    """An output over its share of the 64 MB cap is stored as a fixed,
    seeded sample of its elements."""
    import numpy as np

    sys.path.insert(0, REPO)
    import bench

    big = np.arange(10 * 1024 * 1024, dtype=np.float64)  # 80 MB, every value exact
    small = np.ones(7, dtype=np.float64)
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), {"big": big, "small": small})
    a = np.load(tmp_path / "a" / "big.npy")
    assert a.nbytes + small.nbytes <= bench.DUMP_CAP_BYTES
    assert a.size == bench.DUMP_CAP_BYTES // 2 // 8
    assert np.array_equal(a, np.load(tmp_path / "b" / "big.npy"))
    assert np.all(np.diff(a) > 0)  # distinct source elements, in order
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)


def _rank_main(rank: int, world: int, port: int, q) -> None:
    os.environ.update(
        {
            "RANK": str(rank),
            "WORLD_SIZE": str(world),
            "LOCAL_RANK": str(rank),
            "MASTER_ADDR": "127.0.0.1",
            "MASTER_PORT": str(port),
        }
    )
    try:
        sys.path.insert(0, REPO)
        from bobrapet_amd.engine import EngineConfig, RunEngine
        from bobrapet_amd.enums import Phase
        from bobrapet_amd.parallel import group

        group.init_distributed(backend="gloo")
        eng = RunEngine(EngineConfig(cpu_workers=2)).start()
        # the bench's parallel story shape, shrunk for CPU: 4 embed branches
        # + the cross-rank all-gather join (the lockstep collective)
        eng.apply_yaml(
            """
kind: EngramTemplate
metadata: {name: embed}
spec: {builtin: embed}
---
kind: Engram
metadata: {name: embedder}
spec:
  templateRef: {name: embed}
  with: {dim: 64, vocab: 100, batch: 2, seqLen: 4}
---
kind: EngramTemplate
metadata: {name: allgather-join}
spec: {builtin: allgather-join}
---
kind: Engram
metadata: {name: joiner}
spec: {templateRef: {name: allgather-join}}
---
kind: Story
metadata: {name: par}
spec:
  steps:
    - name: fanout
      type: parallel
      with:
        steps:
          - {name: b0, ref: {name: embedder}, with: {seed: 0}}
          - {name: b1, ref: {name: embedder}, with: {seed: 1}}
          - {name: b2, ref: {name: embedder}, with: {seed: 2}}
          - {name: b3, ref: {name: embedder}, with: {seed: 3}}
    - name: join
      ref: {name: joiner}
      needs: [fanout]
      with:
        branches: "{{ steps.fanout.output.branches }}"
  output:
    rows: "{{ steps.join.output.worldRows }}"
"""
        )
        rows = []
        for i in range(3):  # sequential lockstep runs, like the bench loop
            run = eng.run_story("default/par", {"i": i}, timeout=120)
            assert run.phase == Phase.SUCCEEDED, (run.error, {
                k: str(v.phase) for k, v in run.step_states.items()
            })
            rows.append(run.output["rows"])
        agg = group.sum_over_ranks(float(rows[-1]), device="cpu")
        q.put((rank, {"rows": rows, "agg": agg}))
        eng.stop()
        group.teardown()
    except Exception as exc:
        import traceback

        q.put((rank, {"error": f"{exc}\n{traceback.format_exc()}"}))


@pytest.mark.timeout(240)
def test_parallel_join_two_ranks_lockstep():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    world = 2
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, payload = q.get(timeout=220)
        results[rank] = payload
    for p in procs:
        p.join(timeout=30)
    for rank, payload in results.items():
        assert "error" not in payload, f"rank {rank}: {payload.get('error')}"
        # 4 branches x batch 2 x 2 ranks = 16 joined rows on every rank
        assert payload["rows"] == [16, 16, 16], payload
    assert results[0]["agg"] == results[1]["agg"]


@pytest.mark.timeout(300)
def test_bench_parallel8_pipelined_two_ranks():
    """Rehearse the driver's multi-rank bench launch exactly: torchrun world=2
    (gloo on CPU), the REAL parallel8 story (no cpu fallback), pipelined
    in-flight slots + comm-slot communicators for the all-gather join."""
    port = _free_port()
    env = dict(os.environ)
    env.update({"BOBRA_BENCH_NO_CPU_FALLBACK": "1", "BOBRA_BENCH_INFLIGHT": "4"})
    # the rehearsal is gloo on CPU: hide the GPUs, or two ranks would ask
    # for two devices on a box that may have one
    env["HIP_VISIBLE_DEVICES"] = "-1"
    out = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node", "2",
            "--master-addr", "127.0.0.1", "--master-port", str(port),
            "bench.py", "--gpus", "2", "--steps", "6", "--warmup", "1",
            "--config", "parallel8",
        ],
        cwd=REPO,
        env=env,
        capture_output=True,
        text=True,
        timeout=280,
    )
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert lines, out.stdout[-1500:]
    line = json.loads(lines[-1])
    assert line["n_gpus"] == 2
    assert line["value"] > 0
    assert line["config"]["branches"] == 8
