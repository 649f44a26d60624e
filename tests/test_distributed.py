"""Multi-process distributed tests (gloo backend, world_size=2, CPU).

Covers the cross-rank story path: step→rank placement, topological-level
execution, tensor-aware output broadcast — the same code path that runs
over RCCL/xGMI on a GPU node.
"""
import json
import multiprocessing as mp
import os
import socket

import pytest
import torch


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


RESOURCES = """
kind: EngramTemplate
metadata: {name: echo-tpl}
spec: {builtin: echo}
---
kind: Engram
metadata: {name: echoer}
spec: {templateRef: {name: echo-tpl}}
---
kind: EngramTemplate
metadata: {name: embed}
spec: {builtin: embed}
---
kind: Engram
metadata: {name: embedder}
spec:
  templateRef: {name: embed}
  with: {dim: 256, vocab: 500}
"""

STORY = """
kind: Story
metadata: {name: dist-story}
spec:
  steps:
    - {name: left, ref: {name: echoer}, with: {v: "{{ inputs.x }}", side: left}}
    - {name: right, ref: {name: echoer}, with: {v: "{{ inputs.x * 2 }}", side: right}}
    - name: decide
      type: condition
      needs: [left, right]
      with: {expression: "{{ steps.left.output.v + steps.right.output.v == 30 }}"}
    - name: vectors
      ref: {name: embedder}
      needs: [decide]
      with: {batch: 4, seqLen: 8}
    - name: summary
      ref: {name: echoer}
      needs: [vectors]
      with:
        ok: "{{ steps.decide.output.result }}"
  output:
    ok: "{{ steps.summary.output.ok }}"
"""


def _worker(rank: int, world: int, port: int, q) -> None:
    os.environ.update(
        {
            "RANK": str(rank),
            "WORLD_SIZE": str(world),
            "MASTER_ADDR": "127.0.0.1",
            "MASTER_PORT": str(port),
        }
    )
    try:
        from bobrapet_amd.engine import EngineConfig, RunEngine
        from bobrapet_amd.parallel import distributed, group

        group.init_distributed(backend="gloo")
        eng = RunEngine(EngineConfig(cpu_workers=2)).start()
        eng.apply_yaml(RESOURCES)
        eng.apply_yaml(STORY)
        result = distributed.run_story_distributed(
            eng, "default/dist-story", {"x": 10}, timeout=60
        )
        # tensor payloads must have crossed the rank boundary as tensors
        emb = result["steps"]["vectors"]["output"]["embeddings"]
        tensor_ok = torch.is_tensor(emb) and tuple(emb.shape) == (4, 256)
        q.put(
            (
                rank,
                {
                    "phase": result["phase"],
                    "output": result["output"],
                    "steps": {k: v["phase"] for k, v in result["steps"].items()},
                    "tensor_ok": bool(tensor_ok),
                    "emb_sum": float(emb.float().sum().item()) if tensor_ok else None,
                },
            )
        )
        eng.stop()
        group.teardown()
    except Exception as exc:  # surface worker crashes to the parent
        import traceback

        q.put((rank, {"error": f"{exc}\n{traceback.format_exc()}"}))


@pytest.mark.timeout(120)
def test_distributed_story_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    world = 2
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, payload = q.get(timeout=110)
        results[rank] = payload
    for p in procs:
        p.join(timeout=30)
    for rank, payload in results.items():
        assert "error" not in payload, f"rank {rank}: {payload.get('error')}"
        assert payload["phase"] == "Succeeded", payload
        assert payload["output"] == {"ok": True}
        assert payload["tensor_ok"], payload
    # both ranks hold the SAME broadcast tensor payload
    assert results[0]["emb_sum"] == pytest.approx(results[1]["emb_sum"], rel=1e-3)
    assert results[0]["steps"] == results[1]["steps"]


def test_placement_deterministic():
    from bobrapet_amd.parallel.distributed import place_steps, topo_levels
    from bobrapet_amd.specs import load_yaml

    (story,) = load_yaml(STORY)
    p1 = place_steps(story, 4)
    p2 = place_steps(story, 4)
    assert p1 == p2
    assert set(p1.values()) <= {0, 1, 2, 3}
    levels = topo_levels(story)
    assert levels[0] == ["left", "right"]
    assert levels[1] == ["decide"]


def test_placement_respects_pin():
    from bobrapet_amd.parallel.distributed import place_steps
    from bobrapet_amd.specs import load_yaml

    (story,) = load_yaml(
        """
kind: Story
metadata: {name: pinned}
spec:
  steps:
    - name: a
      ref: {name: x}
      execution: {placement: {gpu: 3}}
    - {name: b, ref: {name: x}}
"""
    )
    p = place_steps(story, 8)
    assert p["a"] == 3


def _ring_attn_rank(rank: int, world: int, port: int, q):
    import os
    import sys

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
        import torch

        from bobrapet_amd import ops
        from bobrapet_amd.parallel import group
        from bobrapet_amd.parallel.ring_attention import ring_attention

        group.init_distributed(backend="gloo")
        torch.manual_seed(7)  # same global tensors on every rank
        B, S, Hq, Hkv, D = 2, 48, 4, 2, 64
        S_glob = S * world
        qg = torch.randn(B, S_glob, Hq, D, dtype=torch.bfloat16)
        kg = torch.randn(B, S_glob, Hkv, D, dtype=torch.bfloat16)
        vg = torch.randn_like(kg)
        res = {}
        for causal in (True, False):
            full = ops.attn_prefill(qg, kg, vg, None, causal)
            lo, hi = rank * S, (rank + 1) * S
            out = ring_attention(
                qg[:, lo:hi].contiguous(),
                kg[:, lo:hi].contiguous(),
                vg[:, lo:hi].contiguous(),
                causal=causal,
            )
            err = (out.float() - full[:, lo:hi].float()).abs().max().item()
            res[f"causal={causal}"] = err
        q.put((rank, res))
        group.teardown()
    except Exception as exc:
        import traceback

        q.put((rank, {"error": f"{exc}\n{traceback.format_exc()}"}))


@pytest.mark.timeout(180)
@pytest.mark.parametrize("world", [2, 3])
def test_ring_attention_matches_full(world):
    """Sequence-parallel ring attention == single-rank full attention,
    causal and non-causal, including an odd ring size."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [
        ctx.Process(target=_ring_attn_rank, args=(r, world, port, q)) for r in range(world)
    ]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, payload = q.get(timeout=160)
        results[rank] = payload
    for p in procs:
        p.join(timeout=30)
    for rank, payload in results.items():
        assert "error" not in payload, f"rank {rank}: {payload.get('error')}"
        for key, err in payload.items():
            assert err < 0.03, f"rank {rank} {key}: err {err}"


def _sp_prefill_rank(rank: int, world: int, port: int, q):
    import os
    import sys

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
        import torch

        from bobrapet_amd.models.llama import LlamaModel
        from bobrapet_amd.parallel import group

        group.init_distributed(backend="gloo")
        torch.manual_seed(0)
        m = LlamaModel("llama-tiny", device="cpu")
        S_loc = 16
        gen = torch.Generator().manual_seed(9)
        ids = torch.randint(0, m.cfg.vocab_size, (1, S_loc * world), generator=gen)
        full = m.prefill(ids, logits_for_all=True)
        lo, hi = rank * S_loc, (rank + 1) * S_loc
        local = m.prefill(
            ids[:, lo:hi].contiguous(), logits_for_all=True, seq_shard=(rank, world)
        )
        err = (local.float() - full[:, lo:hi].float()).abs().max().item()
        scale = full.abs().max().item()
        q.put((rank, {"err": err, "scale": scale}))
        group.teardown()
    except Exception as exc:
        import traceback

        q.put((rank, {"error": f"{exc}\n{traceback.format_exc()}"}))


@pytest.mark.timeout(180)
def test_sequence_parallel_prefill_matches_full():
    """llama-tiny sequence-parallel prefill (ring attention per layer,
    rope positions offset per shard) == single-rank full prefill."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [
        ctx.Process(target=_sp_prefill_rank, args=(r, world, port, q)) for r in range(world)
    ]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, payload = q.get(timeout=160)
        results[rank] = payload
    for p in procs:
        p.join(timeout=30)
    for rank, payload in results.items():
        assert "error" not in payload, f"rank {rank}: {payload.get('error')}"
        assert payload["err"] < 0.05 * max(payload["scale"], 1.0), payload


def _ulysses_rank(rank: int, world: int, port: int, q):
    import os
    import sys

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
        import torch

        from bobrapet_amd import ops
        from bobrapet_amd.parallel import group
        from bobrapet_amd.parallel.ulysses_attention import ulysses_attention

        group.init_distributed(backend="gloo")
        torch.manual_seed(11)
        B, S, Hq, Hkv, D = 2, 40, 4, 2, 64
        S_glob = S * world
        qg = torch.randn(B, S_glob, Hq, D, dtype=torch.bfloat16)
        kg = torch.randn(B, S_glob, Hkv, D, dtype=torch.bfloat16)
        vg = torch.randn_like(kg)
        res = {}
        for causal in (True, False):
            full = ops.attn_prefill(qg, kg, vg, None, causal)
            lo, hi = rank * S, (rank + 1) * S
            out = ulysses_attention(
                qg[:, lo:hi].contiguous(),
                kg[:, lo:hi].contiguous(),
                vg[:, lo:hi].contiguous(),
                causal=causal,
            )
            res[f"causal={causal}"] = (out.float() - full[:, lo:hi].float()).abs().max().item()
        q.put((rank, res))
        group.teardown()
    except Exception as exc:
        import traceback

        q.put((rank, {"error": f"{exc}\n{traceback.format_exc()}"}))


@pytest.mark.timeout(180)
def test_ulysses_attention_matches_full():
    """Head-parallel Ulysses attention == single-rank full attention
    (2 ranks, gloo all-gather fallback for the all-to-all)."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ulysses_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, payload = q.get(timeout=160)
        results[rank] = payload
    for p in procs:
        p.join(timeout=30)
    for rank, payload in results.items():
        assert "error" not in payload, f"rank {rank}: {payload.get('error')}"
        for key, err in payload.items():
            assert err < 0.03, f"rank {rank} {key}: err {err}"


def _sp_engram_rank(rank: int, world: int, port: int, q):
    import os
    import sys

    os.environ.update(
        {
            "RANK": str(rank),
            "WORLD_SIZE": str(world),
            "LOCAL_RANK": str(rank),
            "MASTER_ADDR": "127.0.0.1",
            "MASTER_PORT": str(port),
            # a CPU test (gloo, fp32 CPU reference): on a box with fewer
            # GPUs than ranks the engram must not land on a shared GPU
            "HIP_VISIBLE_DEVICES": "-1",
        }
    )
    try:
        sys.path.insert(0, REPO)
        import torch

        from bobrapet_amd.engine import EngineConfig, RunEngine
        from bobrapet_amd.enums import Phase
        from bobrapet_amd.models.llama import LlamaModel
        from bobrapet_amd.parallel import group

        group.init_distributed(backend="gloo")
        S_loc = 12
        gen = torch.Generator().manual_seed(3)
        full_ids = torch.randint(0, 1024, (1, S_loc * world), generator=gen)
        lo, hi = rank * S_loc, (rank + 1) * S_loc
        eng = RunEngine(EngineConfig(cpu_workers=2)).start()
        eng.apply_yaml(
            """
kind: EngramTemplate
metadata: {name: llm-tpl}
spec: {builtin: llm-infer}
---
kind: Engram
metadata: {name: llm}
spec:
  templateRef: {name: llm-tpl}
  with: {model: llama-tiny}
---
kind: Story
metadata: {name: sp}
spec:
  steps:
    - name: infer
      ref: {name: llm}
      with:
        promptIds: "{{ inputs.ids }}"
        sequenceParallel: true
  output: {tokens: "{{ steps.infer.output.tokens }}"}
"""
        )
        run = eng.run_story(
            "default/sp", {"ids": full_ids[:, lo:hi].tolist()}, timeout=120
        )
        assert run.phase == Phase.SUCCEEDED, run.error
        # single-rank reference: last-position argmax of the FULL sequence,
        # which only the LAST rank's shard output can reproduce
        ref_model = LlamaModel("llama-tiny", device="cpu")
        want = ref_model.prefill(full_ids).argmax(dim=-1, keepdim=True)
        got = torch.tensor(run.output["tokens"])
        res = {"match": bool((rank != world - 1) or torch.equal(got, want))}
        q.put((rank, res))
        eng.stop()
        group.teardown()
    except Exception as exc:
        import traceback

        q.put((rank, {"error": f"{exc}\n{traceback.format_exc()}"}))


@pytest.mark.timeout(240)
def test_llm_infer_engram_sequence_parallel():
    """The llm-infer engram's sequenceParallel knob: each rank submits its
    shard through a full engine Story; the last rank's argmax equals a
    single-rank full-sequence prefill."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [
        ctx.Process(target=_sp_engram_rank, args=(r, world, port, q)) for r in range(world)
    ]
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
        assert payload["match"], f"rank {rank} output mismatch"
