"""The bench.py driver contract on the CPU fake device: one JSON line from rank 0 with the
BASELINE metric fields, single process and under torch.distributed.run (gloo, 2 ranks)."""
import json
import os
import socket
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--model", "tiny-gpt2", "--seq", "32", "--steps", "2", "--warmup", "1"]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


def _run(cmd):
    env = dict(os.environ, PYTHONPATH=REPO, MASTER_ADDR="127.0.0.1")
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return _json_lines(r.stdout)


def _check(line, n):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in line, k
    assert line["n_gpus"] == n and line["steps"] == 2 and line["warmup"] == 1
    assert line["higher_is_better"] is False and line["scaling"] == "weak"
    assert line["value"] > 0 and line["config"]["model"] == "tiny-gpt2"
    assert "synthetic" in line["data"]


def test_bench_single_process():
    lines = _run([sys.executable, "bench.py", "--gpus", "1", *ARGS])
    assert len(lines) == 1
    _check(lines[0], 1)
    # the cache policies the step's kernels ran with (defaults: LM head weight + logits nt,
    # every other GEMM write-through)
    assert lines[0]["cache_policy"] == {"lm_head": 3, "gemm": 4, "attention_flags": 0}


def test_bench_plain_run_is_headline_only_and_full_adds_the_sub_results():
    """A plain run measures the headline alone; ``--full`` adds the capped / strong sub-results
    to the same line, whose headline fields keep their meaning."""
    plain = _run([sys.executable, "bench.py", "--gpus", "1", *ARGS])[0]
    assert "capped" not in plain and "strong" not in plain and "extras_error" not in plain
    full = _run([sys.executable, "bench.py", "--gpus", "1", *ARGS, "--full", "--extra-steps", "1"])[0]
    _check(full, 1)
    assert full["capped"]["MRU_spec"]["ms_per_step"] > 0 and full["strong"]["ms_per_step"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[k] == full[k]
    assert plain["value"] == plain["ms_per_step"] and full["value"] == full["ms_per_step"]


def test_bench_dump_outputs_is_reproducible(tmp_path):
    """``--dump-outputs DIR`` writes the last timed step's outputs (the request's logits) as
    float32 ``.npy`` files; the inputs are seeded, so two runs of the same command write the
    same arrays, and they are the logits the dense reference computes from those inputs."""
    import numpy as np

    outs = []
    for d in ("a", "b"):
        _run([sys.executable, "bench.py", "--gpus", "1", *ARGS, "--dump-outputs", str(tmp_path / d)])
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["output_projection.npy"], files
        outs.append(np.load(tmp_path / d / files[0]))
    a, b = outs
    assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a, b)

    import torch
    from distributed_llm_scheduler_amd.models import reference
    from distributed_llm_scheduler_amd.parallel import runtime
    from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens

    p = runtime.plan("tiny-gpt2", world=1, scheduler="EFT", seq=32, batch=1, cost_model="bytes")
    tok = synthetic_tokens("@tokens", 32, p.cfg.vocab_size).view(1, 32)
    ref = reference.forward(p.cfg, runtime.make_store(p), tok).float().reshape(-1).numpy()
    assert a.shape == ref.shape
    assert np.abs(a - ref).max() <= 0.02 * np.abs(ref).max()


@pytest.mark.timeout(300)
def test_bench_two_ranks_gloo():
    lines = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                  "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2", *ARGS])
    assert len(lines) == 1  # rank 0 only
    _check(lines[0], 2)


@pytest.mark.timeout(300)
def test_bench_isolated_device_p2p_subrun_under_torchrun():
    """The strong device-p2p sub-result runs in child processes that form a job of their own (a
    fault there must not cost the headline line): under torchrun (agent store variables in the
    environment) the children rendezvous on rank 0's new port, rank 0's child result lands in
    the ONE line, marked isolated."""
    lines = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                  "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2", *ARGS,
                  "--full", "--extra-steps", "2", "--device-p2p-extra-cpu"])
    assert len(lines) == 1
    _check(lines[0], 2)
    sd = lines[0]["strong_device_p2p"]
    assert sd["isolated"] and "error" not in sd, sd
    assert sd["ms_per_step"] > 0 and len(sd["per_rank_ms"]) == 2 and sd["cross_gpu_bytes"] > 0


@pytest.mark.timeout(300)
def test_bench_isolated_device_p2p_subrun_crash_keeps_the_headline(monkeypatch):
    """Rank 1's child aborts (as a GPU fault would end it): rank 0's child loses its peer (or, on a
    transport that only hangs, is stopped at the sub-run's time budget); the job still prints its
    ONE line, with the sub-result's error recorded."""
    monkeypatch.setenv("DLS_TEST_CHILD_ABORT", "1")
    lines = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                  "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2", *ARGS,
                  "--full", "--extra-steps", "2", "--device-p2p-extra-cpu", "--extras-timeout", "90"])
    assert len(lines) == 1
    _check(lines[0], 2)
    sd = lines[0]["strong_device_p2p"]
    assert "error" in sd and "ms_per_step" not in sd, sd
    assert lines[0]["strong"]["ms_per_step"] > 0  # the other sub-results stand


def _torchrun(n, args):
    return _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
                 "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", str(n), *args])


MINI = ["--seq", "16", "--steps", "1", "--warmup", "1", "--no-extras"]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("config", ["gpt2m_cap", "llama_pipeline", "mixtral_expert"])
def test_bench_baseline_multi_gpu_configs(world, config):
    """BASELINE.json configs 3-5 as bench.py commands, at mini scale over 2 / 4 / 8 gloo ranks:
    ONE request DAG spanning the GPUs (--replicas 1) or pipeline micro-batches, each printing one
    JSON line with tasks completed and real cross-GPU edges / bytes.
      3: GPT-2-medium across 2 GPUs under an artificial cap  (--cap-gb, --replicas 1)
      4: Llama-3-8B pipeline placement                       (--placement pipeline)
      5: Mixtral-8x7B experts across GPUs                     (--placement expert --replicas 1)"""
    args = {
        # the reference's policy under a cap that binds (evictions + re-fills) spreads the DAG
        "gpt2m_cap": ["--model", "tiny-gpt2", "--replicas", "1", "--cap-gb", "0.0001", "--cost-model", "bytes",
                      "--scheduler", "MRU_spec"],
        "llama_pipeline": ["--model", "tiny-llama", "--placement", "pipeline"],
        "mixtral_expert": ["--model", "tiny-mixtral", "--placement", "expert", "--replicas", "1"],
    }[config]
    lines = _torchrun(world, args + MINI)
    assert len(lines) == 1
    ln = lines[0]
    assert ln["n_gpus"] == world and ln["rccl_world"] == world and len(ln["per_rank_ms"]) == world
    assert ln["tasks_completed"] == ln["tasks_total"] > 0
    assert ln["cross_gpu_edges"] > 0 and ln["cross_gpu_bytes"] > 0, "the DAG must span GPUs"
    assert ln["value"] == max(ln["per_rank_ms"])


@pytest.mark.timeout(600)
def test_bench_extras_two_ranks():
    """The ``--full`` extras over 2 gloo ranks: the reference's experiment executed — ONE DAG over the
    two ranks under the 80 % regime with the reference's 60/40 node split (MRU_spec / EFT / DFS,
    real cross-GPU edges), the per-GPU-replica form, and the strong-scaling pipeline run."""
    lines = _torchrun(2, ["--model", "tiny-gpt2", "--seq", "16", "--steps", "1", "--warmup", "1", "--full",
                          "--extra-steps", "1", "--strong-mb", "4"])
    ln = lines[0]
    cap = ln["capped"]
    assert cap["memory_regime"] == 0.8 and cap["cost_model"] == "reference" and cap["replicas"] == 1
    assert len(cap["mem_cap_gb_per_gpu"]) == 2
    assert abs(cap["mem_cap_gb_per_gpu"][0] / cap["mem_cap_gb_per_gpu"][1] - 1.5) < 1e-6  # 60 / 40
    for s in ("MRU_spec", "EFT", "DFS"):
        assert cap[s]["ms_per_step"] > 0 and cap[s]["tasks_total"] == 19
    assert cap["MRU_spec"]["tasks_completed"] == 19 and cap["MRU_spec"]["cross_gpu_edges"] > 0
    assert cap["MRU_spec"]["cross_gpu_bytes"] > 0
    assert cap["DFS"]["tasks_completed"] < 19  # the reference's DFS fails tasks at 80 %
    rep = ln["capped_replica"]
    assert rep["replicas"] == 2
    assert rep["MRU_spec"]["tasks_completed"] == rep["MRU_spec"]["tasks_total"]
    assert ln["strong"]["cross_gpu_edges"] > 0 and ln["strong"]["micro_batches"] == 4
    # EFT keeps different equal groups resident on the two replicas: a group one rank streams is
    # re-filled from the other rank's arena (RCCL p2p) rather than from the host
    assert rep["EFT"]["peer_fill_gb_per_step"] > 0
    assert rep["EFT"]["peer_fill_gb_per_step"] <= rep["EFT"]["refill_gb_per_step"]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 4, 8])
def test_capped_one_dag_matches_reference_completions(world):
    """The reference's experiment on the REAL GPT-2 DAG (99 tasks), planned as bench.py's capped
    sub-result plans it: ONE DAG over N nodes at the 80 % regime with the reference's node split
    and cost model. Completion counts equal what running the reference's own schedulers gives
    for the same DAG and nodes (/root/reference/schedulers.py + simulation.py:161-214, measured:
    MRU_spec 99 at every N; DFS 79 / 74 / 66 and Critical 79 / 77 / 73 at N = 2 / 4 / 8)."""
    from distributed_llm_scheduler_amd.eval.execute import regime_node_spec
    from distributed_llm_scheduler_amd.parallel import runtime

    ref = {2: {"DFS": 79, "Critical": 79, "MRU_spec": 99}, 4: {"DFS": 74, "Critical": 77, "MRU_spec": 99},
           8: {"DFS": 66, "Critical": 73, "MRU_spec": 99}}[world]
    spec = regime_node_spec("gpt2", 0.8, world)
    for sched, want in ref.items():
        p = runtime.plan("gpt2", world=world, scheduler=sched, cap_gb=[m for m, _ in spec],
                         node_speeds=[v for _, v in spec], cost_model="reference")
        assert p.completed == want, (sched, p.completed, want)
        assert p.stats["cross_gpu_edges"] > 0
    p = runtime.plan("gpt2", world=world, scheduler="EFT", cap_gb=[m for m, _ in spec],
                     node_speeds=[v for _, v in spec], cost_model="reference")
    assert p.completed == 99


def test_bench_self_launch_two_ranks():
    """`python bench.py --gpus 2` with no launcher starts its own 2 rank processes (rendezvous on
    127.0.0.1) and reports n_gpus 2 from a 2-rank job."""
    lines = _run([sys.executable, "bench.py", "--gpus", "2", *ARGS, "--no-extras"])
    assert len(lines) == 1
    _check(lines[0], 2)
    assert lines[0]["rccl_world"] == 2 and len(lines[0]["per_rank_ms"]) == 2


def test_bench_refuses_world_mismatch():
    """A job whose world size is not --gpus exits non-zero instead of reporting another N."""
    env = dict(os.environ, PYTHONPATH=REPO, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", *ARGS, "--no-extras"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and not _json_lines(r.stdout)


@pytest.mark.timeout(300)
def test_bench_extras_watchdog_keeps_headline():
    """Sub-results that do not finish in --extras-timeout never cost the headline: every rank's
    watchdog fires, rank 0 prints ONE line with the headline and the extras marked unfinished,
    and the job exits 0 (2 gloo ranks)."""
    lines = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                  "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2", *ARGS,
                  "--full", "--extras-timeout", "0.01"])
    assert len(lines) == 1
    _check(lines[0], 2)
    assert "unfinished" in lines[0]["extras_error"]


# ------------------------------------------------- device transport: a timed-out wait fails loudly
RUN_DEV = [sys.executable, "-m", "distributed_llm_scheduler_amd", "run", "--placement", "pipeline", "--replicas",
           "2", "--loopback", "2", "--transport", "device", "--steps", "2", "--warmup", "1"]


def _cli(extra, env_extra, device_args):
    env = dict(os.environ, PYTHONPATH=REPO, **env_extra)
    r = subprocess.run(RUN_DEV + device_args + extra, cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=300)
    return r.returncode, _json_lines(r.stdout), r.stderr


@pytest.mark.parametrize("drop", [False, True])
def test_cli_run_device_transport_timeout_exits_nonzero_cpu(drop):
    """``run --loopback 2 --transport device`` on the CPU (devp2p.HostP2PWorld): with every
    notify it prints a valid line and exits 0; with the first message's notify dropped
    (DLS_P2P_DROP_NOTIFY, negative control) the consumer's pull times out, the executor raises
    TransportError naming the rank and the edge, and the CLI exits 3 with ``valid: false``."""
    env = {"DLS_P2P_TIMEOUT_S": "0.5"}
    if drop:
        env["DLS_P2P_DROP_NOTIFY"] = "0"
    rc, lines, err = _cli(["--model", "tiny-gpt2", "--seq", "16"], env, ["--device", "cpu"])
    assert len(lines) == 1, err[-3000:]
    if drop:
        assert rc == 3 and lines[0]["valid"] is False, (rc, lines, err[-2000:])
        e = lines[0]["error"]
        # the consumer (rank 1) names the edge; its producer's ack wait may be reported first
        assert "timed out" in e and ("slot 0" in e or e.startswith("rank 0")), e
    else:
        assert rc == 0 and lines[0]["valid"] is True and lines[0]["p2p_errors"] == [0, 0], (rc, err[-2000:])


@pytest.mark.gpu
@pytest.mark.isolated
@pytest.mark.timeout(280)
@pytest.mark.parametrize("drop", [False, True])
def test_cli_run_device_transport_timeout_exits_nonzero_gpu(drop):
    """The same on one MI355X: two ranks of one process, each rank's step one hipGraph with the
    edges moved by kernels; a dropped notify makes the pull kernel give up into the error word,
    the CLI reads it after the timed steps and exits 3."""
    env = {"DLS_P2P_TIMEOUT_S": "0.2", "GPU_MAX_HW_QUEUES": "16"}
    if drop:
        env["DLS_P2P_DROP_NOTIFY"] = "0"
    rc, lines, err = _cli(["--model", "mini-gpt2", "--seq", "64"], env, [])
    assert len(lines) == 1, err[-3000:]
    if drop:
        assert rc == 3 and lines[0]["valid"] is False, (rc, lines, err[-2000:])
        assert "timed out" in lines[0]["error"] and lines[0]["error"].startswith("rank "), lines[0]["error"]
    else:
        assert rc == 0 and lines[0]["valid"] is True and lines[0]["p2p_errors"] == [0, 0], (rc, err[-2000:])
