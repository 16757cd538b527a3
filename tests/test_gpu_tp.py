"""GPU, tensor parallel 2 (two processes sharing the one GPU of the test box, gloo for the
collectives): the whole TP path that `bench.py --gpus N` runs over RCCL -- column/row-parallel
quantised linears with sharded Marlin weights and scales, head-sharded paged attention and KV cache,
vocab-parallel embedding / lm_head + gather -- must reproduce the single-process model."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

QUANT = dict(method="gptq_marlin", bits=4, group_size=128)
BATCH, PROMPT, STEPS = 2, 24, 4


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(runner, try_capture=False, logits=None):
    """prefill + greedy decode; returns the token ids per step (and appends each decode step's logits to `logits`)"""
    runner.keep_logits = logits is not None
    runner.setup_batch(BATCH, PROMPT, STEPS + 4)
    first = runner.prefill(PROMPT, seed=7)
    toks = [first.cpu()]
    runner.input_ids.copy_(first)
    if try_capture:
        # gloo collectives cannot be captured into a hipGraph: capture() must say so WITHOUT entering a
        # capture (a stream synchronisation by gloo's helper thread inside one left the runtime in a
        # state that segfaulted the next eager all_reduce in round 1), keep the step inputs and leave
        # the runner usable
        assert runner.step_is_capturable() is False
        assert runner.capture() is False
        runner.input_ids.copy_(first)
    for _ in range(STEPS):
        nxt = runner.decode_step()
        toks.append(nxt.cpu())
        if logits is not None:
            logits.append(runner.last_logits.cpu())
    return torch.stack(toks)


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
        import torch.distributed as dist
        from neural_magic_vllm_amd import distributed as nd
        from neural_magic_vllm_amd.worker import decode_runner as dr
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        nd.initialize_model_parallel(world, backend="gloo", local_rank=0)
        dev = torch.device("cuda:0")
        runner = dr.DecodeRunner(dr.TINY, dev, torch.bfloat16, QUANT, dr.CacheConfig(16, "auto"))
        assert runner.tp_size == world
        toks = _run(runner, try_capture=True)
        if rank == 0:
            q.put(("ok", toks.tolist()))
        nd.destroy_model_parallel()
        dist.destroy_process_group()
        if rank != 0:
            q.put(("ok", None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(("err", f"rank {rank}: {e!r}\n{traceback.format_exc()}"))


@pytest.mark.parametrize("world", [2, 4])
def test_tp_matches_single_process(gpu_device, world):
    """world = 4 > the tiny model's 2 KV heads: also covers KV-head replication (llama.py:109-117)"""
    from neural_magic_vllm_amd.worker import decode_runner as dr
    ref_runner = dr.DecodeRunner(dr.TINY, gpu_device, torch.bfloat16, QUANT, dr.CacheConfig(16, "auto"))
    ref_logits = []
    ref = _run(ref_runner, logits=ref_logits).tolist()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    errs = [m for s, m in res if s == "err"]
    assert not errs, errs
    got = [m for s, m in res if m is not None][0]
    # greedy tokens: TP changes the fp32 summation order of the row-parallel GEMMs, so a sequence may leave the
    # single-process one -- but only at a NEAR TIE of the single-process logits: where a sequence first differs,
    # the token TP chose must be within 2 bf16 ulps of the top logit there (later tokens of that sequence follow
    # a different context and are not compared).  The prefill token must agree.
    assert got[0] == ref[0]
    for b in range(BATCH):
        for step in range(1, STEPS + 1):
            if got[step][b] == ref[step][b]:
                continue
            row = ref_logits[step - 1][b]
            top, alt = row[ref[step][b]].item(), row[got[step][b]].item()
            assert top - alt <= 2 * 2.0**-8 * abs(top), \
                f"seq {b} step {step}: TP token {got[step][b]} (logit {alt}) is no near tie of {ref[step][b]} ({top})"
            break


def _bench_cmd(root, extra):
    return [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--model", "tiny",
            "--batch", "4", "--context", "40"] + extra


def _one_json_line(res):
    import json
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("custom_ar", ["0", "force"])
def test_bench_py_multi_rank_rehearsal(gpu_device, custom_ar):
    """bench.py's N > 1 path end to end (driver contract: torch.distributed.run, one JSON line from
    rank 0) rehearsed with two ranks on this box's one GPU and gloo collectives, tiny model, graph
    capture left ON: with the collectives on gloo the runner decides for eager without entering a
    capture; with the P2P all-reduce the step holds no process-group collective and is captured."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NMV_BENCH_DIST_BACKEND="gloo", NMV_BENCH_SINGLE_DEVICE="1",
               NMV_CUSTOM_ALLREDUCE=custom_ar, NMV_CUSTOM_AR_TIMEOUT_MS="30000", NMV_BENCH_COMPARE_RCCL="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + _bench_cmd(root, ["--full"])
    out = _one_json_line(subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600))
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["value"] > 0 and out["scaling"] == "strong"
    assert out["config"]["parallelism"] == "tp2" and out["timed_region_s"] > 0
    if custom_ar == "0":
        assert out["config"]["hip_graph"] is False and "process group" in out["config"]["all_reduce"]
    else:
        assert out["config"]["hip_graph"] is True and "p2p" in out["config"]["all_reduce"]
        # the same step over the process group, measured in the same run
        assert out["process_group_path"]["value"] > 0 and out["process_group_path"]["hip_graph"] is False


def test_bench_py_starts_its_own_ranks(gpu_device):
    """`python bench.py --gpus 2` with no WORLD_SIZE: the script launches the two ranks itself (before it
    touches the GPU) and relays rank 0's line; a world size that does not match --gpus is refused"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(NMV_BENCH_DIST_BACKEND="gloo", NMV_BENCH_SINGLE_DEVICE="1", NMV_CUSTOM_ALLREDUCE="force",
               NMV_CUSTOM_AR_TIMEOUT_MS="30000")
    out = _one_json_line(subprocess.run([sys.executable] + _bench_cmd(root, ["--no-sweep"]), env=env,
                                        capture_output=True, text=True, timeout=600))
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "tp2"
    bad = subprocess.run([sys.executable] + _bench_cmd(root, []), env=dict(env, WORLD_SIZE="1", RANK="0"),
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "WORLD_SIZE" in bad.stderr and not bad.stdout.strip()


def test_bench_py_llama70b_tp8_geometry_rehearsal(gpu_device):
    """`bench.py --model llama3-70b --gpus 8` as a tested code path: the same script and launch contract with the
    TP = 8 per-rank head geometry of Llama-3-70B (8 query heads + 1 KV head per rank) at toy widths and two ranks on
    this box's one GPU; the line carries what an auditor of a multi-GPU run needs (ranks seen, device per rank, P2P
    self-test verdict, collective library version, weight bytes per rank)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NMV_BENCH_DIST_BACKEND="gloo", NMV_BENCH_SINGLE_DEVICE="1",
               NMV_CUSTOM_ALLREDUCE="force", NMV_CUSTOM_AR_TIMEOUT_MS="30000")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(root, "bench.py"),
           "--gpus", "2", "--steps", "4", "--warmup", "2", "--model", "tiny-70b", "--batch", "4", "--context", "40"]
    out = _one_json_line(subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600))
    cfg = out["config"]
    assert out["n_gpus"] == 2 and cfg["parallelism"] == "tp2" and cfg["hip_graph"] is True
    assert cfg["ranks_seen"] == 2 and [r["rank"] for r in cfg["ranks"]] == [0, 1]
    assert all(r["p2p_selftest"] == "passed" and "device_name" in r for r in cfg["ranks"])
    assert "rccl_version" in cfg and cfg["dist_backend"] == "gloo" and cfg["weights_gb_per_rank"] > 0


def test_bench_py_failed_capture_restarts_fresh_ranks(gpu_device):
    """a rank that fails BEFORE the eager warm-up of the capture (injected) is fatal for the whole group -- no rank continues
    eagerly in the same process -- and costs its peers about ONE bounded P2P wait, not one per collective of the warm-up
    (the rendezvous fails fast on the sticky error word, the error word is read after the first eager step); the
    self-launching parent, which never touched the GPU, then starts fresh ranks with --no-graph: one JSON line,
    hip_graph false"""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    bound_s = 6
    env.update(NMV_BENCH_DIST_BACKEND="gloo", NMV_BENCH_SINGLE_DEVICE="1", NMV_CUSTOM_ALLREDUCE="force",
               NMV_CUSTOM_AR_TIMEOUT_MS=str(bound_s * 1000), NMV_TEST_FAIL_CAPTURE_RANK="1")
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable] + _bench_cmd(root, ["--no-sweep"]), env=env, capture_output=True, text=True,
                         timeout=900)
    elapsed = time.perf_counter() - t0
    out = _one_json_line(res)
    assert out["config"]["hip_graph"] is False and out["n_gpus"] == 2
    assert "starting fresh ranks with --no-graph" in res.stderr
    # rank 1 failed by injection; rank 0 either captured (and learnt of the failure) or ran into its one bounded wait
    assert ("capture of the decode step failed on rank(s) [1]" in res.stderr
            or "capture of the decode step failed on rank(s) [0, 1]" in res.stderr)
    # two launches of the ranks (imports, weights, the fresh run) plus ONE bound; 65 collectives x the bound would be 390 s
    assert elapsed < 150 + bound_s, elapsed
