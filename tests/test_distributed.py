"""The N > 1 path on CPU: two gloo processes (reference: tests/distributed/dist_harness.py).
Chains are sharded by rank with per-rank generators (base_seed + rank), sampled independently,
and read back with one all-gather; plus bench.py's multi-process plumbing under torchrun."""

import json
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_SEED = 4321
N_TOTAL, DIM, K = 101, 6, 9  # 101 chains: uneven shards (51 + 50)


def _worker(rank, world, init_file, out_dir):
    os.environ["CUDA_VISIBLE_DEVICES"] = ""
    sys.path.insert(0, ROOT)
    import torchebm_amd as ta
    from torchebm_amd.utils import all_gather_cat, broadcast_tensor, get_rank, get_world_size, shard_rows

    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        assert get_world_size() == world and get_rank() == rank
        start, count = shard_rows(N_TOTAL)
        x_all = torch.randn(N_TOTAL, DIM, generator=torch.Generator().manual_seed(0))
        sampler = ta.LangevinDynamics(ta.DoubleWellModel(), step_size=0.01)
        gen = torch.Generator().manual_seed(BASE_SEED + rank)
        mine = sampler.sample(x=x_all[start : start + count], n_steps=K, generator=gen)
        # equal-sized shards are required by all_gather: pad the short shard, trim after
        pad = (N_TOTAL + world - 1) // world
        padded = torch.zeros(pad, DIM)
        padded[:count] = mine
        gathered = all_gather_cat(padded)
        assert gathered.shape == (world * pad, DIM)
        t = broadcast_tensor(torch.full((3,), float(rank + 7)), src=1)
        # PCD buffer mixing is an exact partition of the union (reference test_pcd_buffer_ranks.py:83-105)
        cd = ta.ContrastiveDivergence(ta.DoubleWellModel(), sampler, k_steps=1, persistent=True, buffer_size=8, init_steps=0)
        cd.get_start_points(torch.zeros(4, DIM))
        cd.replay_buffer.copy_((torch.arange(8.0) + 100 * rank)[:, None].expand(8, DIM))
        cd.mix_buffer_across_ranks(generator=torch.Generator().manual_seed(5))
        # sharded diagnostics: one all-reduce turns per-rank moments into the population's
        from torchebm_amd.utils import all_reduce_diagnostics

        _, dloc = sampler.sample(x=x_all[start : start + count], n_steps=6, thin=2, return_diagnostics=True,
                                 generator=torch.Generator().manual_seed(BASE_SEED + rank))
        dglob = all_reduce_diagnostics(dloc, count)
        # pipelined read-back: 4 row blocks, gather of block i overlapped with the sampling of block i+1
        from torchebm_amd.utils import sample_and_gather

        even = x_all[rank * 48 : (rank + 1) * 48]
        loc, gat = sample_and_gather(sampler, even, K, pieces=4, generator=torch.Generator().manual_seed(BASE_SEED + rank))
        torch.save({"start": start, "count": count, "mine": mine, "gathered": gathered, "bcast": t,
                    "mixed": cd.replay_buffer[:, 0].clone(), "pipe_local": loc, "pipe_gathered": gat.clone(), "dglob": dglob},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_sharded_sampling_and_readback_gloo():
    world = 2
    with tempfile.TemporaryDirectory() as tmp:
        init_file = os.path.join(tmp, "rdv")
        mp.start_processes(_worker, args=(world, init_file, tmp), nprocs=world, join=True, start_method="spawn")
        res = [torch.load(os.path.join(tmp, f"rank{r}.pt")) for r in range(world)]
    sys.path.insert(0, ROOT)
    import torchebm_amd as ta

    # shards tile [0, N_TOTAL) contiguously
    assert res[0]["start"] == 0 and res[0]["count"] == 51 and res[1]["start"] == 51 and res[1]["count"] == 50
    # every rank's shard equals what a single process computes for those rows with that rank's seed
    x_all = torch.randn(N_TOTAL, DIM, generator=torch.Generator().manual_seed(0))
    sampler = ta.LangevinDynamics(ta.DoubleWellModel(), step_size=0.01)
    for r in range(world):
        s, c = res[r]["start"], res[r]["count"]
        want = sampler.sample(x=x_all[s : s + c], n_steps=K, generator=torch.Generator().manual_seed(BASE_SEED + r))
        assert torch.equal(res[r]["mine"], want)
    # the gather is rank-ordered and identical on every rank
    assert torch.equal(res[0]["gathered"], res[1]["gathered"])
    g = res[0]["gathered"]
    assert torch.equal(g[:51], res[0]["mine"]) and torch.equal(g[51 : 51 + 50], res[1]["mine"])
    # different ranks, different noise
    assert not torch.equal(res[0]["mine"][:50], res[1]["mine"][:50])
    assert torch.equal(res[0]["bcast"], torch.full((3,), 8.0)) and torch.equal(res[1]["bcast"], torch.full((3,), 8.0))
    # sharded diagnostics == diagnostics of the concatenated population
    trajs = []
    for r in range(world):
        s_, c_ = res[r]["start"], res[r]["count"]
        trajs.append(sampler.sample(x=x_all[s_ : s_ + c_], n_steps=6, thin=2, return_trajectory=True,
                                    generator=torch.Generator().manual_seed(BASE_SEED + r)))
    pop = torch.cat(trajs)                                   # [N_TOTAL, 3, DIM]
    for r in range(world):
        dg = res[r]["dglob"]
        torch.testing.assert_close(dg["mean"], pop.mean(dim=0), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(dg["var"], pop.var(dim=0, unbiased=False), rtol=1e-4, atol=1e-6)
        want_e = torch.stack([ta.DoubleWellModel()(pop[:, j]).mean() for j in range(3)])
        torch.testing.assert_close(dg["energy"], want_e, rtol=1e-5, atol=1e-5)
    # pipelined read-back: every rank sees every rank's chains, in order; blocks = separate sample() calls
    for r in range(world):
        assert res[r]["pipe_gathered"].shape == (world, 4, 12, DIM)
        for q in range(world):
            assert torch.equal(res[r]["pipe_gathered"][q].reshape(48, DIM), res[q]["pipe_local"])
        gen = torch.Generator().manual_seed(BASE_SEED + r)
        want = torch.cat([sampler.sample(x=x_all[r * 48 + 12 * i : r * 48 + 12 * (i + 1)], n_steps=K, generator=gen) for i in range(4)])
        assert torch.equal(res[r]["pipe_local"], want)
    union = torch.cat([res[0]["mixed"], res[1]["mixed"]]).sort().values
    assert torch.equal(union, torch.cat([torch.arange(8.0), torch.arange(8.0) + 100]))
    assert not torch.equal(res[0]["mixed"].sort().values, torch.arange(8.0))  # rows actually moved


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_contract_two_processes_cpu():
    """bench.py launched exactly as the driver does for N > 1 (torch.distributed.run, one process
    per device), on the CPU plumbing path with gloo: one JSON line from rank 0, aggregate value; with --full, the
    read-back breakdown."""
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--device", "cpu", "--n-chains", "256", "--dim", "8", "--k", "3", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stderr[-3000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["warmup"] == 1 and rec["scaling"] == "weak"
    assert rec["metric"] == "MCMC chain-steps/sec" and rec["unit"] == "chain-steps/s" and rec["higher_is_better"] is True
    assert rec["value"] == pytest.approx(2 * 256 * 3 * 2 / (rec["ms_per_step"] * 2 / 1e3), rel=1e-6)
    assert rec["cpu_baseline"] is None  # rank 0 at N = 1 only
    # the N > 1 line says why it is what it is: the read-back's exposed time, the collective alone, per-rank spread
    rb = rec["readback"]
    assert rb["bytes_per_rank"] == 256 * 8 * 4 and rb["gathered_bytes_per_rank"] == 2 * 256 * 8 * 4
    assert rb["plain_step_ms"] > 0 and rb["step_with_pipelined_readback_ms"] > 0 and rb["exposed_ms"] >= 0
    assert rb["allgather_alone_ms"] > 0 and rb["allgather_error"] is None
    assert rb["algbw_GBps"] == pytest.approx(256 * 8 * 4 / (rb["allgather_alone_ms"] * 1e-3) / 1e9, rel=1e-6)
    assert len(rb["per_rank_ms_per_step"]["all"]) == 2 and rb["per_rank_ms_per_step"]["min"] <= rb["per_rank_ms_per_step"]["max"]
    assert rb["per_rank_kernel_ms"] is None  # event times exist on the GPU only


def test_bench_config4_preset_is_baseline_config_4s_shard():
    """--config 4 times BASELINE configs[3]'s per-GPU shard (2^20 x 128, k = 500); checked on the argument level only
    (the shape is far beyond a CPU test)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    argv, sys.argv = sys.argv, ["bench.py", "--config", "4"]
    try:
        a = mod.parse()
    finally:
        sys.argv = argv
    assert a.config == 4 and (a.n_chains, a.dim, a.k) == (1 << 20, 128, 500)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        a = mod.parse()
    finally:
        sys.argv = argv
    assert (a.n_chains, a.dim, a.k) == (1 << 20, 64, 200)  # BASELINE configs[1]


def test_bench_contract_eight_processes_cpu_config4_shape():
    """the exact 8-rank code path of BASELINE configs[3] (--config 4: dim 128, k steps per call, the
    pipelined read-back of every rank's shard, the rank-ordered gather, per-rank spread), executed once -- on 8 gloo CPU ranks at
    a reduced shard (64 chains per rank, k = 3), launched as the driver launches N > 1.  Reference for the semantics:
    torchebm/utils/distributed.py:43-70 (rank-ordered concatenation), tests/distributed/test_generator_ranks.py:38-51."""
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1",
           "--device", "cpu", "--config", "4", "--n-chains", "64", "--k", "3", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stderr[-3000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 8 and rec["config"]["ranks"] == 8 and rec["config"]["backend_world_size"] == 8
    assert rec["config"]["backend"] == "gloo" and rec["config"]["dim"] == 128 and rec["config"]["k_steps"] == 3
    assert rec["value"] == pytest.approx(8 * 64 * 3 * 2 / (rec["ms_per_step"] * 2 / 1e3), rel=1e-6)
    rb = rec["readback"]
    assert rb["bytes_per_rank"] == 64 * 128 * 4 and rb["gathered_bytes_per_rank"] == 8 * 64 * 128 * 4
    assert rb["allgather_error"] is None and rb["allgather_alone_ms"] > 0
    assert rb["algbw_GBps"] == pytest.approx(7 * 64 * 128 * 4 / (rb["allgather_alone_ms"] * 1e-3) / 1e9, rel=1e-6)
    assert len(rb["per_rank_ms_per_step"]["all"]) == 8
    assert rec["config"]["readback"] is not None


def test_bench_contract_single_process_cpu():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--device", "cpu",
           "--n-chains", "128", "--dim", "4", "--k", "2", "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in rec
    assert rec["n_gpus"] == 1 and rec["dtype"] == "f32" and rec["data"] == "synthetic" and rec["vs_baseline"] is None


def test_bench_self_launches_n_ranks_without_torchrun():
    """`python bench.py --gpus 2` with no torchrun environment must start the two ranks itself (VERDICT r1:
    it used to run one process silently) -- same harness shape as the reference's
    tests/distributed/dist_harness.py:72-84, on the gloo plumbing path."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--device", "cpu",
           "--n-chains", "256", "--dim", "8", "--k", "3"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stderr[-3000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["ranks"] == 2 and rec["config"]["backend"] == "gloo"
    assert "self-launch" in rec["config"]["launcher"]
    assert rec["value"] == pytest.approx(2 * 256 * 3 * 2 / (rec["ms_per_step"] * 2 / 1e3), rel=1e-6)


def test_bench_refuses_more_gpus_than_visible():
    """Fewer visible GPUs than --gpus: no JSON line, a non-zero exit and a message -- never an N-GPU number from
    fewer devices."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    have = torch.cuda.device_count()
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(have + 2), "--steps", "1", "--warmup", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode != 0
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert "GPU(s) are visible" in out.stderr


def test_unsharded_is_duck_typed():
    """utils.unsharded (reference: utils/distributed.py:129-175): toggles reshard-after-forward on modules that have the
    switch (FSDP2), restores it on exit even when the block raises, and passes every other module through."""
    import torch.nn as nn

    from torchebm_amd.utils import unsharded

    calls = []

    class Sharded(nn.Linear):
        def set_reshard_after_forward(self, flag, recurse=True):
            calls.append((flag, recurse))

    m = Sharded(2, 2)
    with unsharded(m, recurse=False) as inside:
        assert inside is m and calls == [(False, False)]
    assert calls == [(False, False), (True, False)]
    with pytest.raises(RuntimeError):
        with unsharded(m):
            raise RuntimeError("boom")
    assert calls[-1] == (True, True)
    plain = nn.Linear(2, 2)
    with unsharded(plain) as inside:
        assert inside is plain
