"""bench.py's two modes: a plain run measures the headline and nothing else; --full adds what takes runs of its own
(roofline probes, CPU baselines, the other BASELINE configs, the N > 1 read-back breakdown)."""

import json
import os
import socket
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "readback", "roofline", "cpu_baseline")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, timeout, env=None):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stderr[-3000:]
    return json.loads(lines[0])


def test_plain_run_skips_the_cpu_baseline_cpu():
    """No --no-cpu-baseline: a plain run still does not time the CPU baseline (it is --full's)."""
    rec = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--device", "cpu",
                "--n-chains", "128", "--dim", "4", "--k", "2"], timeout=600)
    for key in HEADLINE:
        assert key in rec
    assert "extra" not in rec
    assert rec["cpu_baseline"] is None and rec["readback"] is None and rec["config"]["full"] is False
    assert rec["value"] == pytest.approx(128 * 2 * 2 / (rec["ms_per_step"] * 2 / 1e3), rel=1e-6)


def test_plain_run_two_processes_has_no_readback_breakdown_cpu():
    """N > 1 without --full: the timed run is the same (aggregate value, read-back inside the timed region), the
    breakdown measured behind it is not taken."""
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--device", "cpu", "--n-chains", "256", "--dim", "8", "--k", "3"]
    rec = _run(cmd, timeout=600, env=env)
    assert rec["n_gpus"] == 2 and rec["config"]["ranks"] == 2 and rec["config"]["full"] is False
    assert rec["value"] == pytest.approx(2 * 256 * 3 * 2 / (rec["ms_per_step"] * 2 / 1e3), rel=1e-6)
    assert rec["readback"] is None and rec["cpu_baseline"] is None
    assert rec["config"]["readback"].startswith("final state all-gathered inside the timed region")


@pytest.mark.gpu
def test_plain_and_full_runs_gpu(cuda_device):
    """On the GPU: a plain run of the headline workload spends well under 30 s outside its steps and carries only the
    roofline figures of its own launches; --full (extras, CPU baseline and counter passes off) adds the probe figures."""
    steps, warmup = 5, 2
    t0 = time.perf_counter()
    rec = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
               timeout=300)
    wall = time.perf_counter() - t0
    assert wall - (steps + warmup) * rec["ms_per_step"] / 1e3 < 30.0
    assert rec["n_gpus"] == 1 and rec["config"]["full"] is False and "extra" not in rec and rec["cpu_baseline"] is None
    roof = rec["roofline"]
    assert roof["kernel_ms"] > 0 and roof["kernel_ms_per_step"]["launches"] == steps
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-9)
    assert "valu" not in roof and "measured_copy_ceiling" not in roof

    rec = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--n-chains", "65536",
                "--full", "--no-extra", "--no-cpu-baseline", "--no-traffic"], timeout=600)
    assert rec["config"]["full"] is True and "extra" not in rec
    roof = rec["roofline"]
    assert roof["kernel_ms"] > 0 and roof["valu"]["plain_valu_wave_instr_per_s"] > 0 and roof["measured_copy_ceiling"] > 0
    assert 0 < roof["bound_frac"] <= 1.0 and roof["valu_insts_per_group_step"] == 76
