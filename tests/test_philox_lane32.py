"""The lean Langevin loop's Philox at 32-bit counter words (ebm_common.h PhiloxLane32) is the 64-bit philox4x32_10 with both
counter high words 0, bit for bit: 10^6 random (group, step, key), every pair of edge words of group and step, and the Random123
known answer whose counter high words are zero.  Host code compiled by hipcc; no GPU."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_philox_lane32_equals_philox4x32_10(tmp_path):
    exe = tmp_path / "philox_lane32_host"
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "philox_lane32_host.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=600)
    out = subprocess.run([str(exe), "1000000", "0x5eed"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok 1000101", out.stdout
