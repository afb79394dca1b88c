"""examples/convergence_cd_negatives.py runs to completion at its reduced size on the CPU and prints what it promises: max split
R-hat, min ESS and the energy's R-hat of k = 20 and k = 200 Langevin steps from the replay buffer."""

import math
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "examples", "convergence_cd_negatives.py")
LINE = re.compile(r"k = +(\d+) Langevin steps.*max split R-hat = ([0-9.naninf]+), min ESS = ([0-9naninf]+) of (\d+) counted states, "
                  r"energy R-hat = ([0-9.naninf]+)")


def test_the_example_answers_its_question_on_the_cpu():
    env = dict(os.environ, TORCHEBM_SMOKE="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, SCRIPT], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [LINE.search(line) for line in out.stdout.splitlines() if line.startswith("k = ")]
    assert len(rows) == 2 and all(rows), out.stdout
    assert [int(m.group(1)) for m in rows] == [20, 200]
    assert [int(m.group(4)) for m in rows] == [2 * 64 * 10, 2 * 64 * 100]  # 64 chains at the reduced size, both halves counted
    for m in rows:
        rhat, ess, e_rhat = float(m.group(2)), float(m.group(3)), float(m.group(5))
        assert math.isfinite(rhat) and rhat > 0.9 and math.isfinite(e_rhat) and e_rhat > 0.9
        assert 1.0 <= ess <= int(m.group(4))
    assert "device=cpu" in out.stdout and "route eager" in out.stdout
