"""The lean DoubleWell loop (bench.py's kernel) draws its Philox at 32-bit counter words: per step 16 v_mad_u64_u32 (rounds
3-10; the step's multiplies of rounds 1-2 run on the scalar unit), no vector 32-bit multiply, 16 v_bitop3 + 2 v_xor, two
steps per loop trip, no scratch.  The 64-bit fallback keeps the 18 multiplies and 20 three-input XORs it had.  Compiles
langevin.hip to gfx950 assembly (hipcc cross-compiles without a GPU).  A failure here is a performance regression, not a
wrong result."""

import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNEL32 = "langevin_chain_lean_kernelILi0ELb0ELb0ELb0ELb0ELb0EE"  # <DoubleWell, no table / clamp / traj / Heun, 32-bit counters>
KERNEL64 = "langevin_chain_lean_kernelILi0ELb0ELb0ELb0ELb0ELb1EE"


def _kernel(src, key):
    start = next(i for i, l in enumerate(src) if l.startswith("_Z") and key in l.split(":")[0])
    end = next(i for i in range(start, len(src)) if src[i].startswith(".Lfunc_end"))
    meta = "\n".join(src[end:end + 60])
    return src[start:end], int(re.search(r"; ScratchSize: (\d+)", meta).group(1))


def _hot_loop(body):
    """Opcode counts of the biggest backward-branch loop (scripts/isa_mix.py --loop)."""
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    best = (0, 0, 0)
    for i, l in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > best[0]:
            best = (i - labels[m.group(1)], labels[m.group(1)], i)
    return collections.Counter(l.split()[0] for l in body[best[1]:best[2]] if l.startswith("\t") and not l.strip().startswith(";"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_lean_loop_philox_at_32_bit_counters(tmp_path):
    out = tmp_path / "langevin.s"
    subprocess.run([os.path.join(ROOT, "scripts", "asm_unit.sh"), "langevin.hip", str(out)], check=True, capture_output=True, timeout=600)
    src = out.read_text().split("\n")

    body, scratch = _kernel(src, KERNEL32)
    ops = _hot_loop(body)
    trans = sum(ops[o] for o in ("v_log_f32_e32", "v_sin_f32_e32", "v_cos_f32_e32", "v_sqrt_f32_e32"))
    steps = trans // 8  # 8 transcendentals per float4 group and step (two Box-Muller pairs)
    assert steps == 2, ops                                         # `#pragma unroll 2` survived
    assert ops["v_mad_u64_u32"] == 16 * steps, ops
    assert ops["v_mul_lo_u32"] == 0 and ops["v_mul_hi_u32"] == 0, ops
    assert ops["v_bitop3_b32"] + ops["v_xor_b32_e32"] + ops["v_xor_b32_e64"] <= 18 * steps, ops
    assert sum(n for o, n in ops.items() if o.startswith("v_")) == 72 * steps, ops
    assert scratch == 0

    body, scratch = _kernel(src, KERNEL64)
    ops = _hot_loop(body)
    assert ops["v_mad_u64_u32"] == 36 and ops["v_bitop3_b32"] == 40 and scratch == 0, ops
