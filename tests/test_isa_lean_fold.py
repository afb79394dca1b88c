"""The folded DoubleWell loop (langevin_elem.h FOLD, the kernel of bench.py's headline call): the gradient's power-of-two
factor rides in the drift coefficient, so a step issues 70 vector instructions per float4 group where the literal loop issues
72 -- the same 16 v_mad_u64_u32 at 32-bit Philox counters, no vector 32-bit multiply, two steps per loop trip.  Of the
kernel's backward-branch loops exactly two draw normals: the folded step loop and the literal loop that redoes a lane which
failed the guard (one step per trip); the others are the partial last group's store blocks.  No scratch, at most 64 VGPRs
(8 waves per SIMD).  Compiles langevin.hip to gfx950 assembly (hipcc cross-compiles without a GPU).  A failure here is a
performance regression, not a wrong result."""

import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KIND_FOLD = 16  # langevin_elem.h kDoubleWellFold
FOLD32 = f"langevin_chain_lean_kernelILi{KIND_FOLD}ELb0ELb0ELb0ELb0ELb0EE"
FOLD64 = f"langevin_chain_lean_kernelILi{KIND_FOLD}ELb0ELb0ELb0ELb0ELb1EE"
TRANS = ("v_log_f32_e32", "v_sin_f32_e32", "v_cos_f32_e32", "v_sqrt_f32_e32")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "langevin.s"
    subprocess.run([os.path.join(ROOT, "scripts", "asm_unit.sh"), "langevin.hip", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


def _kernel(src, key):
    start = next(i for i, l in enumerate(src) if l.startswith("_Z") and key in l.split(":")[0])
    end = next(i for i in range(start, len(src)) if src[i].startswith(".Lfunc_end"))
    meta = "\n".join(src[end:end + 60])
    return (src[start:end], int(re.search(r"; ScratchSize: (\d+)", meta).group(1)),
            int(re.search(r"; NumVgprs: (\d+)", meta).group(1)))


def _loops(body):
    """Opcode counts of every backward-branch loop (branch to an earlier label) that draws Philox numbers, in listing order."""
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    out = []
    for i, l in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            ops = collections.Counter(x.split()[0] for x in body[labels[m.group(1)]:i]
                                      if x.startswith("\t") and not x.strip().startswith(";"))
            if ops["v_mad_u64_u32"]:
                out.append(ops)
    return out


def _valu(ops):
    return sum(n for o, n in ops.items() if o.startswith("v_"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("key,c64", [(FOLD32, False), (FOLD64, True)])
def test_folded_loop_mix(listing, key, c64):
    body, scratch, vgprs = _kernel(listing, key)
    loops = _loops(body)
    assert len(loops) == 2, [dict(l) for l in loops]
    steps = [sum(ops[o] for o in TRANS) // 8 for ops in loops]  # 8 transcendentals per float4 group and step
    assert sorted(steps) == [1, 2], steps                       # the folded loop two steps per trip, the redo one
    fold, redo = loops[steps.index(2)], loops[steps.index(1)]
    assert fold["v_mul_lo_u32"] == 0 and fold["v_mul_hi_u32"] == 0, fold
    # per step: 2 packed multiplies in Box-Muller, 5 + 3 per pair of elements (the literal step: 6 + 3)
    assert fold["v_pk_mul_f32"] == 2 * 12 and fold["v_pk_add_f32"] == 2 * 6, fold
    if not c64:
        assert fold["v_mad_u64_u32"] == 16 * 2, fold
        assert _valu(fold) == 70 * 2, fold
        assert _valu(redo) == 72, redo                          # the literal step, as in the literal kernel
    else:
        assert fold["v_mad_u64_u32"] == 2 * 18, fold
        assert _valu(redo) - _valu(fold) // 2 == 2, (fold, redo)  # the one packed multiply per pair the fold saves
    assert redo["v_pk_mul_f32"] == 14 and redo["v_pk_add_f32"] == 6, redo
    assert scratch == 0
    assert vgprs <= 64, vgprs
