"""The plain-f32 folded DoubleWell loop (langevin_elem.h PLAIN, kind 17, langevin_fold.hip: the kernel of bench.py's headline
call): the folded loop of tests/test_isa_lean_fold.py with gradient, drift and noise update one element per instruction.  On
this loop a packed-f32 instruction costs more issue time than the two plain ones it replaces (docs/design/langevin_flat.md),
so the loop must hold NO v_pk_* at all: 88 vector instructions per float4 group and step where kind 16 issues 70 (its 18
packed ones as 36 plain), two steps per loop trip, the Philox of kind 16 (16 v_mad_u64_u32, 16 v_bitop3_b32 + 2 v_xor_b32 per
step).  The literal redo loop runs one step per trip.  No scratch, at most 64 VGPRs (8 waves per SIMD).  Compiles
langevin_fold.hip with the Makefile's flag for that unit (-fno-slp-vectorize: without it the SLP vectoriser packs the loop
again) and langevin.hip, for kind 16, without.  hipcc cross-compiles without a GPU.  A failure here is a performance regression,
not a wrong result."""

import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KIND_FOLD = 16    # langevin_elem.h kDoubleWellFold
KIND_PLAIN = 17   # langevin_elem.h kDoubleWellFoldPlain
TRANS = ("v_log_f32_e32", "v_sin_f32_e32", "v_cos_f32_e32", "v_sqrt_f32_e32")


def _symbol(kind, c64):
    return f"langevin_chain_lean_kernelILi{kind}ELb0ELb0ELb0ELb0ELb{int(c64)}EE"


def _asm(tmp_path_factory, unit, *flags):
    out = tmp_path_factory.mktemp("isa") / (unit + ".s")
    subprocess.run([os.path.join(ROOT, "scripts", "asm_unit.sh"), unit, str(out), *flags], check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    return _asm(tmp_path_factory, "langevin_fold.hip", "-fno-slp-vectorize")  # torchebm_amd/csrc/Makefile: langevin_fold.o


@pytest.fixture(scope="module")
def listing_kind16(tmp_path_factory):
    return _asm(tmp_path_factory, "langevin.hip")


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


def _fold_and_redo(listing, kind, c64):
    body, scratch, vgprs = _kernel(listing, _symbol(kind, c64))
    loops = _loops(body)
    assert len(loops) == 2, [dict(l) for l in loops]
    steps = [sum(ops[o] for o in TRANS) // 8 for ops in loops]  # 8 transcendentals per float4 group and step
    assert sorted(steps) == [1, 2], steps                       # the folded loop two steps per trip, the redo one
    return loops[steps.index(2)], loops[steps.index(1)], scratch, vgprs


def _packed(ops):
    return sum(n for o, n in ops.items() if o.startswith("v_pk_"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_plain_loop_mix_at_32_bit_counters(listing):
    fold, redo, scratch, vgprs = _fold_and_redo(listing, KIND_PLAIN, False)
    assert _packed(fold) == 0, fold
    assert _valu(fold) == 2 * 88, fold
    assert fold["v_mad_u64_u32"] == 2 * 16, fold
    assert fold["v_bitop3_b32"] == 2 * 16 and fold["v_xor_b32_e32"] + fold["v_xor_b32_e64"] == 2 * 2, fold
    assert fold["v_cvt_f32_u32_e32"] + fold["v_cvt_f32_u32_e64"] == 2 * 4, fold
    assert fold["v_mul_lo_u32"] == 0 and fold["v_mul_hi_u32"] == 0, fold
    assert scratch == 0
    assert vgprs <= 64, vgprs


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_plain_loop_is_kind_16s_loop_unpacked_at_64_bit_counters(listing, listing_kind16):
    plain, _, scratch, vgprs = _fold_and_redo(listing, KIND_PLAIN, True)
    fold, _, _, _ = _fold_and_redo(listing_kind16, KIND_FOLD, True)
    assert _packed(plain) == 0, plain
    assert _valu(plain) - _valu(fold) == _packed(fold) == 2 * 18, (plain, fold)  # every packed instruction as two plain ones
    assert plain["v_mad_u64_u32"] == fold["v_mad_u64_u32"] == 2 * 18, (plain, fold)
    assert scratch == 0
    assert vgprs <= 64, vgprs
