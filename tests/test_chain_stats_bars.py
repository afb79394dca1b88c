"""The bars of tests/test_chain_stats_gpu.py, on the CPU (derivation: tests/chain_stats_cases.py).  The arithmetic of both
column-statistics kernels is emulated in torch -- the generic kernel's float64 shifted sums; the wide kernel's fp32
subtraction, its four-row fp32 groups strided as the kernel strides, then float64 -- and must stay inside the derived bars on
every shape and data set the GPU test uses.  The same emulation with the float64 accumulators replaced by fp32 must not:
a bar that lets an fp32 accumulation through would not notice the kernel losing its float64 sums."""

import pytest
import torch

import chain_stats_cases as sc

torch.set_num_threads(1)


def _finish(s, t1, t2, n, acc):
    """the last block's lines: mean = s + S1 / n, var = (S2 - S1^2 / n) / n in the accumulator's type, rounded to fp32, clamped"""
    nn = torch.tensor(float(n), dtype=acc)
    mean = (s.to(acc) + t1 / nn).float()
    var = ((t2 - t1 * t1 / nn) / nn).float()
    return mean, var.clamp(torch.tensor(1e-10, dtype=torch.float32), torch.tensor(1e10, dtype=torch.float32))


def generic_emulation(x):
    d = x.double() - x[0:1].double()
    return _finish(x[0], d.sum(0), (d * d).sum(0), x.shape[0], torch.float64)


def _fma32(a, b, c):
    """fl32(a b + c): the product of two fp32 values is exact in float64, the sum is rounded there first (a double rounding
    that differs from the hardware FMA by at most 2^-29 of a unit in the last place: nothing to the bars)"""
    return (a.double() * b.double() + c.double()).float()


def wide_emulation(x, acc=torch.float64):
    """chain_stats_wide_kernel, lane by lane: lane l of the grid owns the float4 groups l, l + stride, ...; while four more of
    them exist it adds the four in fp32 (t1 by additions from zero, t2 by an FMA chain) and folds the two sums into its
    accumulators, the rest goes in one by one; lanes that share a column are then added in lane order (LDS and global atomics:
    some order), the last block finishes.  `acc`: the accumulators' type (the kernel: float64)."""
    n, dim = x.shape
    groups = n * dim // 4
    _, stride = sc.wide_grid(n, dim)
    d = (x - x[0:1]).reshape(groups, 4)  # fp32 subtraction of the shift
    J = -(-groups // stride)
    pad = J * stride - groups
    dj = torch.cat([d, torch.zeros(pad, 4)]).view(J, stride, 4)
    per_lane = torch.full((stride,), J)
    if pad:
        per_lane[stride - pad:] = J - 1
    s1, s2 = torch.zeros(stride, 4, dtype=acc), torch.zeros(stride, 4, dtype=acc)
    for q in range(0, J, 4):
        full = (q + 3) < per_lane
        if q + 3 < J:
            b = dj[q:q + 4]
            t1 = ((b[0] + b[1]) + b[2]) + b[3]
            t2 = torch.zeros(stride, 4)
            for j in range(4):
                t2 = _fma32(b[j], b[j], t2)
            s1 += torch.where(full[:, None], t1, torch.zeros(())).to(acc)
            s2 += torch.where(full[:, None], t2, torch.zeros(())).to(acc)
        for j in range(q, min(q + 4, J)):
            tail = (~full & (j < per_lane))[:, None]
            v = dj[j].to(acc)
            s1 += torch.where(tail, v, torch.zeros((), dtype=acc))
            s2 += torch.where(tail, v * v, torch.zeros((), dtype=acc))
    # lane l, element i is column (4 l + i) % dim: 4 stride is a multiple of 1024, so of dim
    # (added row by row: torch's own sum / cumsum of fp32 accumulate in double or pairwise, which an atomic does not)
    c1, c2 = torch.zeros(dim, dtype=acc), torch.zeros(dim, dtype=acc)
    for r1, r2 in zip(s1.view(-1, dim), s2.view(-1, dim)):
        c1 += r1
        c2 += r2
    return _finish(x[0], c1, c2, n, acc)


@pytest.mark.parametrize("kind", sc.DATA)
def test_generic_emulation_meets_the_bars(kind):
    for n, dim in sc.GENERIC_SHAPES:
        assert not sc.is_wide(n, dim)
        x = sc.data(kind, n, dim)
        mean, var = generic_emulation(x)
        rm, rv, rel = sc.check(mean, var, x, wide=False, what=(kind, n, dim))
        if kind == "constant" or n == 1:
            assert bool((var == torch.tensor(1e-10, dtype=torch.float32)).all()), (kind, n, dim)
    print(kind, "generic: last shape's error / bar: mean %.3f var %.3f, |dvar| / var %.2e" % (rm, rv, rel))


@pytest.mark.parametrize("kind", sc.DATA)
def test_wide_emulation_meets_the_bars(kind):
    worst = (0.0, 0.0, 0.0)
    for n, dim in sc.WIDE_SHAPES:
        assert sc.is_wide(n, dim)
        x = sc.data(kind, n, dim)
        mean, var = wide_emulation(x)
        r = sc.check(mean, var, x, wide=True, what=(kind, n, dim))
        worst = tuple(max(a, b) for a, b in zip(worst, r))
        if kind == "constant" or n == 1:
            assert bool((var == torch.tensor(1e-10, dtype=torch.float32)).all()), (kind, n, dim)
    print(kind, "wide: worst error / bar: mean %.3f var %.3f, worst |dvar| / var %.2e" % worst)


def test_wide_loops_are_the_ones_the_shapes_are_meant_for():
    """n dim = 1024: every lane holds one group (tail loop only); 4096 + 256 groups: lanes with nine and with eight groups
    (two unrolled rounds, then a tail for some); 4096 groups on one block: sixteen per lane, no tail."""
    for n, dim in ((256, 4), (16, 64), (2, 512), (1, 1024)):
        assert sc.wide_grid(n, dim) == (1, 256) and n * dim // 4 == 256
    for n, dim in ((4352, 4), (272, 64), (17, 1024)):
        blocks, stride = sc.wide_grid(n, dim)
        assert (blocks, stride) == (2, 512) and n * dim // 4 == 8 * stride + 256
    for n, dim in ((4096, 4), (256, 64), (16, 1024)):
        blocks, stride = sc.wide_grid(n, dim)
        assert blocks == 1 and (n * dim // 4) % (4 * stride) == 0
    assert sc.wide_grid(*sc.WIDE_LARGE)[0] == 2048 and -(-(sc.WIDE_LARGE[0] * sc.WIDE_LARGE[1] // 4) // 4096) > 2048
    gx, gy = sc.generic_grid(*sc.GENERIC_LARGE)
    assert gy == 1024 and -(-sc.GENERIC_LARGE[0] // 256) > gy
    # the predicate's edges
    assert not sc.is_wide(255, 4) and sc.is_wide(256, 4) and not sc.is_wide(15, 64) and sc.is_wide(16, 64)
    assert not sc.is_wide(10_000, 2) and not sc.is_wide(10_000, 2048) and not sc.is_wide(10_000, 96)


# N partial sums of a column added one after the other in fp32: every addition rounds the running sum, which grows like k S2 / N,
# so the error of S2 is about U S2 / N sqrt(sum k^2) / sqrt(3) = U S2 sqrt(N) / 3, and so is that of var relative to m2.  At
# 2^18 rows of width 4 the grid has N = 2^14 lanes per column: some 40 U m2 against a bar of 15 U m2 -- the shape of the negative
# control.  (At the few hundred rows of the other shapes an fp32 accumulation stays inside the bars: the float64 accumulators
# matter for long columns.)
DEGRADED_SHAPE = (1 << 18, 4)


@pytest.mark.parametrize("kind", ["normal", "mean1e4"])
def test_fp32_accumulators_fail_the_bars(kind):
    n, dim = DEGRADED_SHAPE
    x = sc.data(kind, n, dim)
    mean, var = wide_emulation(x)
    print(kind, "float64 accumulators: error / bar", sc.check(mean, var, x, wide=True)[:2])
    mean32, var32 = wide_emulation(x, acc=torch.float32)
    _, v64, _, var_bar = sc.bars(x, wide=True)
    ratio = ((var32.double() - v64).abs() / var_bar).max().item()
    print(kind, "fp32 accumulators: var error / bar %.1f" % ratio)
    assert ratio > 1.0, "an fp32 accumulation passes the wide kernel's bar"
