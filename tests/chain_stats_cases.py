"""Shapes, data, float64 references and derived bars for the column statistics ebm_chain_stats_f32 (csrc/misc.hip:
chain_stats_kernel, chain_stats_wide_kernel).  Shared by tests/test_chain_stats_bars.py (CPU: the bars are derived here and
checked against an fp32 emulation of the kernels' arithmetic) and tests/test_chain_stats_gpu.py (the kernels held to them).

The reference is ``x.double().mean(0)`` and the biased ``x.double().var(0, unbiased=False)`` clamped to [1e-10, 1e10].

Derivation.  Per column write s = x[0] (the kernels' shift), d_r = x_r - s, A = mean(d), m2 = mean(d^2), so that
mean = s + A and var = m2 - A^2, with |A| <= mean|d| and A^2 <= mean|d|^2 <= m2.  U = 2^-24, U64 = 2^-53,
gamma_k(u) = k u / (1 - k u) the bound of k chained roundings.

Generic kernel (float64 throughout).  d_r is one float64 rounding of the difference of two fp32 values, the n of them are
added in float64 in some order (lanes, LDS partials, atomics) and divided by n:  |dA| <= gamma64(n + 2) mean|d|.  The squares
take one rounding more:  |d m2| <= gamma64(n + 2) m2.  mean = fl64(s + A^) rounded once to fp32:
    |d mean| <= U |mean| + (1 + 2 U) (gamma64(n + 2) mean|d| + U64 |mean|).
var = fl64((S2 - S1^2 / n) / n): the square of S1 carries 2 |A| |dA| + dA^2 <= 2 gamma64(n + 2) m2 (1 + ...), the product,
the two divisions and the subtraction four roundings of quantities bounded by m2:
    |d var64| <= gamma64(3 n + 10) m2,         |d var| <= U var_ref + (1 + 2 U) gamma64(3 n + 10) m2
after the rounding to fp32 and the clamp (a clamp moves two numbers no further apart; the fp32 constant 1e-10f is within
U 1e-10 of the reference's 1e-10, and var_ref >= 1e-10).

Wide kernel (dim a power of two in [4, 1024], n dim >= 1024).  d^ = fl32(x - s) is one fp32 rounding.  The unrolled loop adds
four of them in fp32 starting from zero -- three roundings -- so every term carries at most four fp32 roundings before it
enters a float64 accumulator (the tail loop: one):   |dA| <= (gamma32(4) + gamma64(n + 2)) mean|d|.
The squares: d^ d^ carries two roundings of d, the FMA chain t2 = fma(d^, d^, t2) at most four more (the first term is rounded
by its own FMA and by the three after it):   |d m2| <= (gamma32(6) + gamma64(n + 2)) m2.  Then, as above,
    |d mean| <= U |mean| + (1 + 2 U) ((gamma32(4) + gamma64(n + 2)) mean|d| + U64 |mean|)        [first order: U |mean| + 4 U mean|d|]
    |d var|  <= U var_ref + (1 + 2 U) (gamma32(6) + 2 gamma32(4) + gamma32(4)^2 + gamma64(3 n + 10)) m2     [U var + 14 U m2]
The accuracy of the wide kernel is therefore relative to the spread of the column ABOUT ROW 0 (m2), not to its variance:
a first row far from the others costs accuracy (the outlier data below measures it).

The float64 reference has an error of its own (torch's sums in double); REF_* below add its bound to both bars so that a
kernel result exactly at the rounding bound cannot trip over the reference.
"""

import zlib

import torch

U = 2.0 ** -24
U64 = 2.0 ** -53
VAR_MIN, VAR_MAX = 1e-10, 1e10

N = 301
# ---- shapes (n, dim) ------------------------------------------------------------------------------------------------
GENERIC_SHAPES = (
    [(N, d) for d in (1, 3, 63, 65, 100, 129, 1000, 1025, 5000)]
    + [(N, 2), (N, 96), (N, 2048)]            # not a power of two in [4, 1024]
    + [(255, 4), (15, 64), (1, 512)]           # just under n dim >= 1024
    + [(n, 100) for n in (1, 2, 255, 257, 1000)]
)
GENERIC_LARGE = (300_000, 100)  # past the row-block cap: two column tiles, so gy is capped at 1024 < ceil(n / 256) = 1172

WIDE_SHAPES = (
    [(N, 1 << p) for p in range(2, 11)]                    # every power of two 4 .. 1024
    + [(256, 4), (16, 64), (2, 512), (1, 1024)]            # n dim = 1024 exactly: one block, the tail loop only
    + [(4352, 4), (272, 64), (17, 1024)]                   # n dim / 4 = 4096 + 256: two blocks, both loops
    + [(4096, 4), (256, 64), (16, 1024)]                   # n dim / 4 = 4096 = 4 * 4 * stride: no tail
)
WIDE_LARGE = (1 << 20, 64)  # past the 2048-block cap: ceil(2^24 / 4096) = 4096 blocks asked for

DATA = ("normal", "mean1e4", "constant", "outlier")


def is_wide(n, dim):
    """the dispatch predicate of launch_chain_stats"""
    return 4 <= dim <= 1024 and (dim & (dim - 1)) == 0 and n * dim >= 1024


def wide_grid(n, dim):
    """(blocks, stride in float4 groups) of the wide launch: >= 16 float4 per lane, at most 2048 blocks of 256 lanes"""
    groups = n * dim // 4
    blocks = min(max(-(-groups // (256 * 16)), 1), 256 * 8)
    return blocks, blocks * 256


def generic_grid(n, dim):
    gx = -(-dim // 64)
    gy = min(max(-(-n // 256), 1), -(-(256 * 8) // gx))
    return gx, gy


def data(kind, n, dim, device=None, salt=0):
    """fp32 [n, dim]; seeded per (kind, shape).  `device`: draw there (the two large cases)."""
    seed = zlib.crc32(f"stats/{kind}/{n}/{dim}/{salt}".encode())
    if device is not None:
        g = torch.Generator(device=device).manual_seed(seed)
        z = torch.randn(n, dim, generator=g, device=device)
    else:
        z = torch.randn(n, dim, generator=torch.Generator().manual_seed(seed))
    if kind == "normal":
        return z
    if kind == "mean1e4":  # the cancellation case the shift exists for
        return z + 1e4
    if kind == "constant":
        return torch.ones_like(z) * (z[0:1] * 3.0 + 0.5)
    if kind == "outlier":  # row 0, the shift, 1e3 away from all the other rows
        z[0] += 1e3
        return z
    raise ValueError(kind)


# ---- float64 reference and bars ---------------------------------------------------------------------------------------
def gamma32(k):
    return k * U / (1.0 - k * U)


def gamma64(k):
    return k * U64 / (1.0 - k * U64)


def reference(x):
    """float64 (mean, var clamped, mean|d|, m2, REF_mean, REF_var) of an fp32 [n, dim] input, on x's device."""
    x64 = x.double()
    n = x.shape[0]
    mean = x64.mean(0)
    var_raw = x64.var(0, unbiased=False)
    d = x64 - x64[0:1]
    ref_mean = gamma64(n + 2) * x64.abs().mean(0)
    ref_var = gamma64(n + 8) * var_raw + ref_mean.square()
    return mean, var_raw.clamp(VAR_MIN, VAR_MAX), d.abs().mean(0), d.square().mean(0), ref_mean, ref_var


def bars(x, wide):
    """(mean64, var64, mean bar, var bar) per column."""
    mean, var, mad, m2, ref_mean, ref_var = reference(x)
    n = x.shape[0]
    g1 = gamma64(n + 2) + (gamma32(4) if wide else 0.0)
    g2 = gamma64(3 * n + 10) + ((gamma32(6) + 2 * gamma32(4) + gamma32(4) ** 2) if wide else 0.0)
    mean_bar = U * mean.abs() + (1 + 2 * U) * (g1 * mad + U64 * mean.abs()) + ref_mean
    var_bar = U * var + (1 + 2 * U) * g2 * m2 + ref_var
    return mean, var, mean_bar, var_bar


def check(got_mean, got_var, x, wide, what=""):
    """assert both bars; returns the worst error / bar ratios and the worst |d var| / var (printed by the callers)"""
    mean, var, mean_bar, var_bar = bars(x, wide)
    em = (got_mean.double().to(mean.device) - mean).abs()
    ev = (got_var.double().to(var.device) - var).abs()
    rm = (em / mean_bar.clamp(min=1e-300)).max().item()
    rv = (ev / var_bar).max().item()
    rel = (ev / var).max().item()
    assert bool((em <= mean_bar).all()), (what, "mean", rm)
    assert bool((ev <= var_bar).all()), (what, "var", rv)
    return rm, rv, rel
