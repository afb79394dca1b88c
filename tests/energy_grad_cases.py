"""Inputs, float64 references, natural scales, bars and mutants for the stand-alone evaluator ebm_energy_grad_f32 on the four
original energy kinds: double well, harmonic, dense Gaussian, isotropic mixture (csrc/rows_langevin.hip energy_grad_kernel and
energy_grad_wide_row_kernel, csrc/gauss_big.hip for Gaussians at 132 .. 512 dims in steps of 4).  Shared by
tests/test_energy_grad_bars.py (CPU: the fp32 oracle meets every bar, every mutant misses it) and tests/test_energy_grad_gpu.py
(the kernels held to the same bars).  The three landscape energies have the same pair in tests/landscape_cases.py.

Float64 is the referee: closed forms for the element-wise kinds, chain_cases.gauss_grad64 / energy64 / gmm_grad64 /
gmm_energy64 on the fp32 parameters the kernel is handed, upcast exactly (.double(), as helpers.to64 does).  The yardstick is the fp32 oracle on the CPU
(oracle.DoubleWell / Harmonic / Gaussian / GaussianMixture: forward in fp32, gradient by autograd).  Errors are in units of
U * N with U = 2^-24 and N the natural scale of the quantity:
  element-wise   energy: the sum of absolute terms, h sum (x^2 + b^2)^2 and k/2 sum x^2 (the gradient is held bit for bit)
  Gaussian       gradient per element sum_j |P_ij| |d_j|, energy 1/2 |d|^T |P| |d|          (chain_cases.gauss_grad64, energy64)
  mixture        gradient per row chain_cases.gmm_natural, energy chain_cases.gmm_energy_scale (the expansion scale)
"""

import functools
import math
import zlib
from dataclasses import dataclass
from typing import Any, Optional

import torch

import chain_cases as cc
import descent_cases as dc
import landscape_cases as lc
import oracle

U = cc.U
N = dc.N                # 301 chains
SCALES = lc.SCALES      # (0.5, 5.0)
H, B, K_HARM = 2.0, 1.0, 1.5   # double well (h, b), harmonic k: fp32-exact, as tests/descent_cases.py
# Mixtures have the same geometry at every width from 8 up: per coordinate the means are 1 + N(0, 1), and everything is divided by
# sqrt(dim / 8), so |mu_k|^2 ~ 16 (5 sigma from the origin) and |mu_k - mu_j|^2 ~ 16 (5 sigma apart) whatever the width.  The
# expansion scale (|x|^2 + |mu|^2) / (2 sigma^2) of chain_cases.gmm_natural then stays near 20 and a rounding of one coordinate of
# x is as visible at 1024 dims as at 4 (with means of fixed size per coordinate the scale grows with dim and hides it).
GMM_OFFSET = 1.0
GMM_SPREAD = 1.0 / 1.5  # chain_cases.gmm_params draws the means with standard deviation 1.5


def gmm_shrink(dim):
    return math.sqrt(max(dim, 8) / 8.0)


GAUSS_DECADES = 2.0     # the coordinates' scales span two decades, the precision matrix's entries four

ELEMENTWISE = ("double_well", "harmonic")
GMM_KS = (1, 3, 8, 9, 10, 11, 16, 40)
UNIFORM_K = 8           # the one mixture that also runs with uniform weights
# (kind, components, uniform weights)
# (the small grids of 9 .. 11 components come first among the mixtures: the first launch of each of a kind's seventeen kernel
#  variants loads its code object, and no one parametrised case should pay for all of them)
KINDS = tuple((k, 0, False) for k in ("double_well", "harmonic", "gauss")) + \
    tuple(("gmm", K, False) for K in sorted(GMM_KS, key=lambda K: (K not in (9, 10, 11), K))) + (("gmm", UNIFORM_K, True),)

WIDE_WIDTHS = (1025, 1500, 5000)   # energy_grad_wide_row_kernel: one wave per chain, lanes stride over the row
K40_WIDTHS = (12, 100, 356, 357)   # a 40-component mixture's means leave LDS at 357 dims (plan_floats below)
GAUSS_EXTRA = (132,)               # the first width of the tiled kernel
STRUCT_WIDTHS = dc.STRUCT_WIDTHS
WIDE_STRUCT = 1025

FAMILY = {"rows": "energy_grad_kernel", "wide": "energy_grad_wide_row_kernel", "tiled": "gauss_big_langevin_kernel"}


def kind_id(kind, K=0, uniform=False):
    return kind + (str(K) if K else "") + ("u" if uniform else "")


def widths(kind, K=0):
    if kind in ELEMENTWISE:
        return dc.WIDTHS + WIDE_WIDTHS
    if kind == "gauss":
        return tuple(sorted(dc.WIDTHS + GAUSS_EXTRA))
    if K == 40:
        return K40_WIDTHS
    if K in (9, 10, 11):
        return STRUCT_WIDTHS
    return dc.WIDTHS


def struct_widths(kind, K=0):
    if kind in ELEMENTWISE:
        return STRUCT_WIDTHS + (WIDE_STRUCT,)
    return K40_WIDTHS if K == 40 else STRUCT_WIDTHS


def route(kind, dim):
    """the kernel family ebm_energy_grad_f32 sends (kind, dim) to (csrc/api.hip, csrc/rows_langevin.hip launch_energy_grad)"""
    if kind == "gauss" and 128 < dim <= 512 and dim % 4 == 0:
        return "tiled"
    if dim > 1024:
        assert kind in ELEMENTWISE, (kind, dim)
        return "wide"
    return "rows"


def geometry(dim):
    """(G, NV) of rows.h pick_geometry"""
    nvec = (dim + 3) // 4
    if nvec <= 64:
        g = 1
        while g < nvec:
            g <<= 1
        return g, 1
    return (64, 2) if nvec <= 128 else (64, 4)


def chains_per_block(kind, dim):
    """256 threads: 256 / G chains of a lane-group block, four waves = four chains of the wide-row kernel"""
    return 4 if dim > 1024 else 256 // geometry(dim)[0]


def n_edges(kind, dim):
    c = chains_per_block(kind, dim)
    return tuple(sorted({1, max(1, c - 1), c, c + 1}))


LDS_BUDGET_FLOATS = 56 * 1024 // 4   # rows.h kParamLdsBudget


def plan_floats(kind, dim, K=0):
    """floats of shared parameters rows.h plan_params stages into LDS (they stay in global memory above the budget)"""
    pad = (dim + 3) & ~3
    if kind == "gauss":
        return dim * pad
    kp = 8 if K < 8 else (K + 7) & ~7
    return kp * pad + ((kp + 3) & ~3)


def padded_components(K):
    return 8 if K < 8 else (K + 7) & ~7


# ----------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------
@dataclass
class Setup:
    kind: str
    dim: int
    K: int
    uniform: bool
    scale: float
    x: torch.Tensor            # fp32 [n, dim]
    fp: Any = None             # (mean, sym P) / (means, sigma, logw): the fp32 parameters the kernel is handed
    weights: Optional[torch.Tensor] = None
    case: Optional[cc.Case] = None
    route: str = "rows"

    @property
    def id(self):
        return f"{kind_id(self.kind, self.K, self.uniform)}-d{self.dim}-s{self.scale}"


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(k) for k in ("energy_grad",) + key).encode()))


@functools.lru_cache(maxsize=None)
def params(kind, dim, K=0, uniform=False):
    """(fp, weights, case, Cholesky factor of the covariance) -- made once per (kind, dim, K): the Gaussian's inverse is the expensive part"""
    if kind == "gauss":
        import torchebm_amd as ta

        case = cc.Case("langevin", "gauss", dim, n=N)
        mean, cov = cc.gauss_params(case, GAUSS_DECADES)
        model = ta.GaussianModel(mean, cov)
        return (model.mean.detach().clone(), cc.sym_precision(model.cov_inv.detach())), None, case, torch.linalg.cholesky(cov.double())
    if kind == "gmm":
        case = cc.Case("langevin", "gmm", dim, K=K, n=N)
        means, sigma, weights = cc.gmm_params(case)
        means = ((means * GMM_SPREAD + GMM_OFFSET) / gmm_shrink(dim)).float().contiguous()
        if uniform:
            weights = torch.ones(K)
        return (means, sigma, cc.gmm_log_weights(weights)), weights, case, None
    return None, None, None, None


def mixture_rows(fp, scale, n, g):
    """a third of the rows near the midpoint of two components (the weights decide the responsibilities there), a third part of
    the way from the origin to a component (a spurious component at the origin would carry weight there), the rest around a
    component, 0.03 sigma to 2 sigma times `scale` away per coordinate (shrunk with the means from 8 dims up)."""
    means, sigma, _ = fp
    K, dim = means.shape
    r = gmm_shrink(dim)
    pick = torch.randint(0, K, (n,), generator=g)
    spread = 10.0 ** (torch.rand(n, 1, generator=g) * 1.8 - 1.5)
    x = means[pick] + torch.randn(n, dim, generator=g) * (sigma * scale / r) * spread
    a, b = n // 3, 2 * (n // 3)
    x[:a] = 0.5 * (means[pick[:a]] + means[(pick[:a] + 1) % K]) + (0.05 / r) * torch.randn(a, dim, generator=g)
    t = 0.35 + 0.3 * torch.rand(b - a, 1, generator=g)
    x[a:b] = t * means[pick[a:b]] + (0.05 / r) * torch.randn(b - a, dim, generator=g)
    return x.float().contiguous()


def setup(kind, dim, K=0, uniform=False, scale=SCALES[0], n=N) -> Setup:
    g = _gen(kind, dim, K, uniform, scale, n)
    fp, weights, case, chol = params(kind, dim, K, uniform)
    if kind in ELEMENTWISE:
        x = ((torch.rand(n, dim, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()
    elif kind == "gauss":
        x = (fp[0].double() + scale * torch.randn(n, dim, generator=g, dtype=torch.float64) @ chol.t()).float()
    else:
        x = mixture_rows(fp, scale, n, g)
    return Setup(kind, dim, K, uniform, scale, x, fp, weights, case, route(kind, dim))


def all_cases(kind, K=0, uniform=False):
    return [(dim, scale) for dim in widths(kind, K) for scale in SCALES]


# ----------------------------------------------------------------------------------------------------------------
# float64 references and natural scales
# ----------------------------------------------------------------------------------------------------------------
def reference(s: Setup, x=None, fp=None):
    """(e64 [n], g64 [n, dim], N_E [n], N_g [n, dim] or [n, 1]) of the fp32 states x under the fp32 parameters fp"""
    x = s.x if x is None else x
    fp = s.fp if fp is None else fp
    xd = x.double()
    if s.kind == "double_well":
        u = xd * xd - B * B
        return H * (u * u).sum(1), 4.0 * H * u * xd, H * (xd * xd + B * B).square().sum(1), None
    if s.kind == "harmonic":
        e = 0.5 * K_HARM * (xd * xd).sum(1)
        return e, K_HARM * xd, e, None
    if s.kind == "gauss":
        g, ng = cc.gauss_grad64(x, fp[0], fp[1])
        e, ne = cc.energy64(s.case, x, fp)
        return e, g, ne, ng
    means, sigma, logw = fp
    return (cc.gmm_energy64(x, means, sigma, logw), cc.gmm_grad64(x, means, sigma, logw), cc.gmm_energy_scale(x, means, sigma),
            cc.gmm_natural(x, means, sigma)[:, None])


def errors(ref, e_got, g_got):
    """worst energy and gradient error against the float64 reference, in units of U * N (gradient: None where there is no scale)"""
    e64, g64, ne, ng = ref
    ee = ((e_got.double().cpu() - e64).abs() / (U * ne)).max().item()
    if ng is None:
        return ee, None
    return ee, ((g_got.double().cpu() - g64).abs() / (U * ng)).max().item()


def oracle32(s: Setup):
    if s.kind == "double_well":
        return oracle.DoubleWell(H, B)
    if s.kind == "harmonic":
        return oracle.Harmonic(K_HARM)
    return cc._oracle32(s.case, s.fp)


def cpu32(s: Setup, x=None):
    """the yardstick: the fp32 oracle's energy and gradient on the CPU"""
    x = s.x if x is None else x
    en = oracle32(s)
    return en.energy(x), en.grad(x)


def package_model(s: Setup, device=None):
    import torchebm_amd as ta

    if s.kind == "double_well":
        return ta.DoubleWellModel(barrier_height=H, b=B, device=device)
    if s.kind == "harmonic":
        return ta.HarmonicModel(k=K_HARM, device=device)
    if s.kind == "gauss":
        return ta.GaussianModel(*cc.gauss_params(s.case, GAUSS_DECADES), device=device)
    return ta.GaussianMixtureModel(s.fp[0], sigma=s.fp[1], weights=s.weights, device=device)


# ----------------------------------------------------------------------------------------------------------------
# mutants: evaluations that are wrong in a way a kernel could be.  Each returns (e, g) in float64, or None where it does not
# apply; tests/test_energy_grad_bars.py checks that each misses the bar in EVERY case it applies to.
# ----------------------------------------------------------------------------------------------------------------
def round16(x):
    """x rounded to 16 significant bits (landscape_cases.degraded_grad)"""
    mant, expo = torch.frexp(x.double())
    return torch.ldexp((mant * 65536).round() / 65536, expo).float()


def mutant_inputs16(s: Setup):
    """judged by the gradient alone, as landscape_cases.degraded_grad is: in an energy the roundings of a row's coordinates average
    out with its width.  The element-wise gradients are held bit for bit, which no bar has to defend."""
    if s.kind in ELEMENTWISE:
        return None
    e, g, _, _ = reference(s, x=round16(s.x))
    return e, g


def mutant_uniform_weights(s: Setup):
    if s.kind != "gmm" or s.K == 1 or s.uniform:
        return None
    means, sigma, _ = s.fp
    e, g, _, _ = reference(s, fp=(means, sigma, cc.gmm_log_weights(torch.ones(s.K))))
    return e, g


def mutant_padding(s: Setup):
    """the mixture staged to eight or sixteen components, its padding at the origin with log-weight 0 instead of -inf"""
    if s.kind != "gmm" or padded_components(s.K) == s.K:
        return None
    means, sigma, logw = s.fp
    pad = padded_components(s.K) - s.K
    e, g, _, _ = reference(s, fp=(torch.cat([means, means.new_zeros(pad, s.dim)]), sigma, torch.cat([logw, logw.new_zeros(pad)])))
    return e, g


def mutant_dropped_column(s: Setup):
    """the Gaussian at a ragged width with the last column of Ps left out of every row's sum"""
    if s.kind != "gauss" or s.dim % 4 == 0 or s.dim < 2:
        return None
    mean, ps = s.fp
    d = s.x.double() - mean.double()
    p = ps.double().clone()
    p[:, -1] = 0.0
    g = d @ p.t()
    return 0.5 * (d * g).sum(1), g


# name -> (evaluation, the quantities whose bar it must miss)
MUTANTS = {"inputs16": (mutant_inputs16, ("grad",)), "uniform_weights": (mutant_uniform_weights, ("energy", "grad")),
           "padding": (mutant_padding, ("energy", "grad")), "dropped_column": (mutant_dropped_column, ("energy", "grad"))}


# ----------------------------------------------------------------------------------------------------------------
# Bars.  CPU_WORST is the worst error the fp32 oracle reaches on the CPU over every (width, scale) of the kind, measured with
# tests/test_energy_grad_bars.py's own loop (torch 2 CPU kernels; that test allows another host's torch 1.5 x).  The bar is
# twice that, the margin landscape_cases.BAR takes: the kernel adds a row in another order than torch and may use another,
# equally valid, exp / log.  The element-wise gradients have no bar: they are bit for bit the fp32 oracle's.  The comments give
# each mutant's LOWEST ratio to the bar of the quantity it is caught by, over the cases it applies to (energy / gradient).
# ----------------------------------------------------------------------------------------------------------------
CPU_WORST = {
    "double_well": {"energy": 2.533},
    "harmonic": {"energy": 3.557},
    "gauss": {"energy": 3.386, "grad": 7.414},   # inputs16: - / 5.4;  dropped_column: 1739 / 240761
    "gmm1": {"energy": 3.400, "grad": 1.664},    # inputs16: - / 46.1;  padding: 925461 / 483199
    "gmm3": {"energy": 2.931, "grad": 0.838},    # inputs16: - / 4.3;  uniform_weights: 20943 / 42564;  padding: 777203 / 367226
    "gmm8": {"energy": 2.499, "grad": 0.776},    # inputs16: - / 3.7;  uniform_weights: 43885 / 42350
    "gmm9": {"energy": 3.116, "grad": 0.787},    # inputs16: - / 3.5;  uniform_weights: 81711 / 76071;  padding: 632233 / 264442
    "gmm10": {"energy": 2.426, "grad": 0.693},   # inputs16: - / 4.5;  uniform_weights: 104157 / 64228;  padding: 996641 / 439649
    "gmm11": {"energy": 2.721, "grad": 0.831},   # inputs16: - / 3.7;  uniform_weights: 90969 / 39083;  padding: 991166 / 352763
    "gmm16": {"energy": 3.177, "grad": 0.824},   # inputs16: - / 2.6;  uniform_weights: 60283 / 45581
    "gmm40": {"energy": 2.662, "grad": 0.781},   # inputs16: - / 3.7;  uniform_weights: 93712 / 59458
    "gmm8u": {"energy": 2.653, "grad": 0.747},   # inputs16: - / 4.3
}
BAR = {name: {q: 2.0 * w for q, w in d.items()} for name, d in CPU_WORST.items()}


def bar(s_or_kind, K=0, uniform=False):
    if isinstance(s_or_kind, Setup):
        s_or_kind, K, uniform = s_or_kind.kind, s_or_kind.K, s_or_kind.uniform
    return BAR[kind_id(s_or_kind, K, uniform)]


def mean_energy_bar(s: Setup, x):
    """(float64 mean energy of the states x, the bar on a sampler's diag["energy"] entry for them): every chain's energy within
    the energy bar of its own natural scale, and one fp32 rounding of the mean"""
    e64, _, ne, _ = reference(s, x=x)
    return e64.mean().item(), (bar(s)["energy"] + 1.0) * U * ne.mean().item()
