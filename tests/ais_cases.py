"""Annealed importance sampling: an independent restatement of the algorithm (include/ebm_hip.h, ebm_ais_chain_f32) in torch
ops on the oracle energies -- the literal safe-mode leapfrog sequence of oracle/hmc.py on the path energy U_b -- the cases the
tests run, and their inputs.  Shared by test_ais.py (CPU tier) and test_ais_gpu.py; it never calls the package's class."""

import functools

import torch

from tempering_cases import energy_spec, model_of, oracle_of  # noqa: F401  (re-exported for the tests)
from tempering_cases import start_scale
from tempering_hmc_cases import MARGIN_BAR, STEP_C, leapfrog_steps  # noqa: F401


def f32(v):
    """A double rounded to fp32 once, as a Python float."""
    return float(torch.tensor(float(v), dtype=torch.float64).float())


def sigmoid_betas(T, sharpness=4.0):
    """beta[0 .. T], non-uniform: formed in double, rounded to fp32 once, the ends exactly 0 and 1."""
    t = torch.arange(T + 1, dtype=torch.float64) / T
    s = torch.sigmoid(sharpness * (2.0 * t - 1.0))
    b = ((s - s[0]) / (s[-1] - s[0])).float()
    b[0], b[-1] = 0.0, 1.0
    return b


def linear_betas(T):
    b = (torch.arange(T + 1, dtype=torch.float64) / T).float()
    b[0], b[-1] = 0.0, 1.0
    return b


def _hamiltonian(u, p):
    return u.clamp(min=-1e10, max=1e10) + (0.5 * torch.sum(p.square(), dim=-1)).clamp_(min=0.0, max=1e10)


def restate(energy, x0, z, u, betas, eps, n_leapfrog, base_std, dtype=torch.float32, force_betas=None):
    """x0 [n, dim], z [T, n, dim], u [T, n], betas fp32 [T + 1], eps: T step sizes -> final states [n, dim], logw [n], the accept
    mask [T, n] and the margins |u - a| (inf where the threshold is NaN).  The coefficients the contract forms in fp32 -- the
    difference of the betas, 1 - beta, inv_var0 -- are formed in fp32 here too and then used in `dtype`.  force_betas: another table for the force of the trajectory alone -- a
    deliberately wrong walk (tests/test_tempered_landscape_bars.py); None is the algorithm."""
    T = z.shape[0]
    fb = betas if force_betas is None else force_betas
    inv_var0 = f32(1.0 / float(base_std) ** 2)
    half_inv = 0.5 * inv_var0
    x = x0.to(dtype).clone()
    logw = torch.zeros(x.shape[0], dtype=dtype)
    comp = torch.zeros_like(logw)
    base = lambda y: half_inv * torch.sum(y.square(), dim=-1)  # noqa: E731
    accepted, margins = [], []
    for t in range(1, T + 1):
        b = float(betas[t])
        db = float(betas[t] - betas[t - 1])
        b0 = float(1.0 - betas[t])
        e0, e = base(x), energy.energy(x)
        y = db * (e0 - e) - comp  # the compensated (Kahan) pair
        s = logw + y
        comp = torch.where(torch.isfinite(s), (s - logw) - y, torch.zeros_like(s))
        logw = s
        bf = float(fb[t])
        c0 = float(1.0 - fb[t]) * inv_var0
        force = lambda q: (-(c0 * q + bf * energy.grad(q))).clamp_(min=-1e6, max=1e6)  # noqa: E731
        eps_t = torch.tensor(f32(eps[t - 1]), dtype=dtype)  # the fp32 table entry (oracle/hmc.py: eps as a tensor of the state's dtype)
        p = z[t - 1].to(dtype)
        h0 = _hamiltonian(b0 * e0 + b * e, p)
        xp = x
        for _ in range(n_leapfrog):  # oracle/hmc.py leapfrog(), safe mode, identity mass
            p_half = p + 0.5 * eps_t * force(xp)
            xp = xp + eps_t * p_half
            p = p_half + 0.5 * eps_t * force(xp)
            xp = xp.nan_to_num_(nan=0.0)
            p = p.nan_to_num_(nan=0.0)
        h1 = _hamiltonian(b0 * base(xp) + b * energy.energy(xp), p)
        a = torch.exp((h0 - h1).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
        ut = u[t - 1].to(dtype)
        acc = ut < a
        accepted.append(acc)
        margins.append(torch.where(a == a, (ut - a).abs().double(), torch.full((), float("inf"), dtype=torch.float64)))
        x = torch.where(acc[:, None], xp, x)
    return {"x": x, "logw": logw, "accepted": torch.stack(accepted), "margin": torch.stack(margins)}


# (kind, dim, n, T): the smallest shapes that reach every hazard of the kernel -- dim 2 one lane per chain and 257 chains several
# workgroups plus a tail, 5 unaligned rows, 32 full rows, 100 G = 32 masked, 256 G = 64, a single chain, T = 1 the table (0, 1).
CASES = [
    ("double_well", 2, 257, 3),
    ("double_well", 5, 37, 6),
    ("double_well", 32, 37, 4),
    ("double_well", 100, 37, 4),
    ("double_well", 256, 37, 6),
    ("harmonic", 100, 1, 12),
    ("gaussian", 32, 37, 6),
    ("gaussian", 100, 37, 4),
    ("gmm", 2, 257, 3),
    ("gmm", 32, 37, 6),
    ("rastrigin", 5, 37, 6),
    ("double_well", 32, 37, 1),
]


# Rosenbrock and Ackley at the smallest dim of every lane geometry (tempering_cases.LANDSCAPE_CASES; one vector per lane here),
# with the step sizes of STEP_C_AT below; ackley_c3 is Ackley's product form (c = 3), and one case is a single chain.  Proposals
# rejected on the CPU restatement, in the order of the list:
#   rosenbrock 186 of 771, 23 of 222, 13 of 148, 22 of 148, 9 of 148, 13 of 148, 20 of 222; 1 of 12 (one chain)
#   ackley     279 of 771, 69 of 222, 18 of 148, 40 of 148, 34 of 148, 26 of 148, 74 of 222; 4 of 148 (c = 3)
_LANDSCAPE_SHAPES = [(2, 257, 3), (5, 37, 6), (12, 37, 4), (32, 37, 4), (64, 37, 4), (100, 37, 4), (256, 37, 6)]
LANDSCAPE_CASES = ([("rosenbrock",) + s for s in _LANDSCAPE_SHAPES] + [("rosenbrock", 100, 1, 12)]
                   + [("ackley",) + s for s in _LANDSCAPE_SHAPES] + [("ackley_c3", 12, 37, 4)])


def base_std_of(kind):
    return start_scale(kind)


# The landscapes of LANDSCAPE_CASES: a factor per (kind, dim), chosen on the CPU restatement so that every case rejects between
# 2 % and 50 % of its proposals (tempering_hmc_cases.STEP_C_AT has the replica-exchange cases' own).
STEP_C_AT = {
    ("rosenbrock", 2): 0.28, ("rosenbrock", 5): 0.28, ("rosenbrock", 12): 0.28, ("rosenbrock", 32): 0.4, ("rosenbrock", 64): 0.4,
    ("rosenbrock", 100): 0.5, ("rosenbrock", 256): 0.6,
    ("ackley", 2): 0.3, ("ackley", 5): 0.6, ("ackley", 12): 0.6, ("ackley", 32): 1.0, ("ackley", 64): 1.0, ("ackley", 100): 1.0,
    ("ackley", 256): 1.6,
}


def step_c(kind, dim):
    kind = "ackley" if kind == "ackley_c3" else kind
    return STEP_C_AT[(kind, dim)] if (kind, dim) in STEP_C_AT else 2.0 * STEP_C[kind]


def step_sizes(kind, dim, T):
    """One step size per transition, each a little shorter than the one before: the kernel has to read the table."""
    base = step_c(kind, dim) * (2.0 / dim) ** 0.25  # (STEP_C: twice the replica-exchange cases': a walk that starts in the base's equilibrium rejects little)
    return tuple(base * (1.0 - 0.02 * t) for t in range(T))


def draw_inputs(seed, n, dim, T, base_std):
    g = torch.Generator().manual_seed(seed)
    x0 = f32(base_std) * torch.randn(n, dim, generator=g)
    return x0, torch.randn(T, n, dim, generator=g), torch.rand(T, n, generator=g)


@functools.lru_cache(maxsize=None)
def case(kind, dim, n, T):
    """Inputs and both restatements of a case, computed once per session and shared (read-only) by the tests that use it.  The
    seed is the first whose fp64 restatement has no accept decision closer than MARGIN_BAR to its threshold."""
    from helpers import to64

    spec = energy_spec(kind, dim)
    betas, eps, L, s0 = sigmoid_betas(T), step_sizes(kind, dim, T), leapfrog_steps(dim), base_std_of(kind)
    for seed in range(200):
        x0, z, u = draw_inputs(seed, n, dim, T, s0)
        ref64 = restate(to64(oracle_of(spec)), x0, z, u, betas, eps, L, s0, torch.float64)
        if ref64["margin"].min().item() > MARGIN_BAR:
            break
    ref32 = restate(oracle_of(spec), x0, z, u, betas, eps, L, s0, torch.float32)
    return {"spec": spec, "betas": betas, "eps": eps, "L": L, "base_std": s0, "x0": x0, "z": z, "u": u, "ref32": ref32,
            "ref64": ref64, "seed": seed, "shape": (n, dim), "T": T}
