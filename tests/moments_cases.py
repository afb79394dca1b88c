"""Per-chain running moments: an independent restatement of the algorithm (include/ebm_hip.h, ebm_chain_moments_f32) in torch ops
on the oracle energies -- the Euler-Maruyama step, the literal safe-mode leapfrog sequence of oracle/hmc.py, and the Welford
recurrence exactly as specified -- the cases the tests run, and their inputs.  Shared by test_moments.py (CPU tier) and
test_moments_gpu.py; it never calls the package's samplers."""

import functools

import torch

from ais_cases import f32  # noqa: F401
from tempering_cases import ETA, SIGMA, energy_spec, model_of, oracle_of, start_scale  # noqa: F401
from tempering_hmc_cases import MARGIN_BAR, leapfrog_steps, step_sizes  # noqa: F401  (the bar ais_cases uses)


def recip_table(h):
    """float32(1 / c), c = 1 .. h: formed in double, rounded once."""
    return (1.0 / torch.arange(1, h + 1, dtype=torch.float64)).to(torch.float32)


def welford(traj, h, dtype=torch.float32, recip=None):
    """traj [n, 2 h, ...] -> mean, M2 of shape [2, n, ...]: the recurrence of the contract, every operation rounded on its own in
    `dtype`, with the fp32 reciprocal table (float64: the same table, upcast)."""
    assert traj.shape[1] == 2 * h
    rc = (recip_table(h) if recip is None else recip).to(dtype)
    t = traj.to(dtype)
    shape = (2, t.shape[0]) + tuple(t.shape[2:])
    mean, m2 = torch.zeros(shape, dtype=dtype), torch.zeros(shape, dtype=dtype)
    for j in range(2 * h):
        half, c = divmod(j, h)
        x = t[:, j]
        d = x - mean[half]
        mean[half] = mean[half] + d * rc[c]
        m2[half] = m2[half] + d * (x - mean[half])
    return mean, m2


def two_pass(traj, h):
    """float64 moments of the same trajectory by the textbook two passes: mean, sum of squared deviations, [2, n, ...]."""
    t = traj.double()
    halves = torch.stack((t[:, :h], t[:, h:]))  # [2, n, h, ...]
    mean = halves.mean(dim=2)
    return mean, ((halves - mean.unsqueeze(2)) ** 2).sum(dim=2)


def split(k, burn_in):
    assert (k - burn_in) % 2 == 0 and (k - burn_in) // 2 >= 2
    return (k - burn_in) // 2


def restate_langevin(energy, x0, noise, eta, sigma, burn_in, dtype=torch.float32):
    """x0 [n, dim], noise [k, n, dim] -> the final states, the counted states [n, 2 h, dim] and their energies [n, 2 h]."""
    k = noise.shape[0]
    split(k, burn_in)
    sqrt_eta, coef = eta**0.5, (2.0 * sigma**2) ** 0.5
    x = x0.to(dtype).clone()
    kept, e_kept = [], []
    for s in range(k):
        x1 = x - eta * energy.grad(x)
        dw = noise[s].to(dtype) * sqrt_eta
        x = x1 + coef * dw
        if s >= burn_in:
            kept.append(x.clone())
            e_kept.append(energy.energy(x))
    return {"x": x, "traj": torch.stack(kept, dim=1), "e_traj": torch.stack(e_kept, dim=1)}


def _hamiltonian(e, p):
    return e.clamp(min=-1e10, max=1e10) + (0.5 * torch.sum(p.square(), dim=-1)).clamp_(min=0.0, max=1e10)


def restate_hmc(energy, x0, z, u, eps, n_leapfrog, burn_in, dtype=torch.float32):
    """x0 [n, dim], z [k, n, dim], u [k, n] -> the final states, the accept mask [k, n], the margins |u - a| (inf where the
    threshold is NaN), the counted states [n, 2 h, dim] (a rejected proposal counts the held state again) and their energies."""
    k = z.shape[0]
    split(k, burn_in)
    force = lambda q: (-energy.grad(q)).clamp_(min=-1e6, max=1e6)  # noqa: E731
    eps_t = torch.tensor(f32(eps), dtype=dtype)  # the fp32 scalar (oracle/hmc.py: eps as a tensor of the state's dtype)
    x = x0.to(dtype).clone()
    e = energy.energy(x)
    accepted, margins, kept, e_kept = [], [], [], []
    for t in range(k):
        p = z[t].to(dtype)
        h0 = _hamiltonian(e, p)
        xp = x
        for _ in range(n_leapfrog):  # oracle/hmc.py leapfrog(), safe mode, identity mass
            p_half = p + 0.5 * eps_t * force(xp)
            xp = xp + eps_t * p_half
            p = p_half + 0.5 * eps_t * force(xp)
            xp = xp.nan_to_num_(nan=0.0)
            p = p.nan_to_num_(nan=0.0)
        e1 = energy.energy(xp)
        h1 = _hamiltonian(e1, p)
        a = torch.exp((h0 - h1).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
        ut = u[t].to(dtype)
        acc = ut < a
        accepted.append(acc)
        margins.append(torch.where(a == a, (ut - a).abs().double(), torch.full((), float("inf"), dtype=torch.float64)))
        x = torch.where(acc[:, None], xp, x)
        e = torch.where(acc, e1, e)
        if t >= burn_in:
            kept.append(x.clone())
            e_kept.append(e.clone())
    return {"x": x, "accepted": torch.stack(accepted), "margin": torch.stack(margins), "traj": torch.stack(kept, dim=1),
            "e_traj": torch.stack(e_kept, dim=1)}


# (kind, dim, n, k_steps, burn_in): the geometry edges -- dim 2 one lane per chain, 5 masked, 32 full rows (G = 8), 100 masked
# (G = 32), 256 (G = 64); 9 chains a partial wave, 37 an odd count, 257 several workgroups and a tail; (4, 0) the shortest halves
# (h = 2), (11, 3) and (40, 6) a burn-in in front of h = 4 and h = 17.  Every one of the seven kinds under both samplers.
ELEMENTWISE = ("double_well", "harmonic")
LANGEVIN_CASES = [
    ("double_well", 2, 257, 4, 0),
    ("double_well", 5, 37, 11, 3),
    ("double_well", 32, 37, 40, 6),
    ("double_well", 100, 9, 11, 3),
    ("double_well", 256, 37, 4, 0),
    ("harmonic", 5, 257, 11, 3),
    ("harmonic", 100, 37, 40, 6),
    ("gaussian", 5, 37, 11, 3),
    ("gaussian", 256, 9, 4, 0),
    ("gmm", 32, 37, 40, 6),
    ("rosenbrock", 12, 37, 11, 3),
    ("ackley", 100, 37, 11, 3),
    ("rastrigin", 32, 257, 4, 0),
]
HMC_CASES = [
    ("double_well", 2, 257, 4, 0),
    ("double_well", 5, 37, 11, 3),
    ("double_well", 32, 37, 40, 6),
    ("double_well", 100, 37, 11, 3),
    ("double_well", 256, 9, 4, 0),
    ("harmonic", 5, 257, 11, 3),
    ("harmonic", 100, 37, 40, 6),
    ("gaussian", 5, 37, 11, 3),
    ("gaussian", 256, 9, 4, 0),
    ("gmm", 32, 37, 40, 6),
    ("rosenbrock", 12, 37, 11, 3),
    ("ackley", 100, 37, 11, 3),
    ("rastrigin", 32, 257, 4, 0),
]


def hmc_step(kind, dim):
    """(eps, n_leapfrog): the cold slot's of the replica-exchange cases, a little longer so that proposals are rejected."""
    return 1.5 * step_sizes(kind, dim, 1)[0], leapfrog_steps(dim)


@functools.lru_cache(maxsize=None)
def langevin_case(kind, dim, n, k, burn_in):
    """Inputs and both restatements of a Langevin case, computed once per session and shared (read-only)."""
    from helpers import to64

    spec = energy_spec(kind, dim)
    g = torch.Generator().manual_seed(4000 + dim + n)
    x0 = start_scale(kind) * torch.randn(n, dim, generator=g)
    noise = torch.randn(k, n, dim, generator=g)
    ref32 = restate_langevin(oracle_of(spec), x0, noise, ETA, SIGMA, burn_in, torch.float32)
    ref64 = restate_langevin(to64(oracle_of(spec)), x0, noise, ETA, SIGMA, burn_in, torch.float64)
    return {"spec": spec, "x0": x0, "noise": noise, "ref32": ref32, "ref64": ref64, "h": split(k, burn_in), "shape": (n, dim),
            "k": k, "burn_in": burn_in}


@functools.lru_cache(maxsize=None)
def hmc_case(kind, dim, n, k, burn_in):
    """Inputs and both restatements of an HMC case.  The seed is the first whose fp64 restatement has no accept decision closer
    than MARGIN_BAR to its threshold."""
    from helpers import to64

    spec = energy_spec(kind, dim)
    eps, L = hmc_step(kind, dim)
    for seed in range(200):
        g = torch.Generator().manual_seed(seed)
        x0 = start_scale(kind) * torch.randn(n, dim, generator=g)
        z, u = torch.randn(k, n, dim, generator=g), torch.rand(k, n, generator=g)
        ref64 = restate_hmc(to64(oracle_of(spec)), x0, z, u, eps, L, burn_in, torch.float64)
        if ref64["margin"].min().item() > MARGIN_BAR:
            break
    ref32 = restate_hmc(oracle_of(spec), x0, z, u, eps, L, burn_in, torch.float32)
    return {"spec": spec, "x0": x0, "z": z, "u": u, "eps": eps, "L": L, "ref32": ref32, "ref64": ref64, "seed": seed,
            "h": split(k, burn_in), "shape": (n, dim), "k": k, "burn_in": burn_in}
