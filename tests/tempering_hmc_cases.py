"""Replica-exchange HMC: an independent restatement of the algorithm (include/ebm_hip.h, ebm_tempering_hmc_chain_f32) in
torch ops on the oracle energies -- the literal safe-mode leapfrog sequence of oracle/hmc.py with a step size per slot --
the cases the tests run, and their inputs.  Shared by test_tempering_hmc.py (CPU tier) and test_tempering_hmc_gpu.py; it
never calls the package's sampler."""

import functools

import torch

import tempering_cases
from tempering_cases import TEMPS, energy_spec, model_of, oracle_of  # noqa: F401  (re-exported for the tests)

MARGIN_BAR = 2e-4  # the project's HMC bar on |u - a| (no accept / reject / swap call of the fp64 run may be borderline)


def ladder(temps):
    """sqrt_temp[R], beta[R]: formed in double, rounded to fp32 once."""
    t = torch.tensor(list(temps), dtype=torch.float64)
    return torch.sqrt(t).float(), (1.0 / t).float()


def _force(energy, x):
    n, R, dim = x.shape
    return (-energy.grad(x.reshape(n * R, dim)).view(n, R, dim)).clamp_(min=-1e6, max=1e6)


def _hamiltonian(e, w):
    return e.clamp(min=-1e10, max=1e10) + (0.5 * torch.sum(w.square(), dim=-1)).clamp_(min=0.0, max=1e10)


def restate(energy, x0, z, u_accept, u_swap, eps, n_leapfrog, temps, swap_every, dtype=torch.float32, thin=None,
            sqrt_temp=None, beta=None):
    """x0 [n, R, dim], z [n_mh, n, R, dim], u_accept [n_mh, n, R], u_swap [events, n, R], eps: R step sizes ->
    final states [n, R, dim], the MH mask [n_mh, n, R], the swap mask [events, n, R - 1] (False for unpaired slots), the
    margins |u - a| of both (inf where nothing was decided or the threshold is NaN) and the kept slot-0 states."""
    n, R, dim = x0.shape
    if sqrt_temp is None:
        sqrt_temp, beta = ladder(temps)
    sqrt_temp, beta = sqrt_temp.to(dtype).view(1, R, 1), beta.to(dtype)
    eps_t = torch.tensor([float(v) for v in eps], dtype=dtype).view(1, R, 1)  # (oracle/hmc.py: eps as a tensor of the state's dtype)
    x = x0.to(dtype).clone()
    flat = lambda t: t.reshape(n * R, dim)  # noqa: E731
    accepted, mh_margin, masks, margins, kept = [], [], [], [], []
    m = 0
    for t in range(z.shape[0]):
        w = z[t].to(dtype) * sqrt_temp
        e0 = energy.energy(flat(x)).view(n, R)
        h0 = _hamiltonian(e0, w)
        xp = x
        for _ in range(n_leapfrog):  # oracle/hmc.py leapfrog(), safe mode, identity mass
            w_half = w + 0.5 * eps_t * _force(energy, xp)
            xp = xp + eps_t * w_half
            w = w_half + 0.5 * eps_t * _force(energy, xp)
            xp = xp.nan_to_num_(nan=0.0)
            w = w.nan_to_num_(nan=0.0)
        e1 = energy.energy(flat(xp)).view(n, R)
        h1 = _hamiltonian(e1, w)
        a = torch.exp((beta * (h0 - h1)).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
        ut = u_accept[t].to(dtype)
        acc = ut < a
        accepted.append(acc)
        mh_margin.append(torch.where(a == a, (ut - a).abs().double(), torch.full((), float("inf"), dtype=torch.float64)))
        x = torch.where(acc[:, :, None], xp, x)
        e = torch.where(acc, e1, e0)  # the energies of the states the slots now hold
        if (t + 1) % swap_every == 0:
            mask = torch.zeros(n, R - 1, dtype=torch.bool)
            margin = torch.full((n, R - 1), float("inf"), dtype=torch.float64)
            for r in range(m % 2, R - 1, 2):
                delta = (beta[r] - beta[r + 1]) * (e[:, r] - e[:, r + 1])
                thr = torch.exp(delta.clamp(max=0.0))
                ur = u_swap[m, :, r].to(dtype)
                ok = (delta == delta) & (ur < thr)
                mask[:, r] = ok
                margin[:, r] = torch.where(delta == delta, (ur - thr).abs().double(), margin[:, r])
                lower = x[:, r].clone()
                x[:, r] = torch.where(ok[:, None], x[:, r + 1], lower)
                x[:, r + 1] = torch.where(ok[:, None], lower, x[:, r + 1])
            masks.append(mask)
            margins.append(margin)
            m += 1
        if thin is not None and (t + 1) % thin == 0:
            kept.append(x[:, 0].clone())
    return {
        "x": x,
        "accepted": torch.stack(accepted) if accepted else torch.zeros(0, n, R, dtype=torch.bool),
        "mh_margin": torch.stack(mh_margin) if mh_margin else torch.zeros(0, n, R, dtype=torch.float64),
        "mask": torch.stack(masks) if masks else torch.zeros(0, n, R - 1, dtype=torch.bool),
        "margin": torch.stack(margins) if margins else torch.zeros(0, n, R - 1, dtype=torch.float64),
        "traj": torch.stack(kept, dim=1) if kept else None,
    }


def closest_call(ref):
    """The smallest margin of a run, MH and swap decisions together (inf when it decided nothing)."""
    both = [v.min().item() for v in (ref["mh_margin"], ref["margin"]) if v.numel()]
    return min(both) if both else float("inf")


# Step sizes c (2 / dim)^(1/4): MH acceptance 0.97 - 0.99 on these shapes, so every case of a few hundred decisions rejects
# some proposals and none is so large that an accept-everything decision (borderline with probability 2e-4) leaves no seed.
STEP_C = {"double_well": 0.12, "harmonic": 0.5, "gaussian": 0.25, "gmm": 0.45, "rastrigin": 0.05}


# The landscapes with a neighbour coupling or a mean over the row follow no one law from dim 2 to 256: a factor per (kind, dim),
# chosen on the CPU restatement so that every case of LANDSCAPE_CASES rejects between 2 % and 50 % of its proposals.
STEP_C_AT = {
    ("rosenbrock", 2): 0.2, ("rosenbrock", 5): 0.2, ("rosenbrock", 12): 0.2, ("rosenbrock", 32): 0.3, ("rosenbrock", 64): 0.3,
    ("rosenbrock", 100): 0.3, ("rosenbrock", 256): 0.45,
    ("ackley", 2): 0.3, ("ackley", 5): 0.3, ("ackley", 12): 0.6, ("ackley", 32): 1.0, ("ackley", 64): 1.0, ("ackley", 100): 1.0,
    ("ackley", 256): 1.6,
}


def step_c(kind, dim):
    kind = "ackley" if kind == "ackley_c3" else kind
    return STEP_C_AT[(kind, dim)] if (kind, dim) in STEP_C_AT else STEP_C[kind]


def step_sizes(kind, dim, R):
    """One step size per slot: the hotter slots step a little shorter, so the kernel has to follow the slot's own value."""
    base = step_c(kind, dim) * (2.0 / dim) ** 0.25
    return tuple(base * (1.0 - 0.02 * r) for r in range(R))


def leapfrog_steps(dim):
    return {2: 5, 5: 4, 32: 3, 100: 4, 256: 3}.get(dim, 4)  # (dims 12 and 64 of the landscape cases: 4)


# (kind, dim, R, n_ladders, swap_every, n_mh): the smallest shapes that reach every hazard of the kernel -- dim 2 one lane
# per walker, 5 unaligned rows, 32 full rows, 100 G = 32 not full, 256 G = 64 (a ladder over several waves); R = 3 at dim 100
# and R = 5 at dim 32 leave idle lane groups; 257 ladders fill several workgroups; swap_every 1 has both parities on
# consecutive transitions.  At most about 4000 decisions each.
CASES = [
    ("double_well", 2, 4, 257, 1, 3),
    ("double_well", 5, 3, 37, 2, 6),
    ("double_well", 32, 8, 37, 1, 4),
    ("double_well", 100, 3, 37, 1, 4),
    ("double_well", 256, 4, 37, 2, 6),
    ("harmonic", 100, 3, 1, 3, 12),
    ("gaussian", 32, 5, 37, 2, 6),
    ("gaussian", 100, 2, 37, 1, 4),
    ("gmm", 2, 4, 257, 1, 3),
    ("gmm", 32, 8, 37, 2, 6),
    ("gmm", 100, 3, 37, 1, 4),
    ("rastrigin", 5, 3, 37, 1, 6),
    ("rastrigin", 32, 4, 37, 2, 6),
]


# Rosenbrock and Ackley at the smallest dim of every lane geometry (tempering_cases.LANDSCAPE_CASES; one vector per lane here),
# with the step sizes of STEP_C_AT; ackley_c3 is Ackley's product form (c = 3), and one case is a single ladder.  On the CPU
# restatement, in the order of the list (proposals rejected; swaps accepted):
#   rosenbrock 611 of 3084, 97 of 666, 57 of 592, 229 of 1110, 101 of 592, 32 of 444, 305 of 888; 5 of 36 (one ladder)
#              974 of 1285, 62 of 111, 106 of 222, 80 of 222, 35 of 222, 10 of 148, 6 of 185; 0 of 4
#   ackley     1300 of 3084, 73 of 666, 119 of 592, 186 of 1110, 69 of 592, 47 of 444, 52 of 888; 29 of 592 (c = 3)
#              839 of 1285, 58 of 111, 125 of 222, 161 of 222, 133 of 222, 76 of 148, 106 of 185; 126 of 222
_LANDSCAPE_SHAPES = [(2, 4, 257, 1, 3), (5, 3, 37, 2, 6), (12, 4, 37, 1, 4), (32, 5, 37, 2, 6), (64, 4, 37, 1, 4), (100, 3, 37, 1, 4),
                     (256, 4, 37, 2, 6)]
LANDSCAPE_CASES = ([("rosenbrock",) + s for s in _LANDSCAPE_SHAPES] + [("rosenbrock", 100, 3, 1, 3, 12)]
                   + [("ackley",) + s for s in _LANDSCAPE_SHAPES] + [("ackley_c3", 12, 4, 37, 1, 4)])


def draw_inputs(seed, n, R, dim, n_mh, swap_every, scale):
    g = torch.Generator().manual_seed(seed)
    x0 = scale * torch.randn(n, R, dim, generator=g)
    z = torch.randn(n_mh, n, R, dim, generator=g)
    u_accept = torch.rand(n_mh, n, R, generator=g)
    u_swap = torch.rand(max(n_mh // swap_every, 1), n, R, generator=g)[: n_mh // swap_every]
    return x0, z, u_accept, u_swap


@functools.lru_cache(maxsize=None)
def case(kind, dim, R, n, swap_every, n_mh):
    """Inputs and both restatements (with the slot-0 states kept at thin = 2) of a case, computed once per session and shared
    (read-only) by the tests that use it.  The seed is the first whose fp64 restatement has no MH or swap decision closer
    than MARGIN_BAR to its threshold."""
    from helpers import to64

    spec = energy_spec(kind, dim)
    temps, eps, L = TEMPS[R], step_sizes(kind, dim, R), leapfrog_steps(dim)
    scale = tempering_cases.start_scale(kind)
    for seed in range(200):
        x0, z, ua, us = draw_inputs(seed, n, R, dim, n_mh, swap_every, scale)
        ref64 = restate(to64(oracle_of(spec)), x0, z, ua, us, eps, L, temps, swap_every, torch.float64, thin=2)
        if closest_call(ref64) > MARGIN_BAR:
            break
    ref32 = restate(oracle_of(spec), x0, z, ua, us, eps, L, temps, swap_every, torch.float32, thin=2)
    return {"spec": spec, "temps": temps, "eps": eps, "L": L, "x0": x0, "z": z, "u_accept": ua, "u_swap": us, "ref32": ref32,
            "ref64": ref64, "seed": seed, "shape": (n, R, dim), "n_mh": n_mh, "swap_every": swap_every}


# ---------------------------------------------------------------------------------
# both ladders, states that cannot move: only the swap events act
# ---------------------------------------------------------------------------------
FROZEN_EVENTS = 6  # swap_every = 1: both parities, three times each


def frozen_masks(c):
    """Both restatements on the inputs of frozen_case: the Langevin ladder at eta = 0 with zero noise, the HMC ladder at
    eps = 0 in every slot (dH = 0 exactly, so every proposal -- the unchanged state -- is accepted).  The same u feeds the swaps."""
    (n, R, dim), energy = c["shape"], oracle_of(c["spec"])
    lan = tempering_cases.restate(energy, c["x0"], torch.zeros(FROZEN_EVENTS, n, R, dim), c["u"], 0.0, tempering_cases.SIGMA,
                                  c["temps"], 1, torch.float32)
    hmc = restate(energy, c["x0"], c["z"], c["u_accept"], c["u"], (0.0,) * R, c["L"], c["temps"], 1, torch.float32)
    return lan, hmc


@functools.lru_cache(maxsize=None)
def frozen_case(kind, dim, R, n):
    """Inputs of a run in which no state moves, so the final slot matrix is a permutation of the start made by the swap decisions
    alone.  The seed is the first at which the Langevin restatement both accepts and rejects swaps.  (sigma = 1: both ladders
    have beta = 1 / T, rounded once.)"""
    spec, temps = energy_spec(kind, dim), TEMPS[R]
    attempts = sum(len(range(m % 2, R - 1, 2)) for m in range(FROZEN_EVENTS)) * n
    for seed in range(200):
        x0, z, ua, u = draw_inputs(seed, n, R, dim, FROZEN_EVENTS, 1, 1.0)
        c = {"spec": spec, "temps": temps, "x0": x0, "z": z, "u_accept": ua, "u": u, "L": 2, "seed": seed, "shape": (n, R, dim),
             "attempts": attempts}
        if 0 < int(frozen_masks(c)[0]["mask"].sum()) < attempts:
            break
    return c


def slot_permutation(x, x0):
    """perm [n, R] with x[:, r] == x0[:, perm[:, r]] bit for bit; every state of a ladder must be found exactly once."""
    same = (x[:, :, None, :] == x0[:, None, :, :]).all(dim=-1)  # [n, R now, R at the start]
    assert (same.sum(dim=-1) == 1).all() and (same.sum(dim=-2) == 1).all(), "a state moved"
    return same.long().argmax(dim=-1)
