"""Replica-exchange Langevin: an independent restatement of the algorithm (include/ebm_hip.h, ebm_tempering_chain_f32) in
torch ops on the oracle energies, the cases the tests run, and their inputs.  Shared by test_tempering.py (CPU tier) and
test_tempering_gpu.py; it never calls the package's sampler."""

import functools
import math

import torch

import oracle

MARGIN_BAR = 2e-4  # the project's HMC bar on |u - a| (no accept / reject call of the fp64 run may be borderline)


class Rastrigin:
    """E = a dim + sum_j x_j^2 - a cos(2 pi x_j), gradient by autograd as the reference computes it."""

    def __init__(self, a=10.0):
        self.a = a

    def energy(self, x):
        return self.a * x.shape[-1] + torch.sum(x**2 - self.a * torch.cos(2 * math.pi * x), dim=-1)

    def grad(self, x):
        with torch.enable_grad():
            leaf = x.detach().clone().requires_grad_(True)
            e = self.energy(leaf)
            (g,) = torch.autograd.grad(e, leaf, grad_outputs=torch.ones_like(e))
        return g.detach()


class Landscape:
    """A landscape energy of the package (Rosenbrock, Ackley): the model's CPU forward with an autograd gradient, in the
    dtype of the state it is handed -- fp32 the oracle, float64 the referee (the parameters are Python doubles: to64 has
    nothing to upcast)."""

    def __init__(self, model):
        self.model = model

    def energy(self, x):
        return self.model.forward(x)

    def grad(self, x):
        with torch.enable_grad():
            leaf = x.detach().clone().requires_grad_(True)
            e = self.energy(leaf)
            (g,) = torch.autograd.grad(e, leaf, grad_outputs=torch.ones_like(e))
        return g.detach()


def ladder(sigma, temps):
    """noise_coef[R], beta[R]: formed in double, rounded to fp32 once."""
    t = torch.tensor(list(temps), dtype=torch.float64)
    return torch.sqrt(2.0 * sigma**2 * t).float(), (1.0 / (sigma**2 * t)).float()


def restate(energy, x0, noise, u, eta, sigma, temps, swap_every, dtype=torch.float32, thin=None):
    """x0 [n, R, dim], noise [k, n, R, dim], u [events, n, R] -> final states [n, R, dim], the decision mask
    [events, n, R - 1] (False for unpaired slots), the margins |u - a| (inf where nothing was decided or delta is NaN) and
    the kept slot-0 states [n, k // thin, dim]."""
    n, R, dim = x0.shape
    coef, beta = ladder(sigma, temps)
    coef, beta = coef.to(dtype).view(1, R, 1), beta.to(dtype)
    x = x0.to(dtype).clone()
    masks, margins, kept = [], [], []
    m = 0
    for s in range(noise.shape[0]):
        g = energy.grad(x.reshape(n * R, dim)).view(n, R, dim)
        x1 = x - eta * g
        dw = noise[s].to(dtype) * (eta**0.5)
        x = x1 + coef * dw
        if (s + 1) % swap_every == 0:
            e = energy.energy(x.reshape(n * R, dim)).view(n, R)
            mask = torch.zeros(n, R - 1, dtype=torch.bool)
            margin = torch.full((n, R - 1), float("inf"), dtype=torch.float64)
            for r in range(m % 2, R - 1, 2):
                delta = (beta[r] - beta[r + 1]) * (e[:, r] - e[:, r + 1])
                a = torch.exp(delta.clamp(max=0.0))
                ur = u[m, :, r].to(dtype)
                ok = (delta == delta) & (ur < a)
                mask[:, r] = ok
                margin[:, r] = torch.where(delta == delta, (ur - a).abs().double(), margin[:, r])
                lower = x[:, r].clone()
                x[:, r] = torch.where(ok[:, None], x[:, r + 1], lower)
                x[:, r + 1] = torch.where(ok[:, None], lower, x[:, r + 1])
            masks.append(mask)
            margins.append(margin)
            m += 1
        if thin is not None and (s + 1) % thin == 0:
            kept.append(x[:, 0].clone())
    return {
        "x": x,
        "mask": torch.stack(masks) if masks else torch.zeros(0, n, R - 1, dtype=torch.bool),
        "margin": torch.stack(margins) if margins else torch.zeros(0, n, R - 1, dtype=torch.float64),
        "traj": torch.stack(kept, dim=1) if kept else None,
    }


TEMPS = {2: (1.0, 2.0), 3: (1.0, 2.0, 4.0), 4: (1.0, 2.0, 4.0, 8.0), 5: (1.0, 1.5, 2.25, 3.5, 5.0),
         8: (1.0, 1.4, 2.0, 2.8, 4.0, 5.6, 8.0, 11.0)}


def energy_spec(kind, dim):
    """A dict in the form tests/helpers.py turns into an oracle energy and a package model (landscapes: handled here)."""
    g = torch.Generator().manual_seed(1000 + dim)
    if kind == "double_well":
        return {"kind": kind, "h": 2.0, "b": 1.0}
    if kind == "harmonic":
        return {"kind": kind, "k": 1.5}
    if kind == "gaussian":
        a = torch.randn(dim, dim, generator=g) / dim**0.5
        return {"kind": kind, "mean": 0.3 * torch.randn(dim, generator=g), "cov": a @ a.T + 0.5 * torch.eye(dim)}
    if kind == "gmm":
        return {"kind": kind, "means": 1.5 * torch.randn(8, dim, generator=g), "sigma": 1.0}
    if kind == "rastrigin":
        return {"kind": kind, "a": 1.0}
    if kind == "rosenbrock":  # b = 4: at the default b = 100 ETA below is past the Euler stability limit of the hot slots
        return {"kind": kind, "a": 1.0, "b": 4.0}
    if kind == "ackley":
        return {"kind": kind, "a": 20.0, "b": 0.2, "c": 2.0 * math.pi}
    if kind == "ackley_c3":  # c != 2 pi: the kernels' product form sincosf(c x)
        return {"kind": "ackley", "a": 20.0, "b": 0.2, "c": 3.0}
    raise ValueError(kind)


def oracle_of(spec):
    from helpers import oracle_energy

    if spec["kind"] in ("rosenbrock", "ackley"):
        return Landscape(model_of(spec))
    return Rastrigin(spec["a"]) if spec["kind"] == "rastrigin" else oracle_energy(spec)


def model_of(spec, device=None):
    import torchebm_amd as ta
    from helpers import package_model

    if spec["kind"] == "rosenbrock":
        return ta.core.RosenbrockModel(a=spec["a"], b=spec["b"], device=device)
    if spec["kind"] == "ackley":
        return ta.core.AckleyModel(a=spec["a"], b=spec["b"], c=spec["c"], device=device)
    return ta.core.RastriginModel(a=spec["a"], device=device) if spec["kind"] == "rastrigin" else package_model(spec, device)


def start_scale(kind):
    """The scale of the normal starts: the rippled and the curved-valley landscapes start nearer their minima."""
    return 0.6 if kind in ("rastrigin", "rosenbrock") else 1.0


# (kind, dim, R, n_ladders, swap_every, k): the smallest shapes that reach every hazard of the kernel --
#   dim 2 one lane per walker, 5 unaligned rows, 32 full rows, 100 G = 32 not full, 256 G = 64 (a ladder over several waves),
#   260 two vectors per lane; R = 3 at dim 100 and R = 5 at dim 32 leave idle lane groups; 257 ladders fill several workgroups;
#   swap_every 1 has both parities on consecutive steps, 100 > k has no event; every other case has at least 4 events.
EXACT_CASES = [
    ("double_well", 2, 4, 257, 1, 6),
    ("double_well", 5, 3, 37, 3, 12),
    ("double_well", 32, 5, 37, 1, 5),
    ("double_well", 32, 8, 257, 3, 12),
    ("double_well", 100, 3, 37, 1, 4),
    ("double_well", 256, 2, 1, 1, 4),
    ("double_well", 256, 4, 37, 3, 12),
    ("double_well", 260, 2, 37, 1, 4),
    ("double_well", 32, 4, 37, 100, 6),
    ("harmonic", 5, 2, 257, 1, 4),
    ("harmonic", 100, 3, 1, 3, 12),
    ("harmonic", 260, 3, 37, 1, 4),
]
YARDSTICK_CASES = [
    ("gaussian", 5, 3, 37, 1, 6),
    ("gaussian", 32, 5, 257, 3, 12),
    ("gaussian", 100, 2, 37, 1, 4),
    ("gmm", 2, 4, 257, 1, 6),
    ("gmm", 32, 8, 37, 3, 12),
    ("gmm", 100, 3, 37, 1, 4),
    ("gmm", 260, 2, 37, 3, 12),
    ("rastrigin", 5, 3, 37, 1, 6),
    ("rastrigin", 32, 4, 257, 3, 12),
    ("rastrigin", 260, 2, 37, 1, 4),
]
# The two landscapes with a structure along the row -- Rosenbrock's neighbour exchange, Ackley's mean over dim -- at the smallest
# dim of every lane geometry: 2 G = 1, 5 G = 2 masked, 12 G = 4 masked, 32 G = 8 full, 64 G = 16 (the DPP wrap over a whole
# 16-lane row), 100 G = 32 masked (__shfl), 256 G = 64 full (R = 4: one ladder over four waves), 260 two vectors per lane.
# R = 3 at dim 100 and R = 5 at dim 32 leave idle lane groups.  ackley_c3 is Ackley's product form (c = 3), and one case is
# a single ladder.  Swaps accepted on the CPU restatement, in the order of the list:
#   rosenbrock 1740 of 2313, 133 of 222, 170 of 333, 143 of 296, 76 of 333, 39 of 148, 11 of 222, 17 of 74; 1 of 4 (one ladder)
#   ackley     1829 of 2313, 182 of 222, 294 of 333, 284 of 296, 314 of 333, 140 of 148, 205 of 222, 66 of 74; 293 of 333 (c = 3)
_LANDSCAPE_SHAPES = [(2, 4, 257, 1, 6), (5, 3, 37, 1, 6), (12, 4, 37, 1, 6), (32, 5, 37, 3, 12), (64, 4, 37, 1, 6), (100, 3, 37, 1, 4),
                     (256, 4, 37, 3, 12), (260, 2, 37, 1, 4)]
LANDSCAPE_CASES = ([("rosenbrock",) + s for s in _LANDSCAPE_SHAPES] + [("rosenbrock", 100, 3, 1, 3, 12)]
                   + [("ackley",) + s for s in _LANDSCAPE_SHAPES] + [("ackley_c3", 12, 4, 37, 1, 6)])
ETA, SIGMA = 0.004, 1.0  # (a step size at which the hottest slot of the double well stays stable from these starts)


def draw_inputs(seed, n, R, dim, k, swap_every, scale):
    g = torch.Generator().manual_seed(seed)
    x0 = scale * torch.randn(n, R, dim, generator=g)
    noise = torch.randn(k, n, R, dim, generator=g)
    u = torch.rand(max(k // swap_every, 1), n, R, generator=g)[: k // swap_every]
    return x0, noise, u


@functools.lru_cache(maxsize=None)
def case(kind, dim, R, n, swap_every, k):
    """Inputs and both restatements of a case, computed once per session and shared (read-only) by the tests that use it.
    The seed is the first whose fp64 restatement has no decision closer than MARGIN_BAR to its threshold."""
    spec = energy_spec(kind, dim)
    temps = TEMPS[R]
    scale = start_scale(kind)
    for seed in range(200):
        x0, noise, u = draw_inputs(seed, n, R, dim, k, swap_every, scale)
        from helpers import to64

        ref64 = restate(to64(oracle_of(spec)), x0, noise, u, ETA, SIGMA, temps, swap_every, torch.float64)
        if ref64["margin"].numel() == 0 or ref64["margin"].min().item() > MARGIN_BAR:
            break
    ref32 = restate(oracle_of(spec), x0, noise, u, ETA, SIGMA, temps, swap_every, torch.float32)
    return {"spec": spec, "temps": temps, "x0": x0, "noise": noise, "u": u, "ref32": ref32, "ref64": ref64, "seed": seed,
            "shape": (n, R, dim), "k": k, "swap_every": swap_every}
