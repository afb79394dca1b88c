"""BAOAB and generalized HMC with a scalar or diagonal mass: independent restatements of the two recurrences (include/ebm_hip.h,
ebm_kinetic_chain_mass_f32 and ebm_ghmc_chain_mass_f32) in torch ops on the oracle energies, the cases the tests run, and their
inputs.  Shared by test_mass.py (CPU tier) and test_mass_gpu.py; it never calls the package's samplers.  The constants, the
energies, the step sizes and the decision margin are those of kinetic_cases.py, ghmc_cases.py and tempering_cases.py."""

import functools
import math

import torch

import ghmc_cases
import kinetic_cases
from tempering_cases import energy_spec, model_of, oracle_of, start_scale  # noqa: F401  (re-exported for the tests)

GAMMA, TEMP = kinetic_cases.GAMMA, kinetic_cases.TEMP  # 1.5 and 0.8, as in the unit-mass cases
MARGIN_BAR = ghmc_cases.MARGIN_BAR
SEED_CAP = 20  # seeds tried per GHMC case
SCALAR_MASS = 0.37


def diag_mass(dim):
    """exp(U(-log 2, log 4)) per coordinate, fp32, from a generator seeded with the width."""
    g = torch.Generator().manual_seed(4200 + dim)
    return torch.exp(-math.log(2.0) + (math.log(4.0) + math.log(2.0)) * torch.rand(dim, generator=g))


def mass_of(form, dim):
    """The mass of a case as the samplers and the entries take it: the float, or the fp32 [dim] tensor."""
    return SCALAR_MASS if form == "scalar" else diag_mass(dim)


def forms(mass, dtype):
    """m_raw, m_sqrt, m_safe of the contract, formed as the entries form them in fp32 -- a scalar in double, rounded once; a diagonal
    per element with a correctly rounded square root -- then upcast to `dtype` (float64 runs the same fp32 constants)."""
    if isinstance(mass, float):
        raw, sqrt_, safe = (torch.tensor(v, dtype=torch.float64).to(torch.float32) for v in (mass, math.sqrt(mass), max(mass, 1e-10)))
    else:
        raw = mass.to(torch.float32)
        sqrt_ = raw.double().sqrt().to(torch.float32)  # (53 >= 2 * 24 + 2 bits: rounding the double root once more is the fp32 root)
        safe = torch.where(raw < 1e-10, torch.full_like(raw, 1e-10), raw)
    return raw.to(dtype), sqrt_.to(dtype), safe.to(dtype)


def min_mass(mass):
    return mass if isinstance(mass, float) else float(mass.min())


def start_momentum(mass, z):
    """sqrt(T) sqrt(m) z: a draw of N(0, T m)."""
    return math.sqrt(TEMP) * forms(mass, torch.float32)[1] * z


# ---------------------------------------------------------------------------------
# BAOAB
# ---------------------------------------------------------------------------------
def restate_baoab(energy, x0, p0, noise, h, gamma, temp, mass, thin=1, dtype=torch.float32, xi0=None):
    """x0, p0 [n, dim] (p0 None: (sqrt_temp m_sqrt) xi0), noise [k, n, dim] -> the final x and p and the kept positions
    [n, k // thin, dim].  Every operation rounded on its own in `dtype`."""
    hh, c1, c2, sqrt_temp = kinetic_cases.constants(h, gamma, temp)
    _, m_sqrt, m_safe = forms(mass, dtype)
    a, s = torch.tensor(hh, dtype=dtype) / m_safe, c2 * m_sqrt  # (a true division: `float / tensor` is reciprocal-then-multiply)
    x = x0.to(dtype).clone()
    p = ((sqrt_temp * m_sqrt) * xi0.to(dtype)) if p0 is None else p0.to(dtype).clone()
    g = energy.grad(x)
    kept = []
    for t in range(noise.shape[0]):
        p = p - hh * g
        x = x + a * p
        p = c1 * p + s * noise[t].to(dtype)
        x = x + a * p
        g = energy.grad(x)
        p = p - hh * g
        if (t + 1) % thin == 0:
            kept.append(x.clone())
    n, dim = x0.shape
    return {"x": x, "v": p, "traj": torch.stack(kept, dim=1) if kept else torch.zeros(n, 0, dim, dtype=dtype)}


# (kind, dim, n, k_steps, thin, mass form): the shapes of kinetic_cases.py -- one of every lane-group size, masked rows at 5, 12
# and 100 where a padded slot's mass can go wrong; n a partial wave, an odd count, several workgroups and a tail -- thinned, the
# two mass forms alternating over the seven kinds
BAOAB_EXACT = [
    ("double_well", 2, 257, 4, 2, "scalar"),
    ("double_well", 5, 37, 11, 3, "diag"),
    ("double_well", 12, 9, 1, 1, "diag"),
    ("double_well", 64, 257, 11, 3, "scalar"),
    ("double_well", 100, 9, 11, 3, "diag"),
    ("double_well", 256, 37, 1, 1, "diag"),
    ("harmonic", 5, 257, 1, 1, "scalar"),
    ("harmonic", 12, 37, 4, 2, "scalar"),
    ("harmonic", 32, 257, 11, 3, "diag"),
    ("harmonic", 100, 37, 1, 1, "scalar"),
    ("harmonic", 256, 257, 4, 2, "scalar"),
]
BAOAB_COUPLED = [
    ("gaussian", 5, 37, 11, 3, "diag"),
    ("gaussian", 32, 257, 4, 2, "scalar"),
    ("gaussian", 100, 37, 1, 1, "diag"),
    ("gmm", 2, 257, 4, 2, "diag"),
    ("gmm", 100, 37, 4, 2, "scalar"),
    ("rastrigin", 5, 37, 11, 3, "scalar"),
    ("rastrigin", 32, 257, 4, 2, "diag"),
    ("rosenbrock", 12, 37, 4, 2, "diag"),
    ("rosenbrock", 64, 37, 4, 2, "scalar"),
    ("ackley", 100, 37, 1, 1, "diag"),
    ("ackley", 256, 9, 11, 3, "scalar"),
]


def baoab_step(kind, mass):
    """The unit-mass case's step times sqrt(min m): h^2 E'' / m is at most what that case runs at."""
    return kinetic_cases.STEP[kind] * math.sqrt(min_mass(mass))


@functools.lru_cache(maxsize=None)
def baoab_case(kind, dim, n, k, thin, form):
    """Inputs and both restatements of a case, computed once per session and shared (read-only)."""
    from helpers import to64

    spec, mass = energy_spec(kind, dim), mass_of(form, dim)
    g = torch.Generator().manual_seed(7300 + dim + n)
    x0 = start_scale(kind) * torch.randn(n, dim, generator=g)
    p0 = start_momentum(mass, torch.randn(n, dim, generator=g))
    noise = torch.randn(k, n, dim, generator=g)
    h = baoab_step(kind, mass)
    ref32 = restate_baoab(oracle_of(spec), x0, p0, noise, h, GAMMA, TEMP, mass, thin, torch.float32)
    ref64 = restate_baoab(to64(oracle_of(spec)), x0, p0, noise, h, GAMMA, TEMP, mass, thin, torch.float64)
    return {"spec": spec, "mass": mass, "x0": x0, "v0": p0, "noise": noise, "h": h, "ref32": ref32, "ref64": ref64, "shape": (n, dim),
            "k": k, "thin": thin}


# ---------------------------------------------------------------------------------
# generalized HMC
# ---------------------------------------------------------------------------------
def _force(energy, x):
    return (-energy.grad(x)).clamp_(min=-1e6, max=1e6)


def _hamiltonian(e, p, m_raw, scalar):
    """clamp(E, +-1e10) + K_m(p): 0.5 sum(p^2 / m) of a diagonal mass, (0.5 sum p^2) / m of a scalar one, clamped to [0, 1e10]."""
    k = 0.5 * torch.sum(p.square(), dim=-1) / m_raw if scalar else 0.5 * torch.sum(p.square() / m_raw, dim=-1)
    return e.clamp(min=-1e10, max=1e10) + k.clamp_(min=0.0, max=1e10)


def restate_ghmc(energy, x0, p0, z, u, eps, n_leapfrog, gamma, temp, mass, dtype=torch.float32, thin=1, xi0=None):
    """x0, p0 [n, dim] (p0 None: (sqrt_temp m_sqrt) xi0), z [n_mh, n, dim], u [n_mh, n] -> the final x and p, the kept positions,
    the decisions [n_mh, n] and the closest call min |u - a|.  The trajectory is the literal safe-mode leapfrog sequence with the
    drift eps p / max(m, 1e-10); every operation rounded on its own in `dtype`."""
    c1, c2, sqrt_temp, beta = ghmc_cases.constants(eps, n_leapfrog, gamma, temp)
    scalar = isinstance(mass, float)
    m_raw, m_sqrt, m_safe = forms(mass, dtype)
    s = c2 * m_sqrt
    eps_t = torch.tensor(float(eps), dtype=dtype)
    x = x0.to(dtype).clone()
    p = ((sqrt_temp * m_sqrt) * xi0.to(dtype)) if p0 is None else p0.to(dtype).clone()
    accepted, margins, kept = [], [], []
    for t in range(z.shape[0]):
        p = c1 * p + s * z[t].to(dtype)  # O
        h0 = _hamiltonian(energy.energy(x), p, m_raw, scalar)
        xp, w = x, p
        for _ in range(n_leapfrog):
            w_half = w + 0.5 * eps_t * _force(energy, xp)
            xp = xp + eps_t * w_half / m_safe
            w = w_half + 0.5 * eps_t * _force(energy, xp)
            xp = xp.nan_to_num_(nan=0.0)
            w = w.nan_to_num_(nan=0.0)
        h1 = _hamiltonian(energy.energy(xp), w, m_raw, scalar)
        a = torch.exp((beta * (h0 - h1)).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
        ut = u[t].to(dtype)
        acc = ut < a
        accepted.append(acc)
        margins.append(torch.where(a == a, (ut - a).abs().double(), torch.full((), float("inf"), dtype=torch.float64)))
        x = torch.where(acc[:, None], xp, x)
        p = torch.where(acc[:, None], w, -p)  # the flip: the negative of the momentum after O
        if (t + 1) % thin == 0:
            kept.append(x.clone())
    n, dim = x0.shape
    return {"x": x, "v": p, "traj": torch.stack(kept, dim=1) if kept else torch.zeros(n, 0, dim, dtype=dtype),
            "accepted": torch.stack(accepted) if accepted else torch.zeros(0, n, dtype=torch.bool),
            "margin": min((m.min().item() for m in margins), default=float("inf"))}


# (kind, dim, n, n_mh, thin, L, mass form): the shapes of ghmc_cases.py thinned in the same way; L = 1 and 3 both with both forms
GHMC_CASES = [
    ("double_well", 2, 257, 4, 2, 1, "scalar"),
    ("double_well", 5, 37, 6, 3, 3, "diag"),
    ("double_well", 12, 9, 1, 1, 1, "diag"),
    ("double_well", 64, 257, 6, 3, 1, "scalar"),
    ("double_well", 100, 9, 6, 3, 3, "diag"),
    ("double_well", 256, 37, 1, 1, 1, "diag"),
    ("harmonic", 5, 257, 1, 1, 3, "scalar"),
    ("harmonic", 32, 257, 6, 3, 3, "diag"),
    ("harmonic", 100, 37, 1, 1, 1, "scalar"),
    ("gaussian", 5, 37, 6, 3, 1, "diag"),
    ("gaussian", 32, 257, 4, 2, 3, "scalar"),
    ("gaussian", 256, 9, 4, 2, 3, "diag"),
    ("gmm", 2, 257, 4, 2, 1, "diag"),
    ("gmm", 100, 37, 4, 2, 1, "scalar"),
    ("rastrigin", 5, 37, 6, 3, 1, "scalar"),
    ("rastrigin", 32, 257, 4, 2, 3, "diag"),
    ("rosenbrock", 12, 37, 4, 2, 1, "diag"),
    ("rosenbrock", 32, 37, 6, 3, 3, "scalar"),
    ("ackley", 100, 37, 1, 1, 3, "diag"),
    ("ackley", 256, 9, 6, 3, 1, "scalar"),
]


def ghmc_step(kind, dim, mass):
    return ghmc_cases.step_size(kind, dim) * math.sqrt(min_mass(mass))


def ghmc_inputs(seed, kind, n, dim, n_mh, mass):
    g = torch.Generator().manual_seed(seed)
    x0 = start_scale(kind) * torch.randn(n, dim, generator=g)
    p0 = start_momentum(mass, torch.randn(n, dim, generator=g))
    return x0, p0, torch.randn(n_mh, n, dim, generator=g), torch.rand(n_mh, n, generator=g)


@functools.lru_cache(maxsize=None)
def ghmc_case(kind, dim, n, n_mh, thin, L, form, gamma=GAMMA, temp=TEMP):
    """Inputs and both restatements of a case.  The seed is the first of SEED_CAP whose fp64 restatement decides nothing within
    MARGIN_BAR of u and whose fp32 restatement decides alike; "found" says whether one was."""
    from helpers import to64

    spec, mass = energy_spec(kind, dim), mass_of(form, dim)
    eps = ghmc_step(kind, dim, mass)
    found = False
    for seed in range(SEED_CAP):
        x0, p0, z, u = ghmc_inputs(7400 + seed, kind, n, dim, n_mh, mass)
        ref64 = restate_ghmc(to64(oracle_of(spec)), x0, p0, z, u, eps, L, gamma, temp, mass, torch.float64, thin)
        if ref64["margin"] <= MARGIN_BAR:
            continue
        ref32 = restate_ghmc(oracle_of(spec), x0, p0, z, u, eps, L, gamma, temp, mass, torch.float32, thin)
        if torch.equal(ref32["accepted"], ref64["accepted"]):
            found = True
            break
    if not found:
        ref32 = restate_ghmc(oracle_of(spec), x0, p0, z, u, eps, L, gamma, temp, mass, torch.float32, thin)
    return {"spec": spec, "mass": mass, "x0": x0, "v0": p0, "z": z, "u": u, "eps": eps, "L": L, "gamma": gamma, "temp": temp,
            "ref32": ref32, "ref64": ref64, "seed": seed, "found": found, "shape": (n, dim), "n_mh": n_mh, "thin": thin}


# ---------------------------------------------------------------------------------
# the laws on a quadratic: the unit-mass laws in the scaled coordinate x sqrt(m)
# ---------------------------------------------------------------------------------
LAW_PRECISION = (0.25, 1.0, 4.0, 16.0)  # k, the diagonal of the Gaussian's precision
LAW_MASS = (1.0, 1.0, 4.0, 4.0)
LAW_STEP, LAW_TEMP, LAW_N, LAW_STEPS, LAW_SEED = 0.6, 0.8, 16384, 400, 0
LAW_GAMMA_BAOAB, LAW_GAMMA_GHMC = 1.5, 1.0


def law_model(device=None):
    import torchebm_amd as ta

    k = torch.tensor(LAW_PRECISION)
    return ta.GaussianModel(torch.zeros(4), torch.diag(1.0 / k), device=device)


def law_start(device=None):
    """x ~ N(0, T / k)."""
    k = torch.tensor(LAW_PRECISION)
    x0 = torch.sqrt(LAW_TEMP / k) * torch.randn(LAW_N, 4, generator=torch.Generator().manual_seed(LAW_SEED))
    return x0 if device is None else x0.to(device)


def check_law(x, p, baoab):
    """Per coordinate: var(x) k / T within law_bar(n) of 1, and var(p) / (T m) within the same bar, relative, of 1 - h^2 k / (4 m)
    under BAOAB and of 1 under generalized HMC.  Prints every figure in front of the assertions."""
    bar = kinetic_cases.law_bar(LAW_N)
    k, m = torch.tensor(LAW_PRECISION, dtype=torch.float64), torch.tensor(LAW_MASS, dtype=torch.float64)
    var_x = x.double().var(dim=0) * k / LAW_TEMP
    var_p = p.double().var(dim=0) / (LAW_TEMP * m)
    want_p = 1.0 - LAW_STEP**2 * k / (4.0 * m) if baoab else torch.ones(4, dtype=torch.float64)
    print(f"var(x) k / T = {var_x.tolist()}, var(p) / (T m) = {var_p.tolist()}, expected {want_p.tolist()}, bar {bar:.4f}")
    assert math.isclose(bar, 0.0497, abs_tol=1e-4)
    assert bool(((var_x - 1.0).abs() < bar).all()), var_x
    assert bool(((var_p / want_p - 1.0).abs() < bar).all()), var_p


# ---------------------------------------------------------------------------------
# the payoff: a badly scaled Gaussian, sigma = (1, 0.1, 0.01)
# ---------------------------------------------------------------------------------
PAYOFF_SIGMA = (1.0, 0.1, 0.01)
PAYOFF_N, PAYOFF_STEPS = 4096, 50


def payoff_model(device=None):
    import torchebm_amd as ta

    return ta.GaussianModel(torch.zeros(3), torch.diag(torch.tensor(PAYOFF_SIGMA) ** 2), device=device)


def payoff_start(seed=0):
    return torch.tensor(PAYOFF_SIGMA) * torch.randn(PAYOFF_N, 3, generator=torch.Generator().manual_seed(seed))


def slow_correlation(x0, x):
    """The correlation of the slow (widest) coordinate with its start."""
    return torch.corrcoef(torch.stack((x0[:, 0].double(), x[:, 0].double())))[0, 1].item()
