"""The step-route entries (include/ebm_hip.h: ebm_langevin_step_f32, ebm_langevin_step_diffusion_f32, the leapfrog sub-steps,
ebm_hmc_accept_f32, ebm_descent_step_f32, ebm_lookahead_f32) restated from the header's formulas in plain torch ops on the CPU,
one op per rounded operation, and the inputs the tests run them on.  Shared by test_step_bars.py (CPU tier) and
test_step_kernels_gpu.py; it never calls the package.

Scalars reach the kernels as C floats, so every scalar here is rounded to fp32 first (`s32`).  Separate torch CPU ops do not
contract; where the kernel fuses (descent, lookahead) the product is formed exactly in float64, added there and rounded once."""

import functools
import math

import torch

F32 = torch.float32
MASS_NONE, MASS_SCALAR, MASS_DIAG = 0, 1, 2

# the sizes of the element-wise entries: one lane, a ragged float4 group, one whole group, a group and a tail, the block edge
SMALL = (1, 2, 3, 4, 5, 1023, 1024, 1025)
GRID_LANES = 2048 * 256  # every launcher caps its grid here and strides beyond it
BIG_ELEM = GRID_LANES + 259  # one lane per element: kick, descent, lookahead
BIG_GROUPS = (4 * GRID_LANES + 1028, 4 * GRID_LANES + 1031)  # one lane per float4 group: the wide kernel, the plain one
BIG_KICK_DRIFT = ((174849, 3), (131137, 4))
ACCEPT_CHAINS = (1, 63, 64, 65, 255, 256, 257, 1000)
ACCEPT_DIMS = (1, 3, 8, 1030)
ACCEPT_BIG = ((BIG_ELEM, 1), (BIG_ELEM, 3))


def s32(v):
    """The fp32 value of a Python number, as a 0-dim fp32 tensor."""
    return torch.tensor(float(v), dtype=torch.float64).to(F32)


def same_bits(a, b):
    """torch.equal on the bit patterns (so -0.0 is not 0.0), with every NaN counted as one value: which NaN an operation
    makes (sign, payload) is the processor's choice, not the kernel's."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    a, b = a.detach().cpu(), b.detach().cpu()
    inf = float("inf")
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(
        torch.nan_to_num(a, nan=0.0, posinf=inf, neginf=-inf).view(torch.int32),
        torch.nan_to_num(b, nan=0.0, posinf=inf, neginf=-inf).view(torch.int32))


def share_differing(a, b):
    """Share of elements whose bits differ (NaNs as in same_bits)."""
    inf = float("inf")
    d = torch.nan_to_num(a, nan=0.0, posinf=inf, neginf=-inf).view(torch.int32) != torch.nan_to_num(
        b, nan=0.0, posinf=inf, neginf=-inf).view(torch.int32)
    d |= torch.isnan(a) != torch.isnan(b)
    return d.double().mean().item()


# ---------------------------------------------------------------------------------
# Langevin step
# ---------------------------------------------------------------------------------
def langevin_step(x, grad, noise, eta, sqrt_eta, noise_coef, clamp=None, fused_drift=False):
    """x1 = x - eta g;  dw = eps sqrt_eta;  out = x1 + noise_coef dw;  clamp.  noise_coef == 0: no draw, nothing added.
    grad None: a zero gradient.  `fused_drift`: the WRONG variant with x - eta g contracted into one rounding."""
    g = torch.zeros_like(x) if grad is None else grad
    if fused_drift:
        out = (x.double() - s32(eta).double() * g.double()).to(F32)
    else:
        out = x - s32(eta) * g
    if s32(noise_coef).item() != 0.0:
        dw = noise * s32(sqrt_eta)
        out = out + s32(noise_coef) * dw
    if clamp is not None:
        out = torch.clamp(out, min=s32(clamp[0]).item(), max=s32(clamp[1]).item())  # propagates NaN
    return out


def diffusion_coef(diffusion, period, n_elem, split_sqrt=False):
    """sqrt(fl32(2 D_e)), D_e = diffusion[e % period], correctly rounded (float64 square root of the fp32 product, rounded once:
    innocuous for a square root).  `split_sqrt`: the WRONG variant sqrt(2) sqrt(D)."""
    d = diffusion.reshape(-1)[torch.arange(n_elem) % period]
    if split_sqrt:
        return s32(math.sqrt(2.0)) * torch.sqrt(d.double()).to(F32)
    return torch.sqrt((2.0 * d).double()).to(F32)


def diffusion_field(period):
    """A diffusion tensor of `period` positive values, one of them 0 (where there is more than one)."""
    d = 0.1 + torch.rand(period, generator=torch.Generator().manual_seed(9402 + period))
    if period > 1:
        d[period // 2] = 0.0
    return d


def diffusion_step(x, grad, noise, diffusion, period, eta, sqrt_eta, split_sqrt=False):
    g = torch.zeros_like(x) if grad is None else grad
    x1 = x - s32(eta) * g
    dw = noise * s32(sqrt_eta)
    return x1 + diffusion_coef(diffusion, period, x.numel(), split_sqrt).view(x.shape) * dw


# ---------------------------------------------------------------------------------
# leapfrog sub-steps
# ---------------------------------------------------------------------------------
def _clamp_force(force, safe, drop_nan=False):
    if not safe:
        return force
    if drop_nan:  # the WRONG variant: fminf(fmaxf(f, -1e6), 1e6) swallows a NaN
        return torch.fmin(torch.fmax(force, s32(-1e6)), s32(1e6))
    return torch.clamp(force, min=-1e6, max=1e6)


def kick_drift(x, p, force, eps, mass_kind=MASS_NONE, mass_scalar=0.0, mass_diag=None, safe=False, variant=None):
    """x, p, force [n, dim] -> (x_new, p_half).  f = clamp(force) if safe;  p_half = p + (0.5 eps) f;
    x_new = x + eps p_half  or  x + (eps p_half) / max(m, 1e-10).
    WRONG variants: "half_last" 0.5 (eps f), "hoisted" x + (eps / m) p_half, "drop_nan" a clamp that swallows NaN."""
    e = s32(eps)
    f = _clamp_force(force, safe, drop_nan=variant == "drop_nan")
    if variant == "half_last":
        ph = p + s32(0.5) * (e * f)
    else:
        ph = p + (s32(0.5) * e) * f
    if mass_kind == MASS_NONE:
        return x + e * ph, ph
    if mass_kind == MASS_SCALAR:
        m = s32(max(float(mass_scalar), 1e-10))  # formed in double, rounded once
    else:
        m = torch.clamp(mass_diag, min=1e-10).view(1, -1)  # per element; a NaN mass stays NaN
    if variant == "hoisted":
        return x + (e / m) * ph, ph
    return x + (e * ph) / m, ph


def kick(x_new, p_half, force, eps, safe=False, variant=None):
    """-> (x_new, p_new).  f = clamp(force) if safe;  p_new = p_half + (0.5 eps) f;  if safe: nan_to_num(nan=0) on both."""
    f = _clamp_force(force, safe, drop_nan=variant == "drop_nan")
    pn = p_half + (s32(0.5) * s32(eps)) * f
    if safe:
        return torch.nan_to_num(x_new, nan=0.0), torch.nan_to_num(pn, nan=0.0)
    return x_new.clone(), pn


def leapfrog_once(energy, x, p, eps, mass_kind, mass_scalar, mass_diag, safe, kd=kick_drift, kk=kick):
    """kick-drift, then kick, the force from the oracle energy: one step of oracle.hmc.leapfrog out of the two sub-steps
    (`kd`, `kk`: the restatements, or the kernels behind the same signatures)."""
    xn, ph = kd(x, p, -energy.grad(x), eps, mass_kind, mass_scalar, mass_diag, safe)
    return kk(xn, ph, -energy.grad(xn), eps, safe)


def oracle_mass(mass_kind, mass_scalar, mass_diag):
    return None if mass_kind == MASS_NONE else (float(mass_scalar) if mass_kind == MASS_SCALAR else mass_diag)


# ---------------------------------------------------------------------------------
# descent step and lookahead: FMAs
# ---------------------------------------------------------------------------------
def fma_ref(a, b, c):
    """fma(a, b, c) of fp32 operands: the product is exact in float64, the sum rounds there and once more to fp32.  Equal to a
    true FMA unless the float64 sum sits within one float64 ulp of an fp32 rounding midpoint (fma_midpoint_risk)."""
    return (a.double() * b.double() + c.double()).to(F32)


def fma_midpoint_risk(a, b, c):
    """bool per element: the float64 sum is within one float64 ulp of the midpoint between two neighbouring fp32 values."""
    s = a.double() * b.double() + c.double()
    r = s.to(F32)
    ulp64 = (torch.nextafter(s.abs(), torch.full_like(s, float("inf"))) - s.abs())
    risk = torch.zeros_like(s, dtype=torch.bool)
    for toward in (float("inf"), -float("inf")):
        nb = torch.nextafter(r, torch.full_like(r, toward))
        mid = (r.double() + nb.double()) / 2.0
        risk |= (s - mid).abs() <= ulp64
    return risk & torch.isfinite(s)


def descent_step(x, grad, v, eta, mu, unfused=False):
    """-> (out, v_new).  v None: out = fma(-eta, g, x).  Else v_new = fma(-eta, g, fl32(v mu)), out = x + v_new.
    `unfused`: the WRONG variant, multiply then add."""
    neg_eta = -s32(eta)
    if v is None:
        return (x + neg_eta * grad if unfused else fma_ref(neg_eta, grad, x)), None
    vm = v * s32(mu)
    vn = vm + neg_eta * grad if unfused else fma_ref(neg_eta, grad, vm)
    return x + vn, vn


def lookahead(x, v, mu, unfused=False):
    return x + s32(mu) * v if unfused else fma_ref(s32(mu), v, x)


# ---------------------------------------------------------------------------------
# Metropolis accept
# ---------------------------------------------------------------------------------
ACCEPT_ULPS = 1024  # |u - a64| >= 1024 ulp32(a64), or a64 == 1: three orders of magnitude above any plausible expf error


def accept_ref(h0, h1, u, clamp_at=50.0, strict=True):
    """-> (decision bool [n], a64).  d = clamp(fl32(h0 - h1), -50, 50), a64 = min(1, exp(d)) in float64, u < a64.  A NaN d
    (NaN Hamiltonian, inf - inf) makes a64 NaN and rejects.  WRONG variants: clamp_at=88, strict=False (u <= a)."""
    d = torch.clamp(h0 - h1, min=-clamp_at, max=clamp_at)
    a64 = torch.exp(d.double()).clamp(max=1.0)
    return (u.double() < a64) if strict else (u.double() <= a64), a64


def ulp32(a64):
    a = a64.to(F32)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))).double() - a.double()).abs()


def accept_margin_ok(u, a64):
    """bool per chain: the decision does not depend on the device's expf."""
    return (a64 == 1.0) | ((u.double() - a64).abs() >= ACCEPT_ULPS * ulp32(a64))


def hamiltonians_from_u(u):
    """h1 = 0 and h0 = fl32(log(1.25 u)) (even chains: accepted) or fl32(log(0.75 u)) (odd chains: rejected): a = e^{h0} sits
    25 % off u, whatever expf the decision is taken with."""
    n = u.numel()
    factor = torch.where(torch.arange(n) % 2 == 0, 1.25, 0.75).double()
    return torch.log(u.double() * factor).to(F32), torch.zeros(n)


_NAN, _INF = float("nan"), float("inf")
# (h0, h1, u or None: any u < 1, the decision)
EDGE_ROWS = (
    (3.5, 3.5, 1.0 - 2.0**-24, True),    # h0 == h1 accepts for any u < 1
    (1.0, 0.0, 1.0, False),              # an injected u = 1.0 rejects even at a = 1: the comparison is strict
    (1e30, 0.0, None, True),             # h0 - h1 = +1e30 accepts
    (-1e30, 0.0, 1e-20, False),          # the clamp at -50: a = e^-50 = 1.9e-22
    (-1e30, 0.0, 0.0, True),             # ... which u = 0 is still below
    (-1e30, 0.0, 1e-30, True),           # ... and so is 1e-30 (a clamp at -88 would put a = 6e-39 below it)
    (_NAN, 0.0, None, False),
    (0.0, _NAN, None, False),
    (_INF, _INF, None, False),           # inf - inf
)


def edge_positions(n):
    """{chain: edge row}: the rows in the first tile, a middle tile and the last tile of 256 chains (those that fit)."""
    k, pos = len(EDGE_ROWS), {}
    mid = (n // 512) * 256 + 100
    for start in (0, mid, n - k):
        for j in range(k):
            if 0 <= start + j < n:
                pos[start + j] = j
    return pos


def apply_edges(h0, h1, u, fixed_u=False):
    """Overwrite the edge chains in place.  `fixed_u`: u is the kernel's own field -- only the rows that decide for any u."""
    for c, j in edge_positions(h0.numel()).items():
        e0, e1, eu, _ = EDGE_ROWS[j]
        if fixed_u and eu is not None:
            continue
        h0[c], h1[c] = e0, e1
        if eu is not None:
            u[c] = eu
    return h0, h1, u


@functools.lru_cache(maxsize=None)
def accept_case(n, dim):
    """Injected-u inputs and the expected decisions of a shape; x holds a NaN coordinate in a rejected chain."""
    g = torch.Generator().manual_seed(9100 + 7 * n + dim)
    u = torch.rand(n, generator=g)
    h0, h1 = hamiltonians_from_u(u)
    apply_edges(h0, h1, u)
    x = torch.randn(n, dim, generator=g)
    x_prop = torch.randn(n, dim, generator=g)
    acc, a64 = accept_ref(h0, h1, u)
    rejected = (~acc).nonzero().flatten()
    if rejected.numel():
        x[rejected[0], dim // 2] = _NAN
    return {"h0": h0, "h1": h1, "u": u, "x": x, "x_prop": x_prop, "acc": acc, "a64": a64,
            "x_out": torch.where(acc.view(-1, 1), x_prop, x)}


def accept_shapes():
    return [(n, d) for n in ACCEPT_CHAINS for d in ACCEPT_DIMS] + list(ACCEPT_BIG)


# ---------------------------------------------------------------------------------
# inputs of the element-wise entries
# ---------------------------------------------------------------------------------
ETA, SQRT_ETA, NOISE_COEF = 0.013, math.sqrt(0.013), math.sqrt(2.0 * 0.7**2)
CLAMP = (-1.25, 0.75)
EPS = 1.25       # leapfrog step: above 1, so that 0.5 (eps f) overflows at f = 3e38 where (0.5 eps) f does not
DESCENT_ETA, MOMENTUM = 0.037, 0.9
FORCE_SPECIALS = (_NAN, _INF, -_INF, 1e7, -1e7)


@functools.lru_cache(maxsize=None)
def elem_case(n):
    """x, grad, noise, v of n elements.  (The seeds of this file are the first that meet every condition test_step_bars.py puts
    on the inputs: base 9000 put an FMA operand of the descent step on an fp32 midpoint at 524 547 elements.)"""
    g = torch.Generator().manual_seed(9190 + n)
    return {"x": torch.randn(n, generator=g), "grad": 3.0 * torch.randn(n, generator=g), "noise": torch.randn(n, generator=g),
            "v": 0.5 * torch.randn(n, generator=g)}


def diag_mass(dim):
    """A diagonal mass with 0, -1, 1e-12 and NaN in front (as many as fit beside one clean entry)."""
    m = 0.5 + torch.rand(dim, generator=torch.Generator().manual_seed(9200 + dim))
    special = torch.tensor([0.0, -1.0, 1e-12, _NAN])
    k = min(4, dim - 1)
    m[:k] = special[:k]
    return m


@functools.lru_cache(maxsize=None)
def kick_case(n_chains, dim, wild):
    """x, p, force [n_chains, dim]; `wild`: NaN, +-inf, +-1e7 and 3e38 among the forces (spread over the tensor) and NaN / +-inf in
    x (what the safe kick scrubs)."""
    g = torch.Generator().manual_seed(9300 + 3 * n_chains + dim)
    x = torch.randn(n_chains, dim, generator=g)
    p = torch.randn(n_chains, dim, generator=g)
    force = 4.0 * torch.randn(n_chains, dim, generator=g)
    n = n_chains * dim
    if wild:
        vals = FORCE_SPECIALS + (3e38,)
        for j, val in enumerate(vals):
            force.view(-1)[(j * (n - 1)) // len(vals)] = val
        for j, val in enumerate((_NAN, _INF, -_INF)):
            x.view(-1)[(n - 1) - (j * (n - 1)) // 4] = val
    return {"x": x, "p": p, "force": force}


MASS_FORMS = (("none", MASS_NONE, 0.0), ("scalar", MASS_SCALAR, 2.5), ("tiny", MASS_SCALAR, 1e-12), ("diag", MASS_DIAG, 0.0))
