r"""Dual-averaging step-size adaptation for :class:`GeneralizedHMC` and :class:`HamiltonianMonteCarlo`
(``sampler.adapt_step_size``): Nesterov dual averaging towards a target acceptance (Hoffman & Gelman 2014, section 3.2), in
the shape Stan uses -- EVERY CHAIN ADAPTS ITS OWN STEP SIZE from its own acceptance probabilities, and the host forms one step
size from the per-chain results afterwards (``pool_step_sizes``: the median of the logs).

Transition ``t`` of a chain whose controller holds ``(eps, Hbar, lbar)`` runs the sampler's transition at ``eps`` (the refresh
constants ``c1 = exp(-gamma L eps)``, ``c2 = sqrt(T (1 - exp(-2 gamma L eps)))`` follow it), takes the acceptance probability
``alpha`` the decision forms (NaN counts as 0), and with row ``t`` of ``da_table``, ``(1 - w, w, s, k, 1 - k)``:

.. math::
    \bar H \leftarrow (1 - w) \bar H + w (\delta - \alpha),\quad
    \log\epsilon = \mathrm{clamp}(\mu - s \bar H),\quad
    \log\bar\epsilon \leftarrow k \log\epsilon + (1 - k) \log\bar\epsilon

The next transition runs at ``exp(log eps)``; behind the last one the chain's step size is the averaged ``exp(log eps-bar)``.

Two routes, chosen once per call (``adapt_route``):

``fused``  CUDA fp32 2-D state, no autocast, an analytic energy (not the MLP), ``dim <= 256``, unit mass, a constant step size,
           no ``model_kwargs`` (and, for ``HamiltonianMonteCarlo``, the plain leapfrog integrator): the whole call is ONE launch of
           ``ebm_ghmc_adapt_chain_f32`` (include/ebm_hip_adapt.h states the recurrence exactly; docs/design/adapt.md the
           kernel).  ``HamiltonianMonteCarlo`` calls the same entry with ``gamma = inf``, ``T = 1``.
``fused_mass``  a sampler built with ``mass=`` under the conditions of ``fused``, and ONLY with the opt-in
           ``sampler.fused_adapt_mass = True``: ONE launch of ``ebm_ghmc_adapt_chain_mass_f32`` (include/ebm_hip_adapt_mass.h;
           docs/design/adapt_mass.md).  The carried plane is then the momentum ``p ~ N(0, T m)``; the mass arguments are
           ``sample()``'s on its ``fused_mass`` route.  Off by default: a massed sampler keeps the eager route and its bits.
``eager``  everything else (the CPU, an ``nn.Module`` or ``MLPEnergy``, a mass without the opt-in, a scheduler, wider rows): the same recurrence in
           torch ops around the safe-mode leapfrog transition of the samplers' eager routes, drawing in ``GeneralizedHMC``'s
           documented order: ``randn(n, dim)`` for the start velocities (only when none are passed), then ``randn(n, dim)`` and
           ``rand(n)`` per transition.

A fused-eligible call never falls back to eager: a missing library or a failing launch raises.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from .. import _lib, _rng
from ..core.energies import fused_spec_for
from ..integrators.symplectic import _mass_args
from ._chain_host import mass_forms, mass_row

ENTRY = "ebm_ghmc_adapt_chain_f32"
ENTRY_MASS = "ebm_ghmc_adapt_chain_mass_f32"
FUSED_MAX_DIM = 256  # one vector per lane (csrc/ghmc_adapt.hip)


def da_table(n_adapt: int, m0: int = 0, t0: float = 10.0, gamma: float = 0.05, kappa: float = 0.75) -> torch.Tensor:
    """The table ``ebm_ghmc_adapt_chain_f32`` reads, ``[n_adapt, 5]`` fp32 on the host: row ``t`` is ``(1 - w, w, s, k, 1 - k)``
    with ``m = m0 + t + 1``, ``w = 1 / (m + t0)``, ``s = sqrt(m) / gamma``, ``k = m^(-kappa)``; each value formed in double and
    rounded once.  ``m0``: the adapting transitions earlier calls made."""
    m = torch.arange(m0 + 1, m0 + n_adapt + 1, dtype=torch.float64)
    w = 1.0 / (m + t0)
    k = m.pow(-kappa)
    return torch.stack((1.0 - w, w, m.sqrt() / gamma, k, 1.0 - k), dim=1).to(torch.float32)


def pool_step_sizes(step_sizes: torch.Tensor) -> torch.Tensor:
    """One step size from the per-chain ones, a 0-dim tensor: ``exp(median(log eps))`` over the chains whose value is finite
    (NaN when there is none).  The median is the robust choice when chains sit in different modes."""
    nan = torch.full((), float("nan"), dtype=step_sizes.dtype, device=step_sizes.device)
    if step_sizes.numel() == 0:
        return nan
    logs = step_sizes.log()
    return torch.nanmedian(torch.where(torch.isfinite(logs), logs, nan)).exp()  # (no host read: nothing is compacted)


@dataclass
class StepSizeAdaptation:
    """What ``adapt_step_size`` returns.

    ``x``, ``velocity``: the chains behind the adaptation (``[n, *shape]``; with a mass ``velocity`` is the momentum plane).
    ``step_sizes``: ``[n]``, every chain's own adapted step size (row 0 of the entry's ``da`` plane).
    ``acceptance``: ``[n]``, every chain's mean acceptance probability while it adapted.
    ``step_size``: 0-dim, ``pool_step_sizes(step_sizes)``.
    ``da``: ``[3, n]``, the controllers ``(eps, Hbar, log eps-bar)`` as the run left them."""

    x: torch.Tensor
    velocity: torch.Tensor
    step_sizes: torch.Tensor
    acceptance: torch.Tensor
    step_size: torch.Tensor
    da: torch.Tensor


def _f32(value: float) -> float:
    return torch.tensor(value, dtype=torch.float64).to(torch.float32).item()


def adapt_route(sampler, x: torch.Tensor, friction: float, model_kwargs=None):
    """``("fused", spec)``, ``("fused_mass", spec)`` or ``("eager", None)``: the sampler's own routing, narrowed to what the
    adapting kernels take.  A massed sampler is fused only with its opt-in ``fused_adapt_mass``."""
    route, spec = sampler._route(x, model_kwargs or {})
    massed = getattr(sampler, "mass", None) is not None
    if route not in ("fused", "fused_mass") or spec is None:  # (GeneralizedHMC names its massed route, HamiltonianMonteCarlo does not)
        return "eager", None
    if massed and not getattr(sampler, "fused_adapt_mass", False):
        return "eager", None
    if spec.kind == _lib.ENERGY_MLP or x.ndim != 2 or x.shape[1] > FUSED_MAX_DIM:
        return "eager", None
    if not sampler.schedulers["step_size"].is_constant():
        return "eager", None
    return ("fused_mass" if massed else "fused"), spec


def eager_adapt(sampler, x, v, n_adapt, n_steps, eps0, friction, temperature, n_leapfrog, target_accept, mu, bounds, table,
                generator, da=None, close=True, model_kwargs=None):
    """The recurrence of include/ebm_hip_adapt.h in torch ops, every operation rounded on its own in ``x``'s dtype: ->
    ``(x, v, da [3, n], alpha_mean [n])``.  ``da`` continues controllers an earlier call left (``None``: a fresh start at
    ``eps0``); ``close=False`` keeps the last iterate instead of the averaged one, so that a later call continues the run."""
    model_kwargs = model_kwargs or {}
    dtype, dev = x.dtype, x.device
    n = x.shape[0]
    mass = getattr(sampler, "mass", None)
    massed, m = mass is not None, mass_row(mass, x)
    if massed:
        m_sqrt, m_safe = mass_forms(mass, x)
    clamped_energy = lambda x_: sampler._model_energy(x_, model_kwargs).clamp_(min=-1e10, max=1e10)  # noqa: E731
    if not massed:
        kinetic = lambda v_: (0.5 * torch.sum(v_.flatten(1).square(), dim=-1)).clamp_(min=0.0, max=1e10)  # noqa: E731
    elif isinstance(m, float):
        kinetic = lambda p_: (0.5 * torch.sum(p_.flatten(1).square(), dim=-1) / m).clamp_(min=0.0, max=1e10)  # noqa: E731
    else:
        kinetic = lambda p_: (0.5 * torch.sum((p_.square() / m).flatten(1), dim=-1)).clamp_(min=0.0, max=1e10)  # noqa: E731
    force = lambda x_: (-sampler._model_gradient(x_, model_kwargs)).clamp_(min=-1e6, max=1e6)  # noqa: E731
    per_chain = lambda t_: t_.view(-1, *([1] * (x.ndim - 1)))  # noqa: E731
    draw_normal = getattr(sampler, "_draw_normal", None) or (lambda shape, like, g: torch.randn(shape, dtype=dtype, device=dev, generator=g))
    draw_uniform = getattr(sampler, "_draw_uniform", None) or (lambda k, like, g: torch.rand(k, dtype=dtype, device=dev, generator=g))

    full = math.isinf(friction)
    gamma_l = 0.0 if full else _f32(friction * n_leapfrog)
    temp, sqrt_temp, beta = _f32(temperature), _f32(math.sqrt(temperature)), _f32(1.0 / temperature)
    delta, mu32 = _f32(target_accept), _f32(mu)
    log_min, log_max = _f32(math.log(bounds[0])), _f32(math.log(bounds[1]))
    rows = table.tolist()
    if v is None:
        z0 = draw_normal(x.shape, x, generator)
        v = (sqrt_temp * m_sqrt) * z0 if massed else sqrt_temp * z0
    if da is None:
        eps = torch.full((n,), _f32(eps0), dtype=dtype, device=dev)
        hbar, lbar = torch.zeros(n, dtype=dtype, device=dev), torch.zeros(n, dtype=dtype, device=dev)
    else:
        eps, hbar, lbar = (row.to(device=dev, dtype=dtype).clone() for row in da)
    alpha_sum = torch.zeros(n, dtype=dtype, device=dev)
    with sampler.autocast_context():
        for t in range(n_steps):
            xi = draw_normal(x.shape, x, generator)
            u = draw_uniform(n, x, generator)
            ec = per_chain(eps)
            if full:
                v = 0.0 * v + (sqrt_temp * m_sqrt if massed else sqrt_temp) * xi
            else:
                span = gamma_l * eps
                c1 = per_chain(torch.exp(-span))
                c2 = per_chain(torch.sqrt(temp * (-torch.expm1(-2.0 * span))))
                v = c1 * v + (c2 * m_sqrt if massed else c2) * xi
            h0 = clamped_energy(x) + kinetic(v)
            xp, vp = x, v
            for _ in range(n_leapfrog):  # the safe-mode leapfrog step of the samplers' eager routes
                v_half = vp + 0.5 * ec * force(xp)
                xp = xp + (ec * v_half / m_safe if massed else ec * v_half)
                vp = v_half + 0.5 * ec * force(xp)
                xp = xp.nan_to_num_(nan=0.0)
                vp = vp.nan_to_num_(nan=0.0)
            h1 = clamped_energy(xp) + kinetic(vp)
            alpha = torch.exp((beta * (h0 - h1)).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
            accepted = u < alpha
            x = torch.where(per_chain(accepted), xp, x)
            v = torch.where(per_chain(accepted), vp, -v)  # the flip
            if t < n_adapt:
                a, b, s, k, k1 = rows[t]
                al = torch.where(alpha == alpha, alpha, torch.zeros_like(alpha))
                alpha_sum = alpha_sum + al
                hbar = a * hbar + b * (delta - al)
                le = (mu32 - s * hbar).clamp_(min=log_min, max=log_max)
                lbar = k * le + k1 * lbar
                eps = torch.exp(lbar if (close and t + 1 == n_adapt) else le)
    if n_steps == 0:  # never the caller's tensors
        x, v = x.clone(), v.clone()
    alpha_mean = alpha_sum / n_adapt if n_adapt > 0 else alpha_sum
    return x, v, torch.stack((eps, hbar, lbar)), alpha_mean


def fused_adapt(sampler, spec, x, v, n_adapt, n_steps, eps0, friction, temperature, n_leapfrog, target_accept, mu, bounds, table,
                generator):
    """ONE launch of ``ebm_ghmc_adapt_chain_f32`` -- of ``ebm_ghmc_adapt_chain_mass_f32`` for a sampler with a mass -- ->
    ``(x, v, da [3, n], alpha_mean [n])``; never the caller's tensors."""
    n, dim = x.shape
    state = _lib.dense_f32(x).clone()  # the kernel updates in place
    draw_v0 = v is None
    vel = torch.empty_like(state) if draw_v0 else _lib.dense_f32(v).clone()
    da = torch.empty(3, n, dtype=torch.float32, device=x.device)
    alpha_mean = torch.zeros(n, dtype=torch.float32, device=x.device)
    table_d = table.to(x.device, non_blocking=True)
    seed, step0 = _rng.reserve(generator, x.device, 2 * n_steps + 1)
    stream = _lib.stream_handle(x.device)
    entry, mass = ENTRY, ()
    if getattr(sampler, "mass", None) is not None:  # (kind, scalar, pointer) directly behind `temperature`, as sample() passes them
        kind, m_scalar, m_diag = _mass_args(sampler.mass, state)
        entry, mass = ENTRY_MASS, (kind, m_scalar, _lib.ptr(m_diag))
    if n > 0 and n_steps > 0:
        _lib.call(
            entry,
            spec.to_c(), _lib.ptr(state), _lib.ptr(vel), n, dim, n_steps, n_leapfrog, eps0, target_accept, mu, bounds[0], bounds[1],
            n_adapt, _lib.DA_INIT, _lib.ptr(da), _lib.ptr(table_d), None, _lib.ptr(alpha_mean), friction, temperature, *mass,
            int(draw_v0), 1, None, None, None, None, seed, step0, stream,
        )
    return state, vel, da, alpha_mean


def adapt_step_size(sampler, friction: float, temperature: float, x=None, dim=None, n_steps: int = 200, n_samples: int = 1,
                    target_accept: float = 0.8, init_step_size: Optional[float] = None, t0: float = 10.0, gamma: float = 0.05,
                    kappa: float = 0.75, mu_factor: float = 10.0, bounds: Tuple[float, float] = (1e-6, 1e3), velocity=None,
                    generator=None, apply: bool = True) -> StepSizeAdaptation:
    """What ``GeneralizedHMC.adapt_step_size`` and ``HamiltonianMonteCarlo.adapt_step_size`` run (their docstrings)."""
    if int(n_steps) != n_steps or n_steps < 1:
        raise ValueError("n_steps must be an integer >= 1")
    if not 0.0 < target_accept < 1.0:
        raise ValueError("target_accept must lie in (0, 1)")
    eps0 = float(sampler.get_scheduled_value("step_size") if init_step_size is None else init_step_size)
    if not (eps0 > 0 and math.isfinite(eps0)):
        raise ValueError("init_step_size must be positive and finite")
    if not (t0 >= 0 and gamma > 0 and kappa > 0 and mu_factor > 0 and math.isfinite(t0 + gamma + kappa + mu_factor)):
        raise ValueError("t0 must be >= 0, gamma, kappa and mu_factor positive, all finite")
    lo, hi = (float(b) for b in bounds)
    if not (0 < lo <= hi and math.isfinite(hi)):
        raise ValueError("bounds must be positive and finite, bounds[0] <= bounds[1]")
    n_steps = int(n_steps)
    with torch.no_grad():
        x = sampler._init_state(x, dim, n_samples, generator)
        if velocity is not None:
            if tuple(velocity.shape) != tuple(x.shape):
                raise ValueError(f"velocity must have the state's shape {tuple(x.shape)}, got {tuple(velocity.shape)}")
            velocity = velocity.to(device=sampler.device, dtype=sampler.dtype)
        mass_row(getattr(sampler, "mass", None), x)  # (a mass of another length raises here, in front of any work)
        mu = math.log(mu_factor * eps0)
        table = da_table(n_steps, 0, t0, gamma, kappa)
        route, spec = adapt_route(sampler, x, friction)
        n_leapfrog = int(sampler.n_leapfrog_steps)
        run = (lambda *a: fused_adapt(sampler, spec, *a)) if route != "eager" else (lambda *a: eager_adapt(sampler, *a))
        state, vel, da, alpha_mean = run(x, velocity, n_steps, n_steps, eps0, friction, temperature, n_leapfrog, target_accept, mu,
                                         (lo, hi), table, generator)
        result = StepSizeAdaptation(state, vel, da[0], alpha_mean, pool_step_sizes(da[0]), da)
    if apply:  # one host read
        value = float(result.step_size)
        if not (value > 0 and math.isfinite(value)):
            raise RuntimeError("adapt_step_size: no chain ended on a finite step size")
        sampler._register_param("step_size", value, positive=True)
    return result
