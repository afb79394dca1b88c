r"""Generalized HMC (Horowitz 1991), the Metropolis-adjusted kinetic Langevin sampler: :class:`GeneralizedHMC`.

A chain carries a velocity ``v`` beside its position ``x`` (unit mass, friction ``gamma``, temperature ``T``: the target is
``exp(-E / T)``).  One transition with step ``eps`` and ``L`` leapfrog steps:

.. math::
    v \leftarrow e^{-\gamma \epsilon L} v + \sqrt{T (1 - e^{-2 \gamma \epsilon L})}\,\xi,\quad
    (x', v') = \mathrm{leapfrog}^L_\epsilon(x, v),\quad
    a = \min(1, e^{(H(x, v) - H(x', v')) / T}),\quad
    (x, v) \leftarrow (x', v') \text{ with probability } a, \text{ else } (x, -v)

The partial refresh keeps ``N(0, T)``, the trajectory with its Metropolis decision and the flip keeps ``exp(-H / T)``: the
chain samples ``exp(-E / T)`` exactly for every step size, as ``HamiltonianMonteCarlo`` does (``friction=inf`` IS that
sampler's transition), and with weak friction it keeps its direction across transitions, as ``UnderdampedLangevin`` does --
which is unadjusted and leaves a step-size bias.

Three execution routes, chosen once per ``sample()`` call (``_route``):

``fused``  CUDA fp32 2-D state, no autocast, one of the analytic energies (not the MLP), ``dim <= 256`` and a constant step size:
           the whole call -- start velocities, refreshes, trajectories, decisions, Philox draws, thinned trajectory, accept mask
           -- is ONE launch of ``ebm_ghmc_chain_f32`` (include/ebm_hip.h states the recurrence exactly; docs/design/ghmc.md
           the kernel).
``fused_mlp``  the same state and step size on an ``MLPEnergy`` of hidden width 64 / 128 and ``in_dim <= 128``, and ONLY with the
           opt-in ``sampler.fused_mlp = True``: ONE launch of ``ebm_ghmc_mlp_chain_f32`` (docs/design/ghmc_mlp.md) -- the same
           recurrence, the same Philox coordinates, the matrix-core evaluation inside the trajectory; fp32 accuracy, not
           autograd's rounding.  Off by default: a default sampler on an MLP keeps its eager bits.
``eager``  everything else (CPU, any other ``BaseModel``, a scheduler on ``step_size``, wider rows): the same recurrence in
           torch ops around ``model`` / ``model.gradient`` with the clamps of ``HamiltonianMonteCarlo``'s eager transition,
           drawing ``randn(n, dim)`` for the start velocities (only when none are passed) and ``randn(n, dim)``, ``rand(n)``
           per transition.

``fused_mass``  a sampler built with ``mass=`` (a float or a per-dimension tensor) under the conditions of ``fused``: ONE launch
           of ``ebm_ghmc_chain_mass_f32`` (docs/design/mass.md).  The carried plane is then the MOMENTUM ``p ~ N(0, T m)``:
           ``velocity=`` / ``return_velocity`` carry it; the refresh is ``p = c1 p + c2 sqrt(m) xi``, the kinetic energy
           ``p^2 / (2 m)`` and the drift ``x += eps p / m``, as ``HamiltonianMonteCarlo(mass=...)`` has them (``friction=inf``
           is that sampler's transition with the same mass).  With a mass an ``MLPEnergy`` takes ``eager`` unless both opt-ins below are set.
``fused_mlp_mass``  opt-in twice (``sampler.fused_mlp = True`` and ``sampler.fused_mlp_mass = True``): a sampler built with
           ``mass=`` under the conditions of ``fused_mlp``: ONE launch of ``ebm_ghmc_mlp_chain_mass_f32``
           (docs/design/mass_mlp.md), the momentum plane and the Philox steps as on ``fused_mass`` / ``fused_mlp``.

A fused-eligible call never falls back to eager: a missing library or a failing launch raises.
"""

from __future__ import annotations

import math
from typing import Any, Dict, Optional, Tuple, Union

import torch

from .. import _lib, _rng
from ..core.energies import BaseModel, FusedSpec, fused_spec_for
from ..core.sampler_base import BaseSampler
from ..core.schedules import BaseScheduler
from ..integrators.symplectic import _mass_args
from ._chain_host import (FUSED_MLP_MAX_DIM, check_mass, fused_mlp_walk_fits, kept_statistics,  # noqa: F401
                          kinetic_temperature, mass_forms, mass_row, new_outputs,
                          record_kept)  # (FUSED_MLP_MAX_DIM: importable from here as before)

FUSED_MAX_DIM = 256  # one vector per lane (csrc/ghmc.hip)


def ghmc_constants(eps: float, n_leapfrog: int, friction: float, temperature: float,
                   dtype: torch.dtype = torch.float32) -> Tuple[float, float, float, float]:
    """``(exp(-gamma eps L), sqrt(T (1 - exp(-2 gamma eps L))), sqrt(T), 1 / T)``: formed in double, each rounded once to
    ``dtype`` (the constants ``ebm_ghmc_chain_f32`` forms from the same numbers); ``friction=inf`` gives ``c1 = 0`` and
    ``c2 = sqrt(T)`` exactly."""
    sqrt_temp = math.sqrt(temperature)
    if math.isinf(friction):
        c1, c2 = 0.0, sqrt_temp
    else:
        span = friction * eps * n_leapfrog
        c1, c2 = math.exp(-span), math.sqrt(temperature * (-math.expm1(-2.0 * span)))
    return tuple(torch.tensor((c1, c2, sqrt_temp, 1.0 / temperature), dtype=torch.float64).to(dtype).tolist())


class GeneralizedHMC(BaseSampler):
    """Generalized HMC: partial momentum refresh, a Metropolis-corrected leapfrog trajectory, a momentum flip on a reject.

    Args:
        model: energy model to sample from.
        step_size: leapfrog step ``eps``, a float or (eager route) a ``BaseScheduler``.
        n_leapfrog_steps: leapfrog steps ``L >= 1`` per transition.
        friction: friction ``gamma > 0``; the velocity keeps ``exp(-gamma eps L)`` of itself per transition, ``inf`` is HMC.
        temperature: temperature ``T > 0``; the chains sample ``exp(-E / T)``.
        dtype, device: where the chains live.
        mass: ``None`` (unit mass), a positive finite float, or a 1-D tensor of per-dimension masses (moved to the sampler's
            device; its entries are not inspected).  With a mass the carried plane is the momentum ``p ~ N(0, T m)``.

    ``fused_mlp`` (class attribute, ``False``): set it on a sampler to send an eligible ``MLPEnergy`` call to the one-launch
    route ``fused_mlp`` (module docstring).
    """

    fused_mlp = False
    #: second opt-in, read by ``sample_moments`` only: with ``fused_mlp`` set too, an eligible ``MLPEnergy`` call of
    #: ``sample_moments`` is ONE launch of ``ebm_kinetic_moments_mlp_f32`` (docs/design/kinetic_moments_mlp.md).  Off by default: with
    #: ``fused_mlp`` alone ``sample_moments`` keeps the step-by-step recurrence and autograd's energies.
    fused_mlp_moments = False
    #: third opt-in, read by ``sample`` of a sampler built with ``mass=``: with ``fused_mlp`` set too, an eligible ``MLPEnergy`` call
    #: is ONE launch of ``ebm_ghmc_mlp_chain_mass_f32`` (docs/design/mass_mlp.md).  Off by default: with ``fused_mlp`` alone a
    #: massed sampler on an ``MLPEnergy`` keeps the eager route and its bits.
    fused_mlp_mass = False
    #: opt-in read by ``adapt_step_size`` of a sampler built with ``mass=``: an eligible call (the conditions of ``fused_mass``) is
    #: ONE launch of ``ebm_ghmc_adapt_chain_mass_f32`` (docs/design/adapt_mass.md).  Off by default: a massed sampler's
    #: ``adapt_step_size`` keeps the eager route and its bits.  (``warmup()`` is new and takes the launch without it.)
    fused_adapt_mass = False

    def __init__(
        self,
        model: BaseModel,
        step_size: Union[float, BaseScheduler] = 1e-2,
        n_leapfrog_steps: int = 1,
        friction: float = 1.0,
        temperature: float = 1.0,
        dtype: torch.dtype = torch.float32,
        device: Optional[Union[str, torch.device]] = None,
        mass: Optional[Union[float, torch.Tensor]] = None,
    ):
        super().__init__(model=model, dtype=dtype, device=device)
        self._register_param("step_size", step_size, positive=True)
        self.mass = check_mass(mass, self.device)
        if int(n_leapfrog_steps) != n_leapfrog_steps or n_leapfrog_steps < 1:
            raise ValueError("n_leapfrog_steps must be an integer >= 1")
        if not friction > 0:  # (inf is allowed: a full refresh)
            raise ValueError("friction must be positive")
        if not (temperature > 0 and math.isfinite(temperature)):
            raise ValueError("temperature must be positive")
        self.n_leapfrog_steps = int(n_leapfrog_steps)
        self.friction = float(friction)
        self.temperature = float(temperature)

    # ---------------------------------------------------------------------------------
    # routing: decided here and nowhere else
    # ---------------------------------------------------------------------------------
    def _route(self, x: torch.Tensor, model_kwargs=None) -> Tuple[str, Optional[FusedSpec]]:
        if model_kwargs or not x.is_cuda or x.dtype != torch.float32 or x.ndim != 2:
            return "eager", None
        if not self.schedulers["step_size"].is_constant():
            return "eager", None
        if self.use_mixed_precision and self.autocast_available:
            return "eager", None
        spec = fused_spec_for(self.model, x, None)
        if spec is None or x.shape[1] > FUSED_MAX_DIM:
            return "eager", None
        if spec.kind == _lib.ENERGY_MLP:
            fits = self.fused_mlp and fused_mlp_walk_fits(spec.n_comp, getattr(self.model, "in_dim", None), x.shape[1])
            if self.mass is not None:  # (a second opt-in: with fused_mlp alone a massed MLP sampler stays eager)
                return ("fused_mlp_mass", spec) if fits and self.fused_mlp_mass else ("eager", None)
            return ("fused_mlp", spec) if fits else ("eager", None)
        return ("fused" if self.mass is None else "fused_mass"), spec

    # ---------------------------------------------------------------------------------
    # public API
    # ---------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(
        self,
        x: Optional[torch.Tensor] = None,
        dim: Optional[Union[int, Tuple[int, ...]]] = None,
        n_steps: int = 100,
        n_samples: int = 1,
        thin: int = 1,
        return_trajectory: bool = False,
        return_diagnostics: bool = False,
        reset_schedulers: bool = True,
        *,
        velocity: Optional[torch.Tensor] = None,
        return_velocity: bool = False,
        model_kwargs: Optional[Dict[str, Any]] = None,
        generator: Optional[torch.Generator] = None,
    ):
        """Run ``n_steps`` transitions.

        ``model_kwargs``: conditioning passed to the model at every evaluation; a non-empty dict takes the eager route.

        ``velocity``: the start velocities, shaped as ``x`` (as a call with ``return_velocity=True`` returned them: continue
        that run); ``None`` draws them from ``N(0, T I)``.  A sampler with a ``mass`` carries the momentum in this plane
        (``N(0, T m)``), here and in ``return_velocity``.

        Returns the final positions ``[n, *shape]`` (or, with ``return_trajectory``, the kept positions
        ``[n, n_steps // thin, *shape]``); with ``return_diagnostics`` a dict follows, holding ``"mean"`` / ``"var"``
        (``[n_kept, *shape]``, biased variance clamped to [1e-10, 1e10]), ``"energy"`` and ``"acceptance_rate"``
        (``[n_kept]``: the accepted share of each kept transition) of the kept positions and ``"kinetic_temperature"``, the
        mean of ``v^2`` (with a mass: of ``p^2 / m``) over chains and coordinates of the final velocities (``T`` in law); with ``return_velocity`` the final
        velocities come last.  The caller's ``x`` and ``velocity`` are never written.

        Raises:
            ValueError: ``thin < 1``, ``x`` and ``dim`` both ``None``, a ``velocity`` whose shape differs from the state's, or a
                ``mass`` tensor whose length is not the state's last width.
        """
        if thin < 1:
            raise ValueError("thin must be >= 1")
        if reset_schedulers:
            self.reset_schedulers()
        x = self._init_state(x, dim, n_samples, generator)
        if velocity is not None:
            if tuple(velocity.shape) != tuple(x.shape):
                raise ValueError(f"velocity must have the state's shape {tuple(x.shape)}, got {tuple(velocity.shape)}")
            velocity = velocity.to(device=self.device, dtype=self.dtype)
        model_kwargs = self._prepare_model_kwargs(model_kwargs)
        m = mass_row(self.mass, x)
        route, spec = self._route(x, model_kwargs)
        if route == "fused":
            state, v, traj, diag = self._sample_fused(x, velocity, spec, n_steps, thin, return_trajectory, return_diagnostics, generator)
        elif route == "fused_mass":
            state, v, traj, diag = self._sample_fused(x, velocity, spec, n_steps, thin, return_trajectory, return_diagnostics, generator,
                                                      entry="ebm_ghmc_chain_mass_f32")
        elif route == "fused_mlp":
            state, v, traj, diag = self._sample_fused(x, velocity, spec, n_steps, thin, return_trajectory, return_diagnostics, generator,
                                                      entry="ebm_ghmc_mlp_chain_f32")
        elif route == "fused_mlp_mass":
            state, v, traj, diag = self._sample_fused(x, velocity, spec, n_steps, thin, return_trajectory, return_diagnostics, generator,
                                                      entry="ebm_ghmc_mlp_chain_mass_f32")
        else:
            state, v, traj, diag = self._sample_eager(x, velocity, n_steps, thin, return_trajectory, return_diagnostics, generator,
                                                      model_kwargs)
        out = (traj if return_trajectory else state,)
        if return_diagnostics:
            diag["kinetic_temperature"] = kinetic_temperature(v, m)
            out += (diag,)
        if return_velocity:
            out += (v,)
        return out[0] if len(out) == 1 else out

    def sample_moments(
        self,
        x: Optional[torch.Tensor] = None,
        dim: Optional[Union[int, Tuple[int, ...]]] = None,
        n_steps: int = 100,
        n_samples: int = 1,
        burn_in: int = 0,
        energy: bool = False,
        *,
        velocity: Optional[torch.Tensor] = None,
        return_velocity: bool = False,
        generator: Optional[torch.Generator] = None,
    ):
        """Run ``n_steps`` transitions and keep per-chain running moments of the held positions after the first ``burn_in``
        (with ``energy`` of their energies too; a reject counts the held state again) -- no trajectory is written.

        Returns ``(x_final, ChainMoments)``, with ``return_velocity`` ``(x_final, ChainMoments, v_final)``.  The moments
        carry ``rhat``, ``ess``, ``mean``, ``var`` and ``acceptance_rate`` (``[n_steps]``).  When ``n_steps - burn_in`` is
        odd one more transition is burnt.  On the fused route (see the module docstring) the call is ONE launch of
        ``ebm_kinetic_moments_f32`` and ``x_final``, ``v_final`` are ``sample(return_velocity=True)``'s for the same
        generator state.  On an eligible ``MLPEnergy`` with both opt-ins, ``fused_mlp`` and ``fused_mlp_moments``, it is ONE
        launch of ``ebm_kinetic_moments_mlp_f32`` and matches ``sample()`` under ``fused_mlp`` in the same way (``friction =
        inf``: plain HMC); with ``fused_mlp`` alone it stays step by step.  The caller's ``x`` and ``velocity`` are never written.

        Raises:
            ValueError: fewer than 4 counted steps, ``burn_in`` outside ``0 .. n_steps``, a ``velocity`` of another shape.
        """
        from .kinetic_moments import sample_moments

        return sample_moments(self, True, x, dim, n_steps, n_samples, burn_in, energy, velocity, return_velocity, generator)

    def adapt_step_size(self, x=None, dim=None, n_steps=200, n_samples=1, target_accept=0.8, init_step_size=None, t0=10.0, gamma=0.05,
                        kappa=0.75, mu_factor=10.0, bounds=(1e-6, 1e3), velocity=None, generator=None, apply=True):
        """Find the leapfrog step size by dual averaging (Hoffman & Gelman 2014, section 3.2; ``samplers/adapt.py``): run
        ``n_steps`` transitions in which EVERY CHAIN ADAPTS ITS OWN STEP SIZE towards the acceptance ``target_accept``, then pool.

        ``init_step_size``: where every chain starts (``None``: the sampler's current step size); the iterates shrink towards
        ``mu = log(mu_factor * init_step_size)``.  ``t0``, ``gamma``, ``kappa``: the dual-averaging constants (the defaults are
        Stan's).  ``bounds``: every step size stays inside.  ``velocity``: the start velocities, as in ``sample``.

        Returns a :class:`StepSizeAdaptation`: the chains behind the run (``x``, ``velocity``), ``step_sizes`` and ``acceptance``
        per chain, and ``step_size``, a 0-dim tensor: ``exp(median(log step_sizes))`` over the chains whose value is finite.
        ``apply=True`` sets the sampler's step size to that value, as the constructor would with a float -- ONE host read;
        ``apply=False`` reads nothing back.  A production run at the adapted step accepts somewhat MORE than ``target_accept``
        (the averaged iterate is not the last one).  On the fused route (module docstring of ``samplers/adapt.py``) the call is
        ONE launch of ``ebm_ghmc_adapt_chain_f32``; a mass, a scheduler, the MLP energy, wider rows and the CPU run the same
        recurrence in torch ops.  With the opt-in ``fused_adapt_mass`` a sampler with a mass is ONE launch too, of
        ``ebm_ghmc_adapt_chain_mass_f32`` (``velocity`` is then the momentum plane).  The caller's ``x`` and ``velocity`` are
        never written.
        """
        from .adapt import adapt_step_size

        return adapt_step_size(self, self.friction, self.temperature, x, dim, n_steps, n_samples, target_accept, init_step_size, t0,
                               gamma, kappa, mu_factor, bounds, velocity, generator, apply)

    def warmup(self, x=None, dim=None, n_samples=1, windows=(50, 50, 100), final_steps=50, target_accept=0.8, regularize=True,
               generator=None, apply=True, **dual_averaging_constants):
        """Stan's warm-up in windows (``samplers/warmup.py``): for each ``w`` in ``windows`` adapt the step size for ``w``
        transitions under the current mass (``adapt_step_size``, fresh momenta, starting from the previous window's pooled step
        size), then set the diagonal mass to ``1 / var`` of the window's final positions pooled over ALL CHAINS (with
        ``regularize`` shrunk as Stan shrinks it: ``var <- N/(N+5) var + 1e-3 * 5/(N+5)``; a coordinate whose variance is not
        finite and positive keeps its mass); then one terminal window of ``final_steps`` under the final mass.  Returns a
        :class:`Warmup` (``x``, ``step_size``, ``mass`` and the per-window lists).  ``apply=True`` sets the sampler's step size and
        its mass as the constructor would; ``apply=False`` leaves the sampler as it was.  Under the conditions of the fused routes
        every window is ONE launch -- ``warmup()`` treats the massed route as eligible without the opt-in ``fused_adapt_mass`` --
        and costs ONE host read, the pooled step size.  ``**dual_averaging_constants``: ``t0``, ``gamma``, ``kappa``,
        ``mu_factor``, ``bounds`` of ``adapt_step_size``.

        Raises:
            ValueError: fewer than 2 rows (the variance is an ensemble estimate across chains), or what ``adapt_step_size`` refuses.
        """
        from .warmup import warmup

        return warmup(self, x, dim, n_samples, windows, final_steps, target_accept, regularize, generator, apply,
                      **dual_averaging_constants)

    # ---------------------------------------------------------------------------------
    # route: torch ops
    # ---------------------------------------------------------------------------------
    # the two draws of the eager route, in one place each: a test replays one device's draws on another through them
    def _draw_normal(self, shape, like: torch.Tensor, generator) -> torch.Tensor:
        return torch.randn(shape, dtype=like.dtype, device=like.device, generator=generator)

    def _draw_uniform(self, n: int, like: torch.Tensor, generator) -> torch.Tensor:
        return torch.rand(n, dtype=like.dtype, device=like.device, generator=generator)

    def _sample_eager(self, x, v, n_steps, thin, want_traj, want_diag, generator, model_kwargs=None):
        model_kwargs = model_kwargs or {}
        traj, diag = new_outputs(x, x.shape, n_steps // thin, want_traj, want_diag, acceptance=True)
        energy = lambda x_: self._model_energy(x_, model_kwargs)  # noqa: E731
        clamped_energy = lambda x_: energy(x_).clamp_(min=-1e10, max=1e10)  # noqa: E731
        massed, m = self.mass is not None, mass_row(self.mass, x)
        if massed:  # sqrt(m) and max(m, 1e-10) per slot; the kinetic energy and the drift spelled as HamiltonianMonteCarlo's eager ones
            m_sqrt, m_safe = mass_forms(self.mass, x)
        if not massed:
            kinetic = lambda v_: (0.5 * torch.sum(v_.flatten(1).square(), dim=-1)).clamp_(min=0.0, max=1e10)  # noqa: E731
        elif isinstance(m, float):
            kinetic = lambda p_: (0.5 * torch.sum(p_.flatten(1).square(), dim=-1) / m).clamp_(min=0.0, max=1e10)  # noqa: E731
        else:
            kinetic = lambda p_: (0.5 * torch.sum((p_.square() / m).flatten(1), dim=-1)).clamp_(min=0.0, max=1e10)  # noqa: E731
        force = lambda x_: (-self._model_gradient(x_, model_kwargs)).clamp_(min=-1e6, max=1e6)  # noqa: E731
        per_chain = lambda m: m.view(-1, *([1] * (x.ndim - 1)))  # noqa: E731
        n, L = x.shape[0], self.n_leapfrog_steps
        if v is None:
            sqrt_temp = ghmc_constants(1.0, 1, self.friction, self.temperature, x.dtype)[2]
            z0 = self._draw_normal(x.shape, x, generator)
            v = (sqrt_temp * m_sqrt) * z0 if massed else sqrt_temp * z0
        keep = 0
        with self.autocast_context():
            for t in range(n_steps):
                eps = self.get_scheduled_value("step_size")
                c1, c2, _, beta = ghmc_constants(eps, L, self.friction, self.temperature, x.dtype)
                xi = self._draw_normal(x.shape, x, generator)
                u = self._draw_uniform(n, x, generator)
                # every operation rounded on its own, in the order of the contract (include/ebm_hip.h)
                v = c1 * v + (c2 * m_sqrt if massed else c2) * xi  # O (with a mass v is the momentum: N(0, T m))
                h0 = clamped_energy(x) + kinetic(v)
                eps_t = torch.full((), float(eps), dtype=x.dtype, device=x.device)
                xp, vp = x, v
                for _ in range(L):  # the safe-mode leapfrog step of integrators/symplectic.py, identity mass
                    v_half = vp + 0.5 * eps_t * force(xp)
                    xp = xp + (eps_t * v_half / m_safe if massed else eps_t * v_half)
                    vp = v_half + 0.5 * eps_t * force(xp)
                    xp = xp.nan_to_num_(nan=0.0)
                    vp = vp.nan_to_num_(nan=0.0)
                h1 = clamped_energy(xp) + kinetic(vp)
                accept_prob = torch.exp((beta * (h0 - h1)).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
                accepted = u < accept_prob
                x = torch.where(per_chain(accepted), xp, x)
                v = torch.where(per_chain(accepted), vp, -v)  # the flip
                self.step_schedulers()
                if (t + 1) % thin == 0:
                    record_kept(x, keep, traj, diag, energy, accepted)
                    keep += 1
        if n_steps == 0:  # never the caller's tensors
            x, v = x.clone(), v.clone()
        return x, v, traj, diag

    # ---------------------------------------------------------------------------------
    # routes: one launch of ebm_ghmc_chain_f32, or (fused_mlp) of ebm_ghmc_mlp_chain_f32 -- the same parameter list
    # ---------------------------------------------------------------------------------
    def _sample_fused(self, x, v, spec: FusedSpec, n_steps, thin, want_traj, want_diag, generator, entry: str = "ebm_ghmc_chain_f32"):
        n, dim = x.shape
        n_kept = n_steps // thin
        state = _lib.dense_f32(x).clone()  # the kernel updates in place; never the caller's tensors
        draw_v0 = v is None
        vel = torch.empty_like(state) if draw_v0 else _lib.dense_f32(v).clone()
        need_kept = (want_traj or want_diag) and n_kept > 0
        traj = torch.empty(n, n_kept, dim, dtype=torch.float32, device=x.device) if (want_traj or need_kept) else None
        mask = torch.empty(n_steps, n, dtype=torch.uint8, device=x.device) if (want_diag and n_kept > 0) else None
        seed, step0 = _rng.reserve(generator, x.device, 2 * n_steps + 1)
        stream = _lib.stream_handle(x.device)
        spec_c = spec.to_c()
        mass = ()
        if self.mass is not None:  # (kind, scalar, pointer) directly behind `temperature`; the diagonal is kept until the launch
            kind, m_scalar, m_diag = _mass_args(self.mass, state)
            mass = (kind, m_scalar, _lib.ptr(m_diag))
        if n > 0 and n_steps > 0:
            _lib.call(
                entry,
                spec_c, _lib.ptr(state), _lib.ptr(vel), n, dim, n_steps, self.n_leapfrog_steps, self.get_scheduled_value("step_size"),
                self.friction, self.temperature, *mass, int(draw_v0), thin, _lib.ptr(traj) if need_kept else None, _lib.ptr(mask), None, None,
                seed, step0, stream,
            )
        elif draw_v0:  # no transition: the start velocities alone, the same field
            if n > 0:
                flat = torch.empty((n * dim + 3) // 4 * 4, dtype=torch.float32, device=x.device)
                _lib.call("ebm_noise_fill_f32", _lib.ptr(flat), n * dim, _lib.NOISE_NORMAL, seed, step0, stream)
                sqrt_temp = ghmc_constants(1.0, 1, self.friction, self.temperature)[2]
                scale = sqrt_temp if self.mass is None else sqrt_temp * mass_forms(self.mass, state)[0]
                vel = scale * flat[: n * dim].view(n, dim)
        self.advance_schedulers(n_steps)
        diag = None
        if want_diag:
            diag = new_outputs(state, state.shape, n_kept, False, True, acceptance=True)[1]
            if n > 0 and n_kept > 0:
                if spec.kind == _lib.ENERGY_MLP:  # the kept positions' statistics in torch ops, their energy the model's
                    for keep in range(n_kept):
                        record_kept(traj[:, keep], keep, None, diag, lambda x_: self._model_energy(x_, {}))
                else:
                    kept_statistics(spec_c, traj, diag, stream)
                diag["acceptance_rate"].copy_(mask[thin - 1 :: thin][:n_kept].float().mean(dim=1))
        return state, vel, (traj if want_traj else None), diag
