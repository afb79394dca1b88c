r"""Underdamped (kinetic) Langevin dynamics in the BAOAB splitting: :class:`UnderdampedLangevin`.

A chain carries a velocity ``v`` beside its position ``x`` (unit mass, friction ``gamma``, temperature ``T``: the target is
``exp(-E / T)``).  One step of size ``h`` (Leimkuhler & Matthews 2013), with ``g = dE/dx(x)`` carried from the step before:

.. math::
    v \leftarrow v - \tfrac h2 g,\quad x \leftarrow x + \tfrac h2 v,\quad
    v \leftarrow e^{-\gamma h} v + \sqrt{T (1 - e^{-2 \gamma h})}\,\xi,\quad
    x \leftarrow x + \tfrac h2 v,\quad g \leftarrow \nabla E(x),\quad v \leftarrow v - \tfrac h2 g

One gradient evaluation per step, as Euler-Maruyama -- but on a quadratic energy the position marginal is exact for every
stable step size (Euler-Maruyama's variance is off by ``1 / (1 - eta k / 2)``), and ``var(v) = T (1 - h^2 k / 4)``.

Two execution routes, chosen once per ``sample()`` call (``_route``):

``fused``  CUDA fp32 state, no autocast, one of the analytic energies (not the MLP), ``dim <= 256`` and a constant step size:
           the whole call -- start velocities, steps, Philox draws, thinned trajectory -- is ONE launch of
           ``ebm_kinetic_chain_f32`` (include/ebm_hip.h states the recurrence exactly; docs/design/kinetic.md the kernel).
``fused_mlp``  opt-in (``sampler.fused_mlp = True``): CUDA fp32 state, no autocast, a constant step size, an ``MLPEnergy`` of
           hidden width 64 / 128 and ``dim == in_dim <= 128``: the whole call is ONE launch of ``ebm_kinetic_mlp_chain_f32``
           (docs/design/kinetic_mlp.md), the evaluation on the matrix cores inside the step loop.  Its gradients are the kernel's
           (fp32-accurate, not autograd's rounding) and its draws the Philox field's, so the default stays ``eager`` for the MLP
           and a call made without the opt-in is bit for bit what it was.
``eager``  everything else (CPU, any other ``BaseModel``, a scheduler on ``step_size``, wider rows, ``model_kwargs``): the same
           recurrence in torch ops around ``model.gradient``, drawing ``randn(n, dim)`` for the start velocities and once per
           step.

``fused_mass``  a sampler built with ``mass=`` (a float or a per-dimension tensor) under the conditions of ``fused``: ONE launch
           of ``ebm_kinetic_chain_mass_f32`` (docs/design/mass.md).  The carried plane is then the MOMENTUM ``p ~ N(0, T m)``:
           ``velocity=`` / ``return_velocity`` carry it, and the step reads ``x += (h / 2) p / m``, ``p = c1 p + c2 sqrt(m) xi``.
           With a mass an ``MLPEnergy`` takes ``eager`` unless both opt-ins below are set.
``fused_mlp_mass``  opt-in twice (``sampler.fused_mlp = True`` and ``sampler.fused_mlp_mass = True``): a sampler built with
           ``mass=`` under the conditions of ``fused_mlp``: ONE launch of ``ebm_kinetic_mlp_chain_mass_f32``
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
from ._chain_host import (check_mass, fused_mlp_walk_fits, kept_statistics, kinetic_temperature, mass_forms, mass_row,
                          new_outputs, record_kept)

FUSED_MAX_DIM = 256  # one vector per lane (csrc/kinetic.hip)


def baoab_constants(h: float, friction: float, temperature: float, dtype: torch.dtype = torch.float32) -> Tuple[float, float, float, float]:
    """``(h / 2, exp(-gamma h), sqrt(T (1 - exp(-2 gamma h))), sqrt(T))``: formed in double, each rounded once to ``dtype``
    (the constants ``ebm_kinetic_chain_f32`` forms from the same three numbers)."""
    vals = (0.5 * h, math.exp(-friction * h), math.sqrt(temperature * (-math.expm1(-2.0 * friction * h))), math.sqrt(temperature))
    return tuple(torch.tensor(vals, dtype=torch.float64).to(dtype).tolist())


class UnderdampedLangevin(BaseSampler):
    """Underdamped Langevin dynamics, BAOAB splitting, unadjusted.

    Args:
        model: energy model to sample from.
        step_size: step size ``h``, a float or (eager route) a ``BaseScheduler``.
        friction: friction ``gamma > 0``.
        temperature: temperature ``T > 0``; the chains sample ``exp(-E / T)``.
        dtype, device: where the chains live.
        mass: ``None`` (unit mass), a positive finite float, or a 1-D tensor of per-dimension masses (moved to the sampler's
            device; its entries are not inspected).  With a mass the carried plane is the momentum ``p ~ N(0, T m)``.
    """

    #: opt-in: an ``MLPEnergy`` (hidden 64 / 128, ``dim == in_dim <= 128``, CUDA fp32, no autocast, a constant step size) runs as
    #: ONE launch of ``ebm_kinetic_mlp_chain_f32`` instead of the eager route.  Off by default: the fused evaluation is
    #: three-way-split bf16 arithmetic at fp32 accuracy, not autograd's rounding, and the draws are the Philox field's, not torch's.
    fused_mlp = False
    #: second opt-in, read by ``sample_moments`` only: with ``fused_mlp`` set too, an eligible ``MLPEnergy`` call of
    #: ``sample_moments`` is ONE launch of ``ebm_kinetic_moments_mlp_f32`` (docs/design/kinetic_moments_mlp.md).  Off by default: with
    #: ``fused_mlp`` alone ``sample_moments`` keeps the step-by-step recurrence and autograd's energies.
    fused_mlp_moments = False
    #: third opt-in, read by ``sample`` of a sampler built with ``mass=``: with ``fused_mlp`` set too, an eligible ``MLPEnergy`` call
    #: is ONE launch of ``ebm_kinetic_mlp_chain_mass_f32`` (docs/design/mass_mlp.md).  Off by default: with ``fused_mlp`` alone a
    #: massed sampler on an ``MLPEnergy`` keeps the eager route and its bits.
    fused_mlp_mass = False

    def __init__(
        self,
        model: BaseModel,
        step_size: Union[float, BaseScheduler] = 1e-2,
        friction: float = 1.0,
        temperature: float = 1.0,
        dtype: torch.dtype = torch.float32,
        device: Optional[Union[str, torch.device]] = None,
        mass: Optional[Union[float, torch.Tensor]] = None,
    ):
        super().__init__(model=model, dtype=dtype, device=device)
        self._register_param("step_size", step_size, positive=True)
        self.mass = check_mass(mass, self.device)
        if not (friction > 0 and math.isfinite(friction)):
            raise ValueError("friction must be positive")
        if not (temperature > 0 and math.isfinite(temperature)):
            raise ValueError("temperature must be positive")
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
        """Run ``n_steps`` BAOAB steps.

        ``model_kwargs``: conditioning passed to the model at every evaluation; a non-empty dict takes the eager route.

        ``velocity``: the start velocities, shaped as ``x`` (as a call with ``return_velocity=True`` returned them: continue
        that run); ``None`` draws them from ``N(0, T I)``.  A sampler with a ``mass`` carries the momentum in this plane
        (``N(0, T m)``), here and in ``return_velocity``.

        Returns the final positions ``[n, *shape]`` (or, with ``return_trajectory``, the kept positions
        ``[n, n_steps // thin, *shape]``); with ``return_diagnostics`` a dict follows, holding ``"mean"`` / ``"var"``
        (``[n_kept, *shape]``, biased variance clamped to [1e-10, 1e10]) and ``"energy"`` (``[n_kept]``) of the kept
        positions and ``"kinetic_temperature"``, the mean of ``v^2`` (with a mass: of ``p^2 / m``) over chains and coordinates of the final velocities -- an
        estimate of ``T (1 - h^2 E'' / 4)``, a cheap check of the step size; with ``return_velocity`` the final velocities
        come last.  The caller's ``x`` and ``velocity`` are never written.

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
                                                      entry="ebm_kinetic_chain_mass_f32")
        elif route == "fused_mlp":
            state, v, traj, diag = self._sample_fused(x, velocity, spec, n_steps, thin, return_trajectory, return_diagnostics, generator,
                                                      entry="ebm_kinetic_mlp_chain_f32")
        elif route == "fused_mlp_mass":
            state, v, traj, diag = self._sample_fused(x, velocity, spec, n_steps, thin, return_trajectory, return_diagnostics, generator,
                                                      entry="ebm_kinetic_mlp_chain_mass_f32")
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
        """Run ``n_steps`` BAOAB steps and keep per-chain running moments of the positions after the first ``burn_in``
        (with ``energy`` of their energies too) and the running mean of ``v^2`` -- no trajectory is written.

        Returns ``(x_final, ChainMoments)``, with ``return_velocity`` ``(x_final, ChainMoments, v_final)``.  The moments
        carry ``rhat``, ``ess``, ``mean``, ``var`` and ``kinetic_temperature``, the time- and chain-averaged ``v^2`` per
        coordinate: an estimate of ``T (1 - h^2 E'' / 4)``.  When ``n_steps - burn_in`` is odd one more step is burnt.  On
        the fused route (see the module docstring) the call is ONE launch of ``ebm_kinetic_moments_f32`` and ``x_final``,
        ``v_final`` are ``sample(return_velocity=True)``'s for the same generator state.  On an eligible ``MLPEnergy`` with
        both opt-ins, ``fused_mlp`` and ``fused_mlp_moments``, it is ONE launch of ``ebm_kinetic_moments_mlp_f32`` and matches
        ``sample()`` under ``fused_mlp`` in the same way; with ``fused_mlp`` alone it stays step by step.  The caller's ``x``
        and ``velocity`` are never written.

        Raises:
            ValueError: fewer than 4 counted steps, ``burn_in`` outside ``0 .. n_steps``, a ``velocity`` of another shape.
        """
        from .kinetic_moments import sample_moments

        return sample_moments(self, False, x, dim, n_steps, n_samples, burn_in, energy, velocity, return_velocity, generator)

    # ---------------------------------------------------------------------------------
    # route: torch ops
    # ---------------------------------------------------------------------------------
    def _sample_eager(self, x, v, n_steps, thin, want_traj, want_diag, generator, model_kwargs=None):
        model_kwargs = model_kwargs or {}
        traj, diag = new_outputs(x, x.shape, n_steps // thin, want_traj, want_diag)
        energy = lambda x_: self._model_energy(x_, model_kwargs)  # noqa: E731
        massed = self.mass is not None
        if massed:  # the per-slot forms of the contract: sqrt(m) and max(m, 1e-10), in the state's dtype
            m_sqrt, m_safe = mass_forms(self.mass, x)
        if v is None:
            sqrt_temp = baoab_constants(1.0, self.friction, self.temperature, x.dtype)[3]
            z0 = torch.randn(x.shape, dtype=x.dtype, device=x.device, generator=generator)
            v = (sqrt_temp * m_sqrt) * z0 if massed else sqrt_temp * z0
        keep = 0
        with self.autocast_context():
            g = self._model_gradient(x, model_kwargs)
            for s in range(n_steps):
                hh, c1, c2, _ = baoab_constants(self.get_scheduled_value("step_size"), self.friction, self.temperature, x.dtype)
                xi = torch.randn(x.shape, dtype=x.dtype, device=x.device, generator=generator)
                # every operation rounded on its own, in the order of the contract (include/ebm_hip.h); with a mass v is the
                # momentum, the drift runs on a = hh / m_safe and the refresh on s = c2 * m_sqrt
                # (a true division: torch spells `float / tensor` as reciprocal-then-multiply, two roundings)
                a, sc = (torch.full_like(m_safe, hh) / m_safe, c2 * m_sqrt) if massed else (hh, c2)
                v = v - hh * g
                x = x + a * v
                v = c1 * v + sc * xi
                x = x + a * v
                g = self._model_gradient(x, model_kwargs)
                v = v - hh * g
                self.step_schedulers()
                if (s + 1) % thin == 0:
                    record_kept(x, keep, traj, diag, energy)
                    keep += 1
        if n_steps == 0:  # never the caller's tensors
            x, v = x.clone(), v.clone()
        return x, v, traj, diag

    # ---------------------------------------------------------------------------------
    # routes: one launch of ebm_kinetic_chain_f32, or (fused_mlp) of ebm_kinetic_mlp_chain_f32 -- the same parameter list
    # ---------------------------------------------------------------------------------
    def _sample_fused(self, x, v, spec: FusedSpec, n_steps, thin, want_traj, want_diag, generator, entry: str = "ebm_kinetic_chain_f32"):
        n, dim = x.shape
        n_kept = n_steps // thin
        state = _lib.dense_f32(x).clone()  # the kernel updates in place; never the caller's tensors
        draw_v0 = v is None
        vel = torch.empty_like(state) if draw_v0 else _lib.dense_f32(v).clone()
        need_kept = (want_traj or want_diag) and n_kept > 0
        traj = torch.empty(n, n_kept, dim, dtype=torch.float32, device=x.device) if (want_traj or need_kept) else None
        seed, step0 = _rng.reserve(generator, x.device, n_steps + 1)
        stream = _lib.stream_handle(x.device)
        spec_c = spec.to_c()
        mass = ()
        if self.mass is not None:  # (kind, scalar, pointer) directly behind `temperature`; the diagonal is kept until the launch
            kind, m_scalar, m_diag = _mass_args(self.mass, state)
            mass = (kind, m_scalar, _lib.ptr(m_diag))
        if n > 0 and n_steps > 0:
            _lib.call(
                entry,
                spec_c, _lib.ptr(state), _lib.ptr(vel), n, dim, n_steps, self.get_scheduled_value("step_size"), self.friction,
                self.temperature, *mass, int(draw_v0), thin, _lib.ptr(traj) if need_kept else None, None, seed, step0, stream,
            )
        elif draw_v0:  # no step: the start velocities alone, the same field
            if n > 0:
                flat = torch.empty((n * dim + 3) // 4 * 4, dtype=torch.float32, device=x.device)
                _lib.call("ebm_noise_fill_f32", _lib.ptr(flat), n * dim, _lib.NOISE_NORMAL, seed, step0, stream)
                sqrt_temp = baoab_constants(1.0, self.friction, self.temperature)[3]
                scale = sqrt_temp if self.mass is None else sqrt_temp * mass_forms(self.mass, state)[0]
                vel = scale * flat[: n * dim].view(n, dim)
        self.advance_schedulers(n_steps)
        diag = None
        if want_diag:
            diag = new_outputs(state, state.shape, n_kept, False, True)[1]
            if n > 0 and n_kept > 0:
                if spec.kind == _lib.ENERGY_MLP:  # the kept positions' statistics in torch ops, their energy the model's
                    for keep in range(n_kept):
                        record_kept(traj[:, keep], keep, None, diag, lambda x_: self._model_energy(x_, {}))
                else:
                    kept_statistics(spec_c, traj, diag, stream)
        return state, vel, (traj if want_traj else None), diag
