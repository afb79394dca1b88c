r"""Replica-exchange (parallel tempering) samplers: :class:`ReplicaExchangeLangevin` and :class:`ReplicaExchangeHMC`.

Replica-exchange Langevin dynamics
----------------------------------

Every chain becomes a *ladder* of ``R`` copies at temperatures ``T_0 < T_1 < ... < T_{R-1}``; slot 0 is the target.
Slot ``r`` takes the Euler-Maruyama step of :class:`LangevinDynamics` with the noise coefficient
``sqrt(2 sigma^2 T_r)`` -- it samples ``exp(-E / (sigma^2 T_r))`` -- and every ``swap_every`` steps adjacent slots
propose to exchange their states, accepted with probability ``min(1, exp((beta_r - beta_{r+1}) (E_r - E_{r+1})))``,
``beta_r = 1 / (sigma^2 T_r)``.  Even events pair the slots (0,1), (2,3), ..., odd events (1,2), (3,4), ....  The hot
slots cross barriers that the target slot does not, and the swaps carry those crossings down the ladder.

The execution routes, chosen once per ``sample()`` call (``_route``):

``fused``  CUDA fp32 state, one of the analytic energies (not the MLP), float step size and noise scale, and a ladder
           that fits one workgroup (``R * G <= 256``, ``G`` the lanes per row): the whole call -- steps, swap events,
           Philox draws, thinned trajectory of slot 0, swap counters -- is ONE launch of ``ebm_tempering_chain_f32``
           (include/ebm_hip.h states the algorithm exactly; docs/design/tempering.md the kernel).
``fused_mlp``  only with the opt-in ``sampler.fused_mlp_ladder = True``: an ``MLPEnergy`` of hidden width 64 / 128 with
           ``dim == in_dim <= 128`` and a ladder of 2, 4, 8, 16 or 32 slots, constant step size and noise scale: ONE
           launch of ``ebm_tempering_mlp_chain_f32`` with the same parameter list and Philox coordinates
           (docs/design/tempering_mlp.md).
``eager``  everything else (CPU, any other ``BaseModel`` such as ``MLPEnergy`` without the opt-in or a hand-written energy,
           schedulers): the same algorithm in torch ops, drawing ``randn(n, R, dim)`` per step and ``rand(n, R)`` per event.

A fused-eligible call never falls back to eager: a missing library or a failing launch raises.

Replica-exchange HMC
--------------------
The same ladders with a Metropolis-corrected HMC transition in every slot, so no slot carries a discretisation bias: slot
``r`` samples ``exp(-E / T_r)`` exactly.  See :class:`ReplicaExchangeHMC`; the fused route is ONE launch of
``ebm_tempering_hmc_chain_f32`` (docs/design/tempering_hmc.md) and, for an ``MLPEnergy`` with the opt-in
``sampler.fused_mlp = True``, ONE launch of ``ebm_tempering_hmc_mlp_chain_f32`` (docs/design/tempering_hmc_mlp.md).
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import torch

from .. import _lib, _rng
from ..core.energies import BaseModel, FusedSpec, fused_spec_for
from ..core.sampler_base import BaseSampler
from ..core.schedules import BaseScheduler
from ._chain_host import (FUSED_MLP_LADDERS, FUSED_MLP_MAX_DIM, fused_mlp_walk_fits, kept_statistics, new_outputs,  # noqa: F401
                          record_kept)  # (FUSED_MLP_LADDERS, FUSED_MLP_MAX_DIM: importable from here as before)


def ladder_coefficients(noise_scale: float, temperatures: Sequence[float]) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(noise_coef[R], beta[R])`` as fp32: formed in double, rounded once (include/ebm_hip.h)."""
    t = torch.tensor([float(v) for v in temperatures], dtype=torch.float64)
    s2 = float(noise_scale) ** 2
    return torch.sqrt(2.0 * s2 * t).to(torch.float32), (1.0 / (s2 * t)).to(torch.float32)


def lanes_per_row(dim: int) -> int:
    """The lane-group width ``G`` of csrc/rows.h (``pick_geometry``) for a row of ``dim`` columns."""
    nvec = (dim + 3) // 4
    g = 1
    while g < nvec and g < 64:
        g <<= 1
    return g


class _LadderSampler(BaseSampler):
    """What the replica-exchange samplers share: the ladder's validation and the start conventions of ``sample()``."""

    def _init_ladder(self, temperatures: Sequence[float], swap_every: int) -> None:
        temps = tuple(float(t) for t in temperatures)
        if len(temps) < 2:
            raise ValueError("temperatures must hold at least two values")
        if temps[0] <= 0 or any(b <= a for a, b in zip(temps, temps[1:])):
            raise ValueError(f"temperatures must be positive and strictly increasing, got {temps}")
        if int(swap_every) < 1:
            raise ValueError("swap_every must be >= 1")
        self.temperatures = temps
        self.swap_every = int(swap_every)

    @property
    def n_replicas(self) -> int:
        return len(self.temperatures)

    def _start_ladders(self, x, dim, n_samples, thin, return_trajectory, return_replicas, generator) -> torch.Tensor:
        """The checks every ``sample()`` makes and the start as contiguous ladders ``[n, R, dim]``."""
        if thin < 1:
            raise ValueError("thin must be >= 1")
        if return_trajectory and return_replicas:
            raise ValueError("return_trajectory and return_replicas exclude each other")
        self.reset_schedulers()
        R = self.n_replicas
        x = self._init_state(x, dim, n_samples, generator)
        if x.ndim == 2:
            x = x.unsqueeze(1).expand(-1, R, -1)
        elif x.ndim != 3 or x.shape[1] != R:
            raise ValueError(f"x must be [n, dim] or [n, {R}, dim], got {tuple(x.shape)}")
        return x.contiguous()


class ReplicaExchangeLangevin(_LadderSampler):
    """Langevin dynamics on a temperature ladder with replica exchange.

    Args:
        model: energy model to sample from.
        step_size: step size, a float or (eager route) a ``BaseScheduler``.
        noise_scale: noise scale ``sigma`` of the target slot, a float or (eager route) a ``BaseScheduler``.
        temperatures: strictly increasing, positive, at least two; the first is the target's.
        swap_every: a swap event follows every ``swap_every``-th step.
        dtype, device: where the ladders live.

    ``fused_mlp_ladder`` (class attribute, ``False``): set it on a sampler to send an eligible ``MLPEnergy`` call -- hidden
    width 64 / 128, ``dim == in_dim <= 128``, ``R`` in {2, 4, 8, 16, 32}, constant step size and noise scale -- to the route
    ``fused_mlp``: ONE launch of ``ebm_tempering_mlp_chain_f32`` per call, the matrix-core evaluation inside the walk (split-bf16
    / exact-f32 MFMA arithmetic at fp32 accuracy, not autograd's rounding) and Philox draws instead of torch's generator,
    never a fallback.  Off by default: a default sampler on an MLP keeps its eager bits.
    """

    fused_mlp_ladder = False

    def __init__(
        self,
        model: BaseModel,
        step_size: Union[float, BaseScheduler] = 1e-3,
        noise_scale: Union[float, BaseScheduler] = 1.0,
        temperatures: Sequence[float] = (1.0, 2.0, 4.0, 8.0),
        swap_every: int = 10,
        dtype: torch.dtype = torch.float32,
        device: Optional[Union[str, torch.device]] = None,
    ):
        super().__init__(model=model, dtype=dtype, device=device)
        self._register_param("step_size", step_size, positive=True)
        self._register_param("noise_scale", noise_scale, positive=True)
        self._init_ladder(temperatures, swap_every)

    # ---------------------------------------------------------------------------------
    # routing: decided here and nowhere else
    # ---------------------------------------------------------------------------------
    def _route(self, x: torch.Tensor) -> Tuple[str, Optional[FusedSpec]]:
        """``x``: the ladders ``[n, R, dim]``."""
        if not x.is_cuda or x.dtype != torch.float32 or x.ndim != 3:
            return "eager", None
        if not (self.schedulers["step_size"].is_constant() and self.schedulers["noise_scale"].is_constant()):
            return "eager", None
        if self.use_mixed_precision and self.autocast_available:
            return "eager", None
        rows = x.view(-1, x.shape[-1])
        spec = fused_spec_for(self.model, rows, None)
        if spec is not None and spec.kind == _lib.ENERGY_MLP:
            dim = rows.shape[1]
            if self.fused_mlp_ladder and fused_mlp_walk_fits(spec.n_comp, getattr(self.model, "in_dim", None), dim, self.n_replicas):
                return "fused_mlp", spec
            return "eager", None
        if spec is None:
            return "eager", None
        if self.n_replicas > 64 or self.n_replicas * lanes_per_row(rows.shape[1]) > 256:
            return "eager", None
        return "fused", spec

    # ---------------------------------------------------------------------------------
    # public API
    # ---------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(
        self,
        x: Optional[torch.Tensor] = None,
        dim: Optional[int] = None,
        n_steps: int = 100,
        n_samples: int = 1,
        thin: int = 1,
        return_trajectory: bool = False,
        return_diagnostics: bool = False,
        return_replicas: bool = False,
        generator: Optional[torch.Generator] = None,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, Dict[str, torch.Tensor]]]:
        """Run ``n_steps`` steps of every slot with the swap events between them.

        ``x``: ``[n, dim]`` (every slot of ladder ``i`` starts at ``x[i]``), ``[n, R, dim]`` (a ladder as
        ``return_replicas=True`` returned it: continue), or ``None`` (``n_samples`` draws from N(0, I) of width ``dim``).

        Returns the slot-0 states ``[n, dim]``; with ``return_trajectory`` the kept slot-0 states
        ``[n, n_steps // thin, dim]``; with ``return_replicas`` the whole ladders ``[n, R, dim]``.  With
        ``return_diagnostics`` a second value: ``"swap_acceptance"`` ``[R - 1]`` (accepted / attempted swaps of each adjacent
        pair over the call, NaN for a pair that was never attempted) and ``"mean"`` / ``"var"`` (``[n_kept, dim]``, biased
        variance clamped to [1e-10, 1e10]) / ``"energy"`` (``[n_kept]``) of slot 0 at the kept steps.

        Raises:
            ValueError: ``thin < 1``, ``x`` and ``dim`` both ``None``, a state that is neither ``[n, dim]`` nor
                ``[n, R, dim]``, or ``return_trajectory`` together with ``return_replicas``.
        """
        x = self._start_ladders(x, dim, n_samples, thin, return_trajectory, return_replicas, generator)
        route, spec = self._route(x)
        if route == "fused":
            state, traj, diag = self._sample_fused(x, spec, n_steps, thin, return_trajectory, return_diagnostics, generator)
        elif route == "fused_mlp":
            state, traj, diag = self._sample_fused(x, spec, n_steps, thin, return_trajectory, return_diagnostics, generator,
                                                   entry="ebm_tempering_mlp_chain_f32")
        else:
            state, traj, diag = self._sample_eager(x, n_steps, thin, return_trajectory, return_diagnostics, generator)
        out = traj if return_trajectory else (state if return_replicas else state[:, 0].contiguous())
        return (out, diag) if return_diagnostics else out

    # ---------------------------------------------------------------------------------
    # route: torch ops
    # ---------------------------------------------------------------------------------
    def _sample_eager(self, x, n_steps, thin, want_traj, want_diag, generator):
        n, R, dim = x.shape
        n_kept = n_steps // thin
        x = x.clone()
        traj, diag = new_outputs(x, (n, dim), n_kept, want_traj, want_diag)
        cold_energy = lambda cold: self._model_energy(cold.contiguous(), {})  # noqa: E731
        tried = torch.zeros(R - 1, dtype=torch.float64)
        took = torch.zeros(R - 1, dtype=torch.float64)
        keep = event = 0
        with self.autocast_context():
            for s in range(n_steps):
                eta = self.get_scheduled_value("step_size")
                coef, beta = ladder_coefficients(self.get_scheduled_value("noise_scale"), self.temperatures)
                coef, beta = coef.to(x.device, x.dtype).view(1, R, 1), beta.to(x.device, x.dtype)
                noise = torch.randn(n, R, dim, dtype=x.dtype, device=x.device, generator=generator)
                grad = self._model_gradient(x.view(n * R, dim), {}).view(n, R, dim)
                # the reference's Euler-Maruyama op order (LangevinDynamics): rounded mul, rounded add
                x = (x - eta * grad) + coef * (noise * eta**0.5)
                self.step_schedulers()
                if (s + 1) % self.swap_every == 0:
                    u = torch.rand(n, R, dtype=x.dtype, device=x.device, generator=generator)
                    energy = self._model_energy(x.view(n * R, dim), {}).view(n, R)
                    for r in range(event % 2, R - 1, 2):
                        delta = (beta[r] - beta[r + 1]) * (energy[:, r] - energy[:, r + 1])
                        ok = (delta == delta) & (u[:, r] < torch.exp(delta.clamp(max=0.0)))
                        tried[r] += n
                        took[r] += int(ok.sum())
                        lower = x[:, r].clone()
                        x[:, r] = torch.where(ok[:, None], x[:, r + 1], lower)
                        x[:, r + 1] = torch.where(ok[:, None], lower, x[:, r + 1])
                    event += 1
                if (s + 1) % thin == 0:
                    record_kept(x[:, 0], keep, traj, diag, cold_energy)
                    keep += 1
        if diag is not None:
            diag["swap_acceptance"] = (took / tried).to(device=x.device, dtype=x.dtype)
        return x, traj, diag

    # ---------------------------------------------------------------------------------
    # routes: one launch of ebm_tempering_chain_f32, or (fused_mlp) of ebm_tempering_mlp_chain_f32 -- the same parameter list
    # ---------------------------------------------------------------------------------
    def _ladder_on(self, device: torch.device, sigma: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """The two device arrays of the ladder, kept for the next call with the same noise scale."""
        key = (device, sigma, self.temperatures)
        cached = getattr(self, "_ladder_cache", None)
        if cached is None or cached[0] != key:
            coef, beta = ladder_coefficients(sigma, self.temperatures)
            cached = (key, coef.to(device), beta.to(device))
            self._ladder_cache = cached
        return cached[1], cached[2]

    def _sample_fused(self, x, spec: FusedSpec, n_steps, thin, want_traj, want_diag, generator,
                      entry: str = "ebm_tempering_chain_f32"):
        n, R, dim = x.shape
        n_kept = n_steps // thin
        state = _lib.dense_f32(x).clone()  # the kernel updates in place; never the caller's tensor
        eta = self.get_scheduled_value("step_size")
        coef, beta = self._ladder_on(x.device, self.get_scheduled_value("noise_scale"))
        need_kept = (want_traj or want_diag) and n_kept > 0
        traj = torch.empty(n, n_kept, dim, dtype=torch.float32, device=x.device) if (want_traj or need_kept) else None
        counts = torch.zeros(2 * (R - 1), dtype=torch.int32, device=x.device) if want_diag else None
        seed, step0 = _rng.reserve(generator, x.device, 2 * n_steps)
        stream = _lib.stream_handle(x.device)
        spec_c = spec.to_c()
        if n > 0 and n_steps > 0:
            _lib.call(
                entry,
                spec_c, _lib.ptr(state), n, R, dim, n_steps, eta, eta**0.5, _lib.ptr(coef), _lib.ptr(beta),
                self.swap_every, thin, _lib.ptr(traj) if need_kept else None, _lib.ptr(counts), None, None, seed, step0, stream,
            )
        self.advance_schedulers(n_steps)
        diag = None
        if want_diag:
            diag = new_outputs(state, (n, dim), n_kept, False, True)[1]
            if n > 0 and n_kept > 0:
                if spec.kind == _lib.ENERGY_MLP:  # the kept states' statistics in torch ops, their energy the model's
                    for keep in range(n_kept):
                        record_kept(traj[:, keep], keep, None, diag, lambda x_: self._model_energy(x_.contiguous(), {}))
                else:
                    kept_statistics(spec_c, traj, diag, stream)
            c = (counts.to(torch.int64) & 0xFFFFFFFF).to(torch.float64)  # (uint32 counters in an int32 tensor)
            diag["swap_acceptance"] = (c[R - 1 :] / c[: R - 1]).to(torch.float32)
        return state, (traj if want_traj else None), diag


def hmc_ladder_coefficients(temperatures: Sequence[float]) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(sqrt_temp[R], beta[R])`` as fp32: formed in double, rounded once (include/ebm_hip.h)."""
    t = torch.tensor([float(v) for v in temperatures], dtype=torch.float64)
    return torch.sqrt(t).to(torch.float32), (1.0 / t).to(torch.float32)


class ReplicaExchangeHMC(_LadderSampler):
    r"""Hamiltonian Monte Carlo on a temperature ladder with replica exchange: parallel tempering around a
    Metropolis-corrected kernel, so every slot -- the target included -- samples its law without a discretisation bias.

    Slot ``r`` samples ``exp(-E / T_r)`` with the mass ``M = I / T_r``: in the velocity variable that is the ordinary
    leapfrog on ``E`` with velocities drawn from ``N(0, T_r)``, accepted with probability
    ``min(1, exp((H0 - H1) / T_r))``, ``H = E + |w|^2 / 2``.  After every ``swap_every``-th transition adjacent slots
    propose to exchange their states exactly as in :class:`ReplicaExchangeLangevin`
    (``min(1, exp((1/T_r - 1/T_{r+1}) (E_r - E_{r+1})))``, even events pair (0,1), (2,3), ..., odd events (1,2), ...), on
    the energies the transitions already computed.  ``include/ebm_hip.h`` (``ebm_tempering_hmc_chain_f32``) states the
    algorithm exactly.

    Args:
        model: energy model to sample from.
        step_size: leapfrog step size: a float (every slot), a sequence of ``R`` floats (one per slot: hot slots of an energy
            with quartic walls need shorter steps) or, on the eager route, a ``BaseScheduler``.
        n_leapfrog_steps: leapfrog steps per transition.
        temperatures: strictly increasing, positive, at least two; the first is the target's.
        swap_every: a swap event follows every ``swap_every``-th transition.
        dtype, device: where the ladders live.

    Routes, chosen once per ``sample()`` call (``_route``): ``fused`` -- CUDA fp32 state, an analytic energy (not the MLP),
    constant step sizes, ``dim <= 256`` and a ladder that fits one workgroup (``R * G <= 256``): ONE launch of
    ``ebm_tempering_hmc_chain_f32`` per call, never a fallback; ``eager`` -- everything else, the same algorithm in torch
    ops, drawing ``randn(n, R, dim)`` and ``rand(n, R)`` per transition and ``rand(n, R)`` per event.

    ``fused_mlp`` (class attribute, ``False``): set it on a sampler to send an eligible ``MLPEnergy`` call -- hidden width
    64 / 128, ``dim == in_dim <= 128``, ``R`` in {2, 4, 8, 16, 32}, constant step sizes -- to the route ``fused_mlp``: ONE launch
    of ``ebm_tempering_hmc_mlp_chain_f32`` per call with the same Philox coordinates, the matrix-core evaluation inside the
    trajectories (fp32 accuracy, not autograd's rounding), never a fallback.  Off by default: a default sampler on an MLP keeps
    its eager bits.
    """

    fused_mlp = False

    def __init__(
        self,
        model: BaseModel,
        step_size: Union[float, Sequence[float], BaseScheduler] = 1e-3,
        n_leapfrog_steps: int = 10,
        temperatures: Sequence[float] = (1.0, 2.0, 4.0, 8.0),
        swap_every: int = 1,
        dtype: torch.dtype = torch.float32,
        device: Optional[Union[str, torch.device]] = None,
    ):
        super().__init__(model=model, dtype=dtype, device=device)
        self._init_ladder(temperatures, swap_every)
        self.slot_step_sizes: Optional[Tuple[float, ...]] = None
        if isinstance(step_size, (BaseScheduler, float, int)):
            self._register_param("step_size", step_size, positive=True)
        else:
            sizes = tuple(float(v) for v in step_size)
            if len(sizes) != self.n_replicas:
                raise ValueError(f"step_size must be a float or hold one value per slot ({self.n_replicas}), got {len(sizes)}")
            if any(v <= 0 for v in sizes):
                raise ValueError("step_size must be positive")
            self.slot_step_sizes = sizes
            self._register_param("step_size", sizes[0], positive=True)
        if int(n_leapfrog_steps) < 1:
            raise ValueError("n_leapfrog_steps must be >= 1")
        self.n_leapfrog_steps = int(n_leapfrog_steps)

    def _step_sizes(self) -> Tuple[float, ...]:
        """The R step sizes the next transition uses."""
        if self.slot_step_sizes is not None:
            return self.slot_step_sizes
        return (self.get_scheduled_value("step_size"),) * self.n_replicas

    # ---------------------------------------------------------------------------------
    # routing: decided here and nowhere else
    # ---------------------------------------------------------------------------------
    def _route(self, x: torch.Tensor) -> Tuple[str, Optional[FusedSpec]]:
        """``x``: the ladders ``[n, R, dim]``."""
        if not x.is_cuda or x.dtype != torch.float32 or x.ndim != 3:
            return "eager", None
        if not self.schedulers["step_size"].is_constant():
            return "eager", None
        if self.use_mixed_precision and self.autocast_available:
            return "eager", None
        rows = x.view(-1, x.shape[-1])
        if rows.shape[1] > 256:
            return "eager", None
        spec = fused_spec_for(self.model, rows, None)
        if spec is None:
            return "eager", None
        if spec.kind == _lib.ENERGY_MLP:
            dim = rows.shape[1]
            if self.fused_mlp and fused_mlp_walk_fits(spec.n_comp, getattr(self.model, "in_dim", None), dim, self.n_replicas):
                return "fused_mlp", spec
            return "eager", None
        if self.n_replicas > 64 or self.n_replicas * lanes_per_row(rows.shape[1]) > 256:
            return "eager", None
        return "fused", spec

    # ---------------------------------------------------------------------------------
    # public API
    # ---------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(
        self,
        x: Optional[torch.Tensor] = None,
        dim: Optional[int] = None,
        n_steps: int = 100,
        n_samples: int = 1,
        thin: int = 1,
        return_trajectory: bool = False,
        return_diagnostics: bool = False,
        return_replicas: bool = False,
        generator: Optional[torch.Generator] = None,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, Dict[str, torch.Tensor]]]:
        """Run ``n_steps`` transitions of every slot with the swap events between them.

        Arguments and return conventions are those of :meth:`ReplicaExchangeLangevin.sample` (``x``: ``[n, dim]``,
        ``[n, R, dim]`` or ``None``; the slot-0 states, their kept trajectory, or with ``return_replicas`` the ladders).
        The diagnostics add ``"acceptance_rate"`` ``[R]``: accepted / proposed transitions of each slot over the call.
        """
        x = self._start_ladders(x, dim, n_samples, thin, return_trajectory, return_replicas, generator)
        route, spec = self._route(x)
        if route == "fused":
            state, traj, diag = self._sample_fused(x, spec, n_steps, thin, return_trajectory, return_diagnostics, generator)
        elif route == "fused_mlp":
            state, traj, diag = self._sample_fused(x, spec, n_steps, thin, return_trajectory, return_diagnostics, generator,
                                                   entry="ebm_tempering_hmc_mlp_chain_f32")
        else:
            state, traj, diag = self._sample_eager(x, n_steps, thin, return_trajectory, return_diagnostics, generator)
        out = traj if return_trajectory else (state if return_replicas else state[:, 0].contiguous())
        return (out, diag) if return_diagnostics else out

    # ---------------------------------------------------------------------------------
    # route: torch ops
    # ---------------------------------------------------------------------------------
    def _sample_eager(self, x, n_steps, thin, want_traj, want_diag, generator):
        n, R, dim = x.shape
        n_kept = n_steps // thin
        x = x.clone()
        traj, diag = new_outputs(x, (n, dim), n_kept, want_traj, want_diag)
        cold_energy = lambda cold: self._model_energy(cold.contiguous(), {})  # noqa: E731
        sqrt_temp, beta = (v.to(x.device, x.dtype) for v in hmc_ladder_coefficients(self.temperatures))
        sqrt_temp = sqrt_temp.view(1, R, 1)
        accepted = torch.zeros(R, dtype=torch.float64)
        tried = torch.zeros(R - 1, dtype=torch.float64)
        took = torch.zeros(R - 1, dtype=torch.float64)
        rows = lambda t: t.reshape(n * R, dim)  # noqa: E731
        force_at = lambda t: (-self._model_gradient(rows(t), {}).view(n, R, dim)).clamp_(min=-1e6, max=1e6)  # noqa: E731
        hamiltonian = lambda e, w: e.clamp(min=-1e10, max=1e10) + (0.5 * torch.sum(w.square(), dim=-1)).clamp_(min=0.0, max=1e10)  # noqa: E731
        keep = event = 0
        with self.autocast_context():
            for t in range(n_steps):
                eps = torch.tensor(self._step_sizes(), dtype=x.dtype, device=x.device).view(1, R, 1)
                half = 0.5 * eps
                w = torch.randn(n, R, dim, dtype=x.dtype, device=x.device, generator=generator) * sqrt_temp
                u = torch.rand(n, R, dtype=x.dtype, device=x.device, generator=generator)
                e0 = self._model_energy(rows(x), {}).view(n, R)
                h0 = hamiltonian(e0, w)
                # the safe-mode leapfrog step of HamiltonianMonteCarlo, literally: the force re-evaluated at the top of
                # every step, two half kicks, both scrubs
                xp = x
                for _ in range(self.n_leapfrog_steps):
                    w_half = w + half * force_at(xp)
                    xp = xp + eps * w_half
                    w = w_half + half * force_at(xp)
                    xp = xp.nan_to_num_(nan=0.0)
                    w = w.nan_to_num_(nan=0.0)
                e1 = self._model_energy(rows(xp), {}).view(n, R)
                h1 = hamiltonian(e1, w)
                a = torch.exp((beta * (h0 - h1)).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
                ok = u < a
                accepted += ok.sum(dim=0).double().cpu()
                x = torch.where(ok[:, :, None], xp, x)
                energy = torch.where(ok, e1, e0)  # of the states the slots now hold: an event evaluates nothing
                self.step_schedulers()
                if (t + 1) % self.swap_every == 0:
                    u = torch.rand(n, R, dtype=x.dtype, device=x.device, generator=generator)
                    for r in range(event % 2, R - 1, 2):
                        delta = (beta[r] - beta[r + 1]) * (energy[:, r] - energy[:, r + 1])
                        ok = (delta == delta) & (u[:, r] < torch.exp(delta.clamp(max=0.0)))
                        tried[r] += n
                        took[r] += int(ok.sum())
                        lower = x[:, r].clone()
                        x[:, r] = torch.where(ok[:, None], x[:, r + 1], lower)
                        x[:, r + 1] = torch.where(ok[:, None], lower, x[:, r + 1])
                    event += 1
                if (t + 1) % thin == 0:
                    record_kept(x[:, 0], keep, traj, diag, cold_energy)
                    keep += 1
        if diag is not None:
            diag["swap_acceptance"] = (took / tried).to(device=x.device, dtype=x.dtype)
            diag["acceptance_rate"] = (accepted / max(n * n_steps, 1)).to(device=x.device, dtype=x.dtype)
        return x, traj, diag

    # ---------------------------------------------------------------------------------
    # routes: one launch of ebm_tempering_hmc_chain_f32, or (fused_mlp) of ebm_tempering_hmc_mlp_chain_f32 -- the same parameter list
    # ---------------------------------------------------------------------------------
    def _ladder_on(self, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The three device arrays of the ladder, kept for the next call with the same step sizes."""
        key = (device, self._step_sizes(), self.temperatures)
        cached = getattr(self, "_ladder_cache", None)
        if cached is None or cached[0] != key:
            sqrt_temp, beta = hmc_ladder_coefficients(self.temperatures)
            eps = torch.tensor(key[1], dtype=torch.float32)
            cached = (key, eps.to(device), sqrt_temp.to(device), beta.to(device))
            self._ladder_cache = cached
        return cached[1], cached[2], cached[3]

    def _sample_fused(self, x, spec: FusedSpec, n_steps, thin, want_traj, want_diag, generator,
                      entry: str = "ebm_tempering_hmc_chain_f32"):
        n, R, dim = x.shape
        n_kept = n_steps // thin
        state = _lib.dense_f32(x).clone()  # the kernel updates in place; never the caller's tensor
        eps, sqrt_temp, beta = self._ladder_on(x.device)
        need_kept = (want_traj or want_diag) and n_kept > 0
        traj = torch.empty(n, n_kept, dim, dtype=torch.float32, device=x.device) if (want_traj or need_kept) else None
        # (uint32 counters in int32 tensors) accepted proposals per slot, then attempts and accepts per pair
        accepts = torch.zeros(R, dtype=torch.int32, device=x.device) if want_diag else None
        swaps = torch.zeros(2 * (R - 1), dtype=torch.int32, device=x.device) if want_diag else None
        seed, step0 = _rng.reserve(generator, x.device, 3 * n_steps)
        stream = _lib.stream_handle(x.device)
        spec_c = spec.to_c()
        if n > 0 and n_steps > 0:
            _lib.call(
                entry,
                spec_c, _lib.ptr(state), n, R, dim, n_steps, self.n_leapfrog_steps, _lib.ptr(eps), _lib.ptr(sqrt_temp), _lib.ptr(beta),
                self.swap_every, thin, _lib.ptr(traj) if need_kept else None, None, _lib.ptr(accepts), _lib.ptr(swaps),
                None, None, None, seed, step0, stream,
            )
        self.advance_schedulers(n_steps)
        diag = None
        if want_diag:
            diag = new_outputs(state, (n, dim), n_kept, False, True)[1]
            if n > 0 and n_kept > 0:
                if spec.kind == _lib.ENERGY_MLP:  # the kept states' statistics in torch ops, their energy the model's
                    for keep in range(n_kept):
                        record_kept(traj[:, keep], keep, None, diag, lambda x_: self._model_energy(x_.contiguous(), {}))
                else:
                    kept_statistics(spec_c, traj, diag, stream)
            c = (swaps.to(torch.int64) & 0xFFFFFFFF).to(torch.float64)
            diag["swap_acceptance"] = (c[R - 1 :] / c[: R - 1]).to(torch.float32)
            got = (accepts.to(torch.int64) & 0xFFFFFFFF).to(torch.float64)
            diag["acceptance_rate"] = (got / max(n * n_steps, 1)).to(torch.float32)
        return state, (traj if want_traj else None), diag
