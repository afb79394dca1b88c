r"""Hamiltonian Monte Carlo sampler (reference: torchebm/samplers/hmc.py:19-315).

Per transition: draw ``p ~ N(0, M)``; ``H0 = U(x) + K(p)``; ``L`` leapfrog steps in safe
mode; ``H1``; accept with probability ``min(1, exp(H0 - H1))``.  The RNG draw order per
transition is momentum normals, then the accept uniforms.

Execution routes (chosen once per ``sample()`` call):

``fused``  CUDA fp32 2-D state + analytic energy + default leapfrog: all transitions run
           inside ONE launch of ``ebm_hmc_chain_f32`` (per-chain energies are wavefront
           reductions, the accept decision never leaves the wave).
``step``   CUDA fp32, any other model: Philox momentum fill, ``LeapfrogIntegrator`` on the
           HIP kick kernels around ``model.gradient`` (autograd), HIP Metropolis kernel.
``eager``  CPU state, or configurations outside the hot path: the reference loop in torch.

``RiemannianManifoldHMC`` of the reference is out of scope.
"""

from __future__ import annotations

import math
from typing import Any, Dict, Optional, Tuple, Union

import torch

from .. import _lib, _rng
from ..core.energies import BaseModel, FusedSpec, fused_spec_for
from ..core.integrator_base import BaseSymplecticIntegrator
from ..core.module import graph_state_key, warn_once
from ..core.sampler_base import BaseSampler
from ..core.schedules import BaseScheduler
from ..integrators.registry import resolve_integrator
from ..integrators.symplectic import LeapfrogIntegrator, _mass_args
from ._chain_host import new_outputs, record_kept, run_with_records, run_with_state_passes, sample_graph, schedule_table, use_graph


class HamiltonianMonteCarlo(BaseSampler):
    """Hamiltonian Monte Carlo.

    Args:
        model: energy model.
        step_size: leapfrog step size (float or ``BaseScheduler``).
        n_leapfrog_steps: leapfrog steps per proposal.
        mass: ``None``, a float, or a per-dimension tensor.
        dtype, device: where the chains live.
        integrator: ``None`` (leapfrog), a registry name, or a separable
            ``BaseSymplecticIntegrator`` instance matching the sampler's device/dtype.
    """

    #: Opt-in, an ATTRIBUTE (``sampler.exact = True``; the constructor keeps the reference's signature, whose own tests pin
    #: ``integrator`` as its last parameter).
    #: ``False`` (default): the fused transition kernel's FAST leapfrog body -- merged half kicks, fused
    #: multiply-adds, ``eps / m`` hoisted: not less accurate than the reference's own fp32 run against an fp64 referee
    #: (medians 0.5 - 0.8x, tests/test_grid_gpu.py), identical accept decisions on every recorded fixture, but not the
    #: reference's operation sequence: after 200 leapfrog steps a quarter of the chains differ from the reference's
    #: states by more than 5e-4 (tests/test_hmc_audit_gpu.py reports the figure).  ``True``: the reference's safe-mode
    #: sequence LITERALLY (torchebm/samplers/hmc.py:243-312, integrators/leapfrog.py:156-185: separate half kicks, every
    #: multiply and add rounded on its own, the drift divided by ``max(m, 1e-10)`` per step, both scrubs, energy and
    #: force re-evaluated at the top of every transition).  For the element-wise energies (``DoubleWellModel``,
    #: ``HarmonicModel``; dim <= 256) that is one launch of the library's literal kernel -- given the same momenta and
    #: uniforms the states are the reference's bit for bit -- at 1.9x the fast body's time (2 L + 2 evaluations per
    #: transition instead of L; 1.18 against 0.61 ms at 2^18 x 32, L = 20, 10 transitions).  For every other energy
    #: ``exact=True`` takes the per-transition route: the reference's own torch operations around the HIP momentum /
    #: accept kernels.  (The in-kernel Philox field is the package's on every GPU route; ``exact`` is about the
    #: arithmetic between the draws.)
    exact: bool = False

    #: opt-in read by ``adapt_step_size`` of a sampler built with ``mass=``: an eligible call (CUDA fp32, an analytic energy,
    #: ``dim <= 256``, a constant step size, the plain leapfrog integrator) is ONE launch of ``ebm_ghmc_adapt_chain_mass_f32``
    #: (docs/design/adapt_mass.md).  Off by default: a massed sampler's ``adapt_step_size`` keeps the eager route and its bits.
    #: (``warmup()`` is new and takes the launch without it.)
    fused_adapt_mass = False

    #: energies the literal kernel (``ebm_hmc_chain_audit_f32``) takes, and its widest state
    _EXACT_KINDS = (_lib.ENERGY_DOUBLE_WELL, _lib.ENERGY_HARMONIC)
    _EXACT_MAX_DIM = 256

    def __init__(
        self,
        model: BaseModel,
        step_size: Union[float, BaseScheduler] = 1e-3,
        n_leapfrog_steps: int = 10,
        mass: Optional[Union[float, torch.Tensor]] = None,
        dtype: torch.dtype = torch.float32,
        device: Optional[Union[str, torch.device]] = None,
        integrator: Union[str, BaseSymplecticIntegrator, None] = None,
    ):
        super().__init__(model=model, dtype=dtype, device=device)
        self._register_param("step_size", step_size, positive=True)
        if n_leapfrog_steps <= 0:
            raise ValueError("n_leapfrog_steps must be positive")
        self.n_leapfrog_steps = n_leapfrog_steps
        if mass is not None and not isinstance(mass, float):
            mass = mass.to(self.device)
        self.mass = mass
        integ = resolve_integrator(
            integrator,
            default="leapfrog",
            family=BaseSymplecticIntegrator,
            owner="HamiltonianMonteCarlo",
            device=self.device,
            dtype=self.dtype,
        )
        if not integ.separable:
            raise TypeError(
                "HamiltonianMonteCarlo requires a separable symplectic integrator (drift/mass contract); "
                f"got non-separable {type(integ).__name__}. Use RiemannianManifoldHMC for non-separable "
                "Hamiltonians."
            )
        self.integrator = integ

    # ---------------------------------------------------------------------------------
    # momentum / kinetic energy in torch ops (eager + step routes; hmc.py:92-159)
    # ---------------------------------------------------------------------------------
    def _scale_momentum_(self, p: torch.Tensor) -> torch.Tensor:
        if self.mass is None:
            return p
        if isinstance(self.mass, float):
            return p.mul_(math.sqrt(self.mass))
        return p.mul_(torch.sqrt(self.mass).view((1,) * (p.ndim - 1) + (-1,)))

    def _initialize_momentum(self, shape: torch.Size, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``p ~ N(0, M)`` with torch's own generator stream (CPU / eager route)."""
        buf = getattr(self, "_momentum_buf", None)
        if buf is None or buf.shape != shape or buf.dtype != self.dtype or buf.device != self.device:
            buf = torch.empty(shape, dtype=self.dtype, device=self.device)
            self._momentum_buf = buf
        return self._scale_momentum_(buf.normal_(generator=generator))

    def _compute_kinetic_energy(self, p: torch.Tensor) -> torch.Tensor:
        """``K(p) = 0.5 p^T M^{-1} p`` per chain."""
        if self.mass is None:
            return 0.5 * torch.sum(p.square(), dim=-1)
        if isinstance(self.mass, float):
            return 0.5 * torch.sum(p.square(), dim=-1) / self.mass
        return 0.5 * torch.sum(p.square() / self.mass.view((1,) * (p.ndim - 1) + (-1,)), dim=-1)

    # ---------------------------------------------------------------------------------
    # routing
    # ---------------------------------------------------------------------------------
    def _route(self, x: torch.Tensor, model_kwargs: Dict[str, Any]) -> Tuple[str, Optional[FusedSpec]]:
        if not x.is_cuda:
            return "eager", None
        plain = type(self.integrator) is LeapfrogIntegrator
        if x.dtype != torch.float32 or not plain or (self.use_mixed_precision and self.autocast_available):
            warn_once(
                "hmc-eager-cuda",
                "torchebm_amd: HamiltonianMonteCarlo with a non-fp32 state, autocast, or a non-default integrator "
                "is not accelerated by the HIP kernels; running the eager torch loop on the GPU.",
                UserWarning,
            )
            return "eager", None
        spec = None
        mass_ok = self.mass is None or isinstance(self.mass, float) or (
            torch.is_tensor(self.mass) and self.mass.ndim == 1 and self.mass.numel() == x.shape[-1]
        )
        if mass_ok:
            spec = fused_spec_for(self.model, x, model_kwargs)
            if spec is not None and not spec.hmc:
                spec = None  # (a wide MLP energy: fused for Langevin only)
            if spec is not None and self.exact and not (spec.kind in self._EXACT_KINDS and x.shape[-1] <= self._EXACT_MAX_DIM):
                spec = None  # exact=True without a literal kernel for this energy: the reference's torch operations, per transition
            if (spec is not None and spec.kind == _lib.ENERGY_GAUSSIAN and spec.dim is not None
                    and spec.dim > 160  # (up to 160: the split operands stay in LDS -- five tiles; widths off multiples of 4 on shifted rows)
                    and not (spec.dim <= 256 and spec.aux is not None)  # (161 .. 256: the slabs stream from the pre-split image -- one per alignment class off multiples of 4, up to 254)
                    and x.shape[0] >= 16384 and self.capture_graph is not False and self._graph_eligible(model_kwargs)):
                # Above 256 dims (255 included) the transition kernel is the lane-group mat-vec (2 TFLOP/s); the per-transition route -- the
                # gradient and the energy as one library GEMM each (GaussianModel), kick / drift / accept kernels on the same
                # random field, replayed from a HIP graph -- is 1.5 - 30x faster there (scripts/bench_gauss_hmc_big.py), for
                # batches that fill the GEMMs and calls that can be replayed; otherwise the one fused launch is kept.
                spec = None
        return ("fused", spec) if spec is not None else ("step", None)

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
        reset_schedulers: bool = True,
        *,
        model_kwargs: Optional[Dict[str, Any]] = None,
        generator: Optional[torch.Generator] = None,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, Dict[str, torch.Tensor]]]:
        """Generate samples; ``n_steps`` is the number of MH proposals.

        Diagnostics keys: ``"mean"``, ``"var"`` (``[n_kept, dim]``), ``"energy"`` and
        ``"acceptance_rate"`` (``[n_kept]``).  ``dim`` is inferred from ``model.mean`` when
        neither ``x`` nor ``dim`` is given.

        Raises:
            ValueError: ``thin < 1``, or the state dimension cannot be determined.
        """
        if thin < 1:
            raise ValueError("thin must be >= 1")
        if reset_schedulers:
            self.reset_schedulers()
        model_kwargs = self._prepare_model_kwargs(model_kwargs)
        if x is None and dim is None:
            mean = getattr(self.model, "mean", None)
            if not isinstance(mean, torch.Tensor):
                raise ValueError("dim must be provided when x is None and cannot be inferred from model")
            dim = mean.shape[0]
        x = self._init_state(x, dim, n_samples, generator)
        route, spec = self._route(x, model_kwargs)
        if route == "fused":
            return self._sample_fused(x, spec, n_steps, thin, return_trajectory, return_diagnostics, generator)
        return self._sample_stepwise(
            x, model_kwargs, n_steps, thin, return_trajectory, return_diagnostics, generator, hip=(route == "step")
        )

    def sample_moments(
        self,
        x: Optional[torch.Tensor] = None,
        dim: Optional[int] = None,
        n_steps: int = 100,
        n_samples: int = 1,
        burn_in: int = 0,
        energy: bool = True,
        *,
        generator: Optional[torch.Generator] = None,
    ):
        """Run ``n_steps`` transitions and return ``(x_final, ChainMoments)``: per-chain time averages and sums of squared
        deviations over the two halves of the transitions behind ``burn_in`` (a rejected proposal counts the held state
        again) -- split R-hat, effective sample size and pooled posterior moments without a trajectory
        (``samplers/moments.py``).  ``energy=True`` (the default: the transition carries it) keeps the same for ``E(x)``;
        ``ChainMoments.acceptance_rate`` holds accepted / proposed per transition.

        ``n_steps - burn_in`` must be even: when it is odd, one more transition is burnt.  At least four counted
        transitions are needed (``ValueError``).  On the fused route (CUDA fp32, an analytic energy, ``dim <= 256``,
        constant step size, ``mass is None``, the plain leapfrog integrator) the call is ONE launch of
        ``ebm_chain_moments_f32``; anything else runs ``sample(n_steps=1)`` per transition around the same recurrence."""
        from .moments import sample_moments

        return sample_moments(self, True, x, dim, n_steps, n_samples, burn_in, energy, generator)

    def adapt_step_size(self, x=None, dim=None, n_steps=200, n_samples=1, target_accept=0.8, init_step_size=None, t0=10.0, gamma=0.05,
                        kappa=0.75, mu_factor=10.0, bounds=(1e-6, 1e3), velocity=None, generator=None, apply=True):
        """Find the leapfrog step size by dual averaging: ``GeneralizedHMC.adapt_step_size`` (its docstring) with a full momentum
        refresh and ``T = 1`` -- this sampler's transition.  Every chain adapts its own step size; the returned
        :class:`StepSizeAdaptation` carries them and their pooled value ``step_size``, which ``apply=True`` (ONE host read) makes
        the sampler's.  On the fused route (CUDA fp32, an analytic energy, ``dim <= 256``, ``mass is None``, a constant step size,
        the plain leapfrog integrator) the call is ONE launch of ``ebm_ghmc_adapt_chain_f32`` with ``gamma = inf``; anything else
        runs the recurrence in torch ops with the safe-mode leapfrog step, drawing ``randn(n, dim)`` for the (discarded) start
        velocities when none are passed, then ``randn(n, dim)`` and ``rand(n)`` per transition.  With the opt-in
        ``fused_adapt_mass`` a sampler with a mass is ONE launch too, of ``ebm_ghmc_adapt_chain_mass_f32``.

        Raises:
            ValueError: a symplectic integrator other than the plain leapfrog (the recurrence spells that step), or what
                ``GeneralizedHMC.adapt_step_size`` refuses.
        """
        from .adapt import adapt_step_size

        if type(self.integrator) is not LeapfrogIntegrator:
            raise ValueError("adapt_step_size needs the plain leapfrog integrator")
        return adapt_step_size(self, math.inf, 1.0, x, dim, n_steps, n_samples, target_accept, init_step_size, t0, gamma, kappa,
                               mu_factor, bounds, velocity, generator, apply)

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
            ValueError: fewer than 2 rows (the variance is an ensemble estimate across chains), a symplectic integrator other than the plain leapfrog, or what
                ``adapt_step_size`` refuses.
        """
        from .warmup import warmup

        return warmup(self, x, dim, n_samples, windows, final_steps, target_accept, regularize, generator, apply,
                      **dual_averaging_constants)

    # ---------------------------------------------------------------------------------
    # route: per-transition loop
    # ---------------------------------------------------------------------------------
    def _sample_stepwise(self, x, model_kwargs, n_steps, thin, want_traj, want_diag, generator, hip: bool):
        n, dim = x.shape[0], x.shape[1]
        traj, diag = new_outputs(self, (n, dim), n_steps // thin, want_traj, want_diag, acceptance=True)
        drift = lambda x_, t_: -self._model_gradient(x_, model_kwargs)  # noqa: E731
        energy = lambda x_: self._model_energy(x_, model_kwargs).clamp_(min=-1e10, max=1e10)  # noqa: E731
        if hip and n > 0 and self._use_graph(model_kwargs, n_steps):
            return sample_graph(self, x, n_steps, thin, traj, diag, generator, 2, energy)
        if hip:
            x = _lib.dense_f32(x)
            seed, step0 = _rng.reserve(generator, x.device, 2 * n_steps)
            stream = _lib.stream_handle(x.device)
            row_dim = x.numel() // max(n, 1)
        keep = 0
        with self.autocast_context():
            for i in range(n_steps):
                if hip:
                    p = torch.empty_like(x)
                    _lib.call("ebm_noise_fill_f32", _lib.ptr(p), p.numel(), _lib.NOISE_NORMAL, seed, step0 + 2 * i, stream)
                    p = self._scale_momentum_(p)
                else:
                    p = self._initialize_momentum(x.shape, generator)

                h0 = self._model_energy(x, model_kwargs).clamp_(min=-1e10, max=1e10) + self._compute_kinetic_energy(
                    p
                ).clamp_(min=0.0, max=1e10)
                self.integrator.carry_force = bool(self.carry_force)
                prop = self.integrator.integrate(
                    {"x": x, "p": p},
                    step_size=self.get_scheduled_value("step_size"),
                    n_steps=self.n_leapfrog_steps,
                    mass=self.mass,
                    drift=drift,
                    safe=True,
                )
                x_prop, p_prop = prop["x"], prop["p"]
                h1 = self._model_energy(x_prop, model_kwargs).clamp_(min=-1e10, max=1e10) + self._compute_kinetic_energy(
                    p_prop
                ).clamp_(min=0.0, max=1e10)

                if hip:
                    mask = torch.empty(n, dtype=torch.uint8, device=x.device)
                    x_next = x.clone()
                    # locals keep any dense copies alive until the launch that reads them is enqueued
                    xp_d, h0_d, h1_d = _lib.dense_f32(x_prop), _lib.dense_f32(h0), _lib.dense_f32(h1)
                    _lib.call(
                        "ebm_hmc_accept_f32",
                        _lib.ptr(x_next), _lib.ptr(xp_d), _lib.ptr(h0_d), _lib.ptr(h1_d), None, _lib.ptr(mask), None,
                        n, row_dim, seed, step0 + 2 * i + 1, stream,
                    )
                    x = x_next
                    accepted = mask
                else:
                    delta = (h0 - h1).clamp_(min=-50.0, max=50.0)
                    accept_prob = torch.exp(delta).clamp_(max=1.0)
                    u = torch.rand(n, device=self.device, generator=generator)
                    accepted = u < accept_prob
                    x = torch.where(accepted.view(-1, *([1] * (x.ndim - 1))), x_prop, x)

                if (i + 1) % thin == 0:
                    record_kept(x, keep, traj, diag, energy, accepted)
                    keep += 1
                self.step_schedulers()
        out = traj if want_traj else x
        return (out, diag) if want_diag else out

    # ---------------------------------------------------------------------------------
    # route: one transition of the step route captured in a HIP graph (the default whenever eligible)
    # ---------------------------------------------------------------------------------
    #: Capture ONE Metropolis transition of the step route -- momentum draw, H0, L leapfrog steps (kick /
    #: autograd gradient / kick), H1, accept -- into a HIP graph and replay it n_steps times.  With an
    #: nn.Module energy a transition is ~15 small launches per leapfrog step; a replay is one submission.
    #: The Philox coordinates live in a device buffer the graph advances by 2 per transition
    #: (``ebm_noise_fill_dev_f32`` at +0, ``ebm_hmc_accept_dev_f32`` at +1), so the generator contract and
    #: the noise field are those of the eager step route, bit for bit.  Requirements: constant step
    #: size, no conditioning, a model whose forward is static-shape and free of host-side randomness.
    #: ``None`` (default): replay whenever eligible, the call has at least ``GRAPH_MIN_STEPS`` transitions and the first
    #: (eager) transition showed no side effect of the model's forward; ``True``: whenever eligible; ``False``: never.
    #: See ``LangevinDynamics.capture_graph`` for the rules (first transition eager = the warm-up, thread-local capture,
    #: per-configuration refusal).
    capture_graph: Optional[bool] = None
    GRAPH_MIN_STEPS = 4
    #: Step route only (the fused kernels always do this, bit-identically): reuse the force a leapfrog step ends on as
    #: the force the next one starts from -- L + 1 gradient evaluations per transition instead of the reference's 2 L,
    #: i.e. 1.8x fewer autograd round trips at L = 10.  Off by default because it is observable in two corners: an
    #: energy whose forward is stochastic (dropout in training mode, RNG calls) sees half as many evaluations, and a
    #: chain whose position had to be scrubbed in safe mode keeps the unscrubbed position's force for one step.
    carry_force: bool = False

    def _graph_eligible(self, model_kwargs: Dict[str, Any]) -> bool:
        return not model_kwargs and not self.use_mixed_precision and self.schedulers["step_size"].is_constant()

    _use_graph = use_graph

    def _graph_for(self, x: torch.Tensor):
        eps = self.get_scheduled_value("step_size")
        key = (
            tuple(x.shape), x.device, eps, self.n_leapfrog_steps, id(self.integrator), bool(self.carry_force),
            None if self.mass is None else (self.mass if isinstance(self.mass, float) else self.mass.data_ptr()),
            graph_state_key(self.model),
        )
        cached = getattr(self, "_step_graph", None)
        if cached is not None and cached["key"] == key:
            return cached
        n = x.shape[0]
        row_dim = x.numel() // n
        state = torch.empty_like(x)                                        # static buffers of the graph
        rng = torch.zeros(2, dtype=torch.int64, device=x.device)           # {seed, step} as raw 64-bit patterns
        mask = torch.zeros(n, dtype=torch.uint8, device=x.device)
        drift = lambda x_, t_: -self._model_gradient(x_, {})  # noqa: E731

        def body():
            stream = _lib.stream_handle(x.device)
            p = torch.empty_like(state)
            _lib.call("ebm_noise_fill_dev_f32", _lib.ptr(p), p.numel(), _lib.NOISE_NORMAL, _lib.ptr(rng), 0, stream)
            p = self._scale_momentum_(p)
            h0 = self._model_energy(state, {}).clamp_(min=-1e10, max=1e10) + self._compute_kinetic_energy(p).clamp_(
                min=0.0, max=1e10)
            self.integrator.carry_force = bool(self.carry_force)
            prop = self.integrator.integrate(
                {"x": state, "p": p}, step_size=eps, n_steps=self.n_leapfrog_steps, mass=self.mass, drift=drift, safe=True)
            h1 = self._model_energy(prop["x"], {}).clamp_(min=-1e10, max=1e10) + self._compute_kinetic_energy(
                prop["p"]).clamp_(min=0.0, max=1e10)
            xp_d, h0_d, h1_d = _lib.dense_f32(prop["x"]), _lib.dense_f32(h0), _lib.dense_f32(h1)
            _lib.call(
                "ebm_hmc_accept_dev_f32",
                _lib.ptr(state), _lib.ptr(xp_d), _lib.ptr(h0_d), _lib.ptr(h1_d), _lib.ptr(mask), None,
                n, row_dim, _lib.ptr(rng), 1, stream,
            )
            rng[1:2].add_(2)

        self._step_graph = {"key": key, "graph": None, "state": state, "rng": rng, "mask": mask, "body": body}
        return self._step_graph

    # ---------------------------------------------------------------------------------
    # route: fused HIP kernel
    # ---------------------------------------------------------------------------------
    def _launch_hmc(self, spec_c, state, n, dim, eps_vals, t0, n_mh, thin, traj, counts, seed, step, stream, records=None):
        kind, m_scalar, m_diag = _mass_args(self.mass, state)
        if len(eps_vals) == 1:
            eps, table = eps_vals[0], None
        else:
            eps = eps_vals[t0]
            table = schedule_table(self, eps_vals, state.device)[t0 : t0 + n_mh]
        cptr = None if counts is None else counts.data_ptr() + 4 * t0
        if self.exact:  # the literal body (no in-kernel records: `_sample_fused` asks for none)
            assert records is None
            _lib.call(
                "ebm_hmc_chain_audit_f32",
                spec_c, _lib.ptr(state), n, dim, n_mh, self.n_leapfrog_steps, eps, _lib.ptr(table),
                kind, m_scalar, _lib.ptr(m_diag), thin, _lib.ptr(traj), None, cptr, None, None,
                seed, step, stream,
            )
            return
        _lib.call(
            "ebm_hmc_chain_f32",
            spec_c, _lib.ptr(state), n, dim, n_mh, self.n_leapfrog_steps, eps, _lib.ptr(table),
            kind, m_scalar, _lib.ptr(m_diag), thin, _lib.ptr(traj), _lib.ptr(records), None, cptr, None, None,
            seed, step, stream,
        )

    #: see LangevinDynamics.donate_input / DIAG_RECORD_BYTES
    donate_input: bool = False
    DIAG_RECORD_BYTES = 1 << 30

    def _sample_fused(self, x, spec: FusedSpec, n_steps, thin, want_traj, want_diag, generator):
        n, dim = x.shape
        n_kept = n_steps // thin
        state = _lib.dense_f32(x)
        if state.data_ptr() == x.data_ptr() and not self.donate_input:
            state = state.clone()  # the kernel updates in place; never touch the caller's tensor unless it was donated
        traj, diag = new_outputs(self, (n, dim), n_kept, want_traj, want_diag, acceptance=True)
        sched = self.schedulers["step_size"]
        eps_vals = [sched.get_value()] if sched.is_constant() else sched.preview(n_steps)
        seed, step0 = _rng.reserve(generator, x.device, 2 * n_steps)
        stream = _lib.stream_handle(x.device)
        spec_c = spec.to_c()

        if n_steps > 0 and n > 0:
            if not want_diag or n_kept == 0:
                self._launch_hmc(spec_c, state, n, dim, eps_vals, 0, n_steps, thin, traj, None, seed, step0, stream)
            else:
                layout = None if self.exact else _lib.diag_layout(spec_c, _lib.DIAG_HMC, n, dim, False, want_traj)
                self._fused_with_diagnostics(spec_c, state, eps_vals, n_steps, thin, traj, diag, layout, seed, step0, stream)
        self.advance_schedulers(n_steps)
        out = traj if want_traj else state
        return (out, diag) if want_diag else out

    def _fused_with_diagnostics(self, spec_c, state, eps_vals, n_steps, thin, traj, diag, layout, seed, step0, stream):
        """With a ``layout``, diagnostics from inside the transition kernel: at every kept transition each workgroup stores
        one record (column sums / M2, the energy of the states its chains hold, its accept count) and
        ``ebm_diag_finish_f32`` merges them (``_chain_host.run_with_records``).  Without one (the MLP energy's
        matrix-layout kernel, ``exact``): one launch per ``thin`` transitions, each leaving its accepted proposals per
        transition in ``counts`` (uint32 bit patterns; the trailing launch counts nothing), then the column-statistics
        and energy kernels on the state (``_chain_host.run_with_state_passes``)."""
        n, dim = state.shape
        counts = None if layout is not None else torch.zeros(n_steps, dtype=torch.int32, device=state.device)
        kept_end = n_steps // thin * thin

        def launch(t0, n_mh, piece, records, first):
            self._launch_hmc(spec_c, state, n, dim, eps_vals, t0, n_mh, thin, piece, counts if t0 < kept_end else None,
                             seed, step0 + 2 * t0, stream, records=records)

        if layout is not None:
            run_with_records(self, state, n_steps, thin, traj, diag, layout, stream, launch)
            return
        energy = torch.empty(n, dtype=torch.float32, device=state.device)

        def mean_energy():
            _lib.call("ebm_energy_grad_f32", spec_c, _lib.ptr(state), n, dim, _lib.ptr(energy), None, stream)
            return energy.clamp_(min=-1e10, max=1e10).mean()

        run_with_state_passes(state, n_steps, thin, traj, diag, stream, launch, mean_energy, counts)
