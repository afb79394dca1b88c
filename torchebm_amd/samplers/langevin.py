r"""Langevin dynamics sampler (reference: torchebm/samplers/langevin_dynamics.py:16-188).

.. math:: x_{t+1} = x_t - \eta \nabla_x U(x_t) + \sqrt{2\eta}\,\sigma\,\epsilon_t

Three execution routes, chosen once per ``sample()`` call:

``fused``  CUDA fp32 state + one of the analytic energies + default Euler-Maruyama
           integrator: the whole k-step loop (gradient, update, Philox noise, clamp, thinned
           trajectory) is ONE launch of ``ebm_langevin_chain_f32``; schedulers are
           pre-expanded on the host into a per-step coefficient table.
``step``   CUDA fp32 state, any other model (e.g. an MLP energy, conditioning): the gradient
           comes from ``model.gradient`` (autograd) and each step is one launch of
           ``ebm_langevin_step_f32`` (update + noise + clamp fused).
``eager``  CPU state (BASELINE config 1) -- or a configuration outside the hot path
           (non-fp32, non-default integrator): the reference's loop with eager torch ops.

A CUDA state never silently runs on the CPU and never skips the HIP library: ``fused`` and
``step`` raise if ``libebm_hip.so`` is missing.
"""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple, Union

import torch

from .. import _lib, _rng
from ..core.energies import BaseModel, FusedSpec, fused_spec_for
from ..core.integrator_base import BaseSDERungeKuttaIntegrator
from ..core.module import graph_state_key, warn_once
from ..core.sampler_base import BaseSampler
from ..core.schedules import BaseScheduler
from ..integrators.em import EulerMaruyamaIntegrator, HeunIntegrator
from ..integrators.registry import resolve_integrator
from ._chain_host import _CAPTURE_LOCK  # noqa: F401  (the one capture lock: utils.graphed_step takes it from here)
from ._chain_host import new_outputs, record_kept, run_with_records, run_with_state_passes, sample_graph, schedule_table, use_graph


def em_coefficients(eta: float, sigma: float) -> Tuple[float, float, float]:
    """The three scalars of one Euler-Maruyama step, computed in double exactly as the
    reference's Python-float arithmetic does (base_integrator.py:728-729): they are cast to
    fp32 only when they enter the tensor ops / the kernel."""
    return eta, eta**0.5, (2.0 * sigma**2) ** 0.5


WIDE_GAUSSIAN_STEP_ROUTE_MIN_CHAINS = 16384  # below: k x (GEMM + update) launches lose to the one fused launch


def _gaussian_chain_on_matrix_cores(dim: int) -> bool:
    """Widths at which ``ebm_langevin_chain_f32`` runs the dense Gaussian on the matrix cores (csrc/gauss_mfma.hip: up to 128,
    packed rows below 20 included; csrc/gauss_shift.hip, gauss_res_shift.hip: widths off multiples of 4 up to 254 on shifted rows;
    csrc/gauss_big.hip: multiples of 4 up to 512)."""
    return dim <= 254 or (dim % 4 == 0 and dim <= 512)


class LangevinDynamics(BaseSampler):
    """Langevin dynamics sampler.

    Args:
        model: energy model to sample from.
        step_size: step size, a float or a ``BaseScheduler``.
        noise_scale: noise scale, a float or a ``BaseScheduler``.
        decay: stored, unused (as in the reference).
        clamp: optional ``(min, max)`` applied to the state after every step.
        dtype, device: where the chains live.
        integrator: ``None`` (Euler-Maruyama), a registry name, or a
            ``BaseSDERungeKuttaIntegrator`` instance matching the sampler's device/dtype.
    """

    def __init__(
        self,
        model: BaseModel,
        step_size: Union[float, BaseScheduler] = 1e-3,
        noise_scale: Union[float, BaseScheduler] = 1.0,
        decay: float = 0.0,
        clamp: Optional[Tuple[float, float]] = None,
        dtype: torch.dtype = torch.float32,
        device: Optional[Union[str, torch.device]] = None,
        integrator: Union[str, BaseSDERungeKuttaIntegrator, None] = None,
    ):
        super().__init__(model=model, dtype=dtype, device=device)
        self._register_param("step_size", step_size, positive=True)
        self._register_param("noise_scale", noise_scale, positive=True)
        if clamp is not None and clamp[0] >= clamp[1]:
            raise ValueError(f"clamp min must be < max, got {clamp}")
        self.clamp = clamp
        self.decay = decay
        self.integrator = resolve_integrator(
            integrator,
            default="euler_maruyama",
            family=BaseSDERungeKuttaIntegrator,
            owner="LangevinDynamics",
            device=self.device,
            dtype=self.dtype,
        )

    # ---------------------------------------------------------------------------------
    # routing
    # ---------------------------------------------------------------------------------
    def _route(self, x: torch.Tensor, model_kwargs: Dict[str, Any]) -> Tuple[str, Optional[FusedSpec]]:
        if not x.is_cuda:
            return "eager", None
        plain_em = type(self.integrator) is EulerMaruyamaIntegrator
        heun = type(self.integrator) is HeunIntegrator
        if heun and x.dtype == torch.float32 and not (self.use_mixed_precision and self.autocast_available):
            # Heun has a fused kernel for the analytic energies only; anything else keeps the eager loop
            spec = self._fusable_spec(x, model_kwargs)
            if spec is not None and not spec.langevin_only:
                return "fused", spec
        if x.dtype != torch.float32 or not plain_em or (self.use_mixed_precision and self.autocast_available):
            warn_once(
                "langevin-eager-cuda",
                "torchebm_amd: LangevinDynamics with a non-fp32 state, autocast, or a non-default integrator is "
                "not accelerated by the HIP kernels; running the eager torch loop on the GPU.",
                UserWarning,
            )
            return "eager", None
        spec = self._fusable_spec(x, model_kwargs)
        if (spec is not None and spec.kind == _lib.ENERGY_GAUSSIAN and not _gaussian_chain_on_matrix_cores(spec.dim)
                and x.shape[0] >= WIDE_GAUSSIAN_STEP_ROUTE_MIN_CHAINS and self.capture_graph is not False
                and self._graph_eligible(model_kwargs)):
            # The chain kernels for these widths (not a multiple of 4 above 128, or above 512) are the lane-group mat-vec:
            # 2 TFLOP/s.  The step route -- one library GEMM for the gradient (GaussianModel._hip_gradient) and the fused
            # update kernel on the same random field, replayed from a HIP graph -- is 10 - 40x faster there, for batches
            # that fill the GEMM and calls that can be replayed.  Few chains, capture_graph = False, a scheduled step size
            # or conditioning keep the ONE fused launch (with its in-kernel records and donate_input).
            return "step", None
        return ("fused", spec) if spec is not None else ("step", None)

    def _fusable_spec(self, x: torch.Tensor, model_kwargs: Dict[str, Any]) -> Optional[FusedSpec]:
        # element-wise energies run on the flat kernel, which has no row-width limit
        return fused_spec_for(self.model, x, model_kwargs, cap_elementwise=False)

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
        model_kwargs: Optional[Dict[str, Any]] = None,
        generator: Optional[torch.Generator] = None,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, Dict[str, torch.Tensor]]]:
        """Generate samples.

        Returns the final state ``[n, *shape]`` (or, with ``return_trajectory``, the kept
        trajectory ``[n, n_steps // thin, *shape]``), optionally with a diagnostics dict
        holding ``"mean"``/``"var"`` (``[n_kept, *shape]``) and ``"energy"`` (``[n_kept]``).

        Raises:
            ValueError: ``thin < 1``, or ``x`` and ``dim`` both ``None``.
        """
        if thin < 1:
            raise ValueError("thin must be >= 1")
        if reset_schedulers:
            self.reset_schedulers()
        x = self._init_state(x, dim, n_samples, generator)
        model_kwargs = self._prepare_model_kwargs(model_kwargs)
        route, spec = self._route(x, model_kwargs)
        if route == "fused":
            return self._sample_fused(x, spec, n_steps, thin, return_trajectory, return_diagnostics, generator)
        return self._sample_stepwise(
            x, model_kwargs, n_steps, thin, return_trajectory, return_diagnostics, generator, hip=(route == "step")
        )

    def sample_moments(
        self,
        x: Optional[torch.Tensor] = None,
        dim: Optional[Union[int, Tuple[int, ...]]] = None,
        n_steps: int = 100,
        n_samples: int = 1,
        burn_in: int = 0,
        energy: bool = False,
        *,
        generator: Optional[torch.Generator] = None,
    ):
        """Run ``n_steps`` steps and return ``(x_final, ChainMoments)``: per-chain time averages and sums of squared
        deviations over the two halves of the steps behind ``burn_in`` -- split R-hat, effective sample size and pooled
        posterior moments without a trajectory (``samplers/moments.py``).  ``energy=True`` keeps the same for ``E(x)``.

        ``n_steps - burn_in`` must be even: when it is odd, one more step is burnt.  At least four counted steps are needed
        (``ValueError``).  Schedulers are reset first, as in ``sample()``.  On the fused route (CUDA fp32, an analytic
        energy, ``dim <= 256``, constant step size and noise scale, no clamp) the call is ONE launch of
        ``ebm_chain_moments_f32`` and, for the element-wise energies, ``x_final`` is ``sample()``'s for the same generator
        state bit for bit; with the opt-in ``fused_mlp_moments`` an eligible ``MLPEnergy`` call is ONE launch of
        ``ebm_chain_moments_mlp_f32``; anything else runs ``sample(n_steps=1)`` per step around the same recurrence."""
        from .moments import sample_moments

        return sample_moments(self, False, x, dim, n_steps, n_samples, burn_in, energy, generator)

    # ---------------------------------------------------------------------------------
    # shared helpers
    # ---------------------------------------------------------------------------------
    def _clamp_args(self) -> Tuple[int, float, float]:
        if self.clamp is None:
            return 0, 0.0, 0.0
        return 1, float(self.clamp[0]), float(self.clamp[1])

    # ---------------------------------------------------------------------------------
    # route: per-step loop (eager torch ops, or the per-step HIP kernel)
    # ---------------------------------------------------------------------------------
    def _sample_stepwise(self, x, model_kwargs, n_steps, thin, want_traj, want_diag, generator, hip: bool):
        traj, diag = new_outputs(self, x.shape, n_steps // thin, want_traj, want_diag)
        energy = lambda x_: self._model_energy(x_, model_kwargs)  # noqa: E731
        keep = 0
        if hip and self._use_graph(model_kwargs, n_steps):
            return sample_graph(self, x, n_steps, thin, traj, diag, generator, 1, energy)
        if hip:
            x = _lib.dense_f32(x)
            seed, step0 = _rng.reserve(generator, x.device, n_steps)
            stream = _lib.stream_handle(x.device)
            clamp_on, cmin, cmax = self._clamp_args()
        else:
            drift = lambda x_, t_: -self._model_gradient(x_, model_kwargs)  # noqa: E731
        with self.autocast_context():
            for i in range(n_steps):
                eta = self.get_scheduled_value("step_size")
                sigma = self.get_scheduled_value("noise_scale")
                if hip:
                    grad = _lib.dense_f32(self._model_gradient(x, model_kwargs))
                    out = torch.empty_like(x)
                    a, sq, coef = em_coefficients(eta, sigma)
                    _lib.call(
                        "ebm_langevin_step_f32",
                        _lib.ptr(x), _lib.ptr(grad), _lib.ptr(out), None, x.numel(),
                        a, sq, coef, clamp_on, cmin, cmax, seed, step0 + i, stream,
                    )
                    x = out
                else:
                    x = self.integrator.step(
                        state={"x": x}, step_size=eta, noise_scale=sigma, drift=drift, generator=generator
                    )["x"]
                    if self.clamp is not None:
                        x = x.clamp_(*self.clamp)
                self.step_schedulers()

                if (i + 1) % thin == 0:
                    record_kept(x, keep, traj, diag, energy)
                    keep += 1
        out = traj if want_traj else x
        return (out, diag) if want_diag else out

    # ---------------------------------------------------------------------------------
    # route: per-step loop replayed from a HIP graph (the default whenever the configuration is eligible)
    # ---------------------------------------------------------------------------------
    #: Capture one "autograd gradient + fused update" iteration of the step route into a HIP graph and
    #: replay it n_steps times.  The step route is launch-bound (BASELINE config 5: ~13 small
    #: kernels per Langevin step): a replay costs one submission instead of 13.  The Philox
    #: coordinates live in a device buffer advanced inside the graph (``ebm_langevin_step_dev_f32``), so
    #: every replay draws fresh noise and the generator contract is unchanged; the result is bit-identical
    #: to the eager step route.
    #:   ``None`` (default)  replay whenever the call is eligible -- constant step size / noise scale, no conditioning, no
    #:                       autocast, at least ``GRAPH_MIN_STEPS`` steps -- AND capturing has no observable side effect:
    #:                       the first step of the call runs eagerly (it is the warm-up; nothing is evaluated that the
    #:                       eager route would not evaluate), and the graph is captured behind it only if that step
    #:                       wrote no buffer of the model (BatchNorm statistics in training mode), drew nothing from the
    #:                       default CUDA / CPU generators (dropout) and changed no attribute (``core.module.ForwardProbe``),
    #:                       and the model holds no attribute the cache key cannot see into
    #:                       (``core.module.graph_blind_spots``); otherwise the call continues with eager launches.
    #:                       The graph is kept for the next call and re-captured when the batch shape, the coefficients
    #:                       or the model's state key (``core.module.graph_state_key``: parameter / buffer storages, every
    #:                       hashable attribute of every submodule incl. tensor-valued ones, ``training``, autocast)
    #:                       change.  A forward that cannot be captured (host sync, data-dependent control flow) continues
    #:                       with eager launches with a one-time warning; only THAT configuration is remembered as
    #:                       uncapturable.  Capture uses ``capture_error_mode="thread_local"``: work other threads
    #:                       submit meanwhile (a DataLoader's pinning thread) neither breaks it nor is broken by it.
    #:                       Blind spots that remain: state reached through a closure or a global, tensors replaced
    #:                       inside containers the key hashes by storage, side effects outside the model.
    #:   ``True``            capture whenever eligible, without the minimum step count and without the side-effect checks.
    #:   ``False``           always eager launches.
    capture_graph: Optional[bool] = None
    GRAPH_MIN_STEPS = 8

    _use_graph = use_graph

    def _graph_eligible(self, model_kwargs: Dict[str, Any]) -> bool:
        return (
            not model_kwargs
            and not self.use_mixed_precision
            and self.schedulers["step_size"].is_constant()
            and self.schedulers["noise_scale"].is_constant()
        )

    def _graph_for(self, x: torch.Tensor):
        """The replay state for this (batch shape, coefficients, model state): static buffers + the step body; the graph
        itself is captured by ``_chain_host.sample_graph`` behind the first eager step."""
        a, sq, coef = em_coefficients(self.get_scheduled_value("step_size"), self.get_scheduled_value("noise_scale"))
        key = (
            tuple(x.shape), x.device, (a, sq, coef), self._clamp_args(),
            graph_state_key(self.model),
        )
        cached = getattr(self, "_step_graph", None)
        if cached is not None and cached["key"] == key:
            return cached
        state = torch.empty_like(x)                                        # static buffers of the graph
        rng = torch.zeros(2, dtype=torch.int64, device=x.device)           # {seed, step} as raw 64-bit patterns
        clamp_on, cmin, cmax = self._clamp_args()

        def body():
            grad = _lib.dense_f32(self._model_gradient(state, {}))
            _lib.call(
                "ebm_langevin_step_dev_f32",
                _lib.ptr(state), _lib.ptr(grad), _lib.ptr(state), state.numel(), a, sq, coef,
                clamp_on, cmin, cmax, _lib.ptr(rng), _lib.stream_handle(x.device),
            )
            rng[1:2].add_(1)

        self._step_graph = {"key": key, "graph": None, "state": state, "rng": rng, "body": body}
        return self._step_graph

    # ---------------------------------------------------------------------------------
    # route: k-fused HIP kernel
    # ---------------------------------------------------------------------------------
    def _coef_rows(self, k: int) -> Tuple[bool, List[Tuple[float, float, float]]]:
        """Pre-expand the two schedulers for the next k steps (values are read before
        ``step_schedulers()`` in the reference loop, i.e. at step counts 0..k-1)."""
        s_eta, s_sig = self.schedulers["step_size"], self.schedulers["noise_scale"]
        constant = s_eta.is_constant() and s_sig.is_constant()
        if constant:
            return True, [em_coefficients(s_eta.get_value(), s_sig.get_value())]
        etas, sigmas = s_eta.preview(k), s_sig.preview(k)
        return False, [em_coefficients(e, s) for e, s in zip(etas, sigmas)]

    def _launch_chain(self, spec_c, x, n, dim, rows, row0, k, thin, traj, seed, step, stream, table=None, records=None, src=None):
        """One ``ebm_langevin_chain_f32`` launch for steps [row0, row0+k) of ``rows``.  With ``src`` (the first launch of an
        out-of-place call, plain Euler-Maruyama only) the chains start from ``src`` and ``x`` is only written:
        ``ebm_langevin_chain_from_f32``, the same launch and the same states."""
        clamp_on, cmin, cmax = self._clamp_args()
        if len(rows) == 1:  # constant schedule: scalars, no table
            a, sq, coef = rows[0]
            tab = None
        else:
            a, sq, coef = rows[row0]
            tab = (schedule_table(self, rows, x.device) if table is None else table)[row0 : row0 + k]
        coords = getattr(self, "_graph_coords", None)
        if coords is not None:  # being captured in a HIP graph: `step` is an offset from the device-resident coordinates
            _lib.call(
                "ebm_langevin_chain_dev_f32",
                spec_c, _lib.ptr(x), n, dim, k, a, sq, coef, _lib.ptr(tab),
                clamp_on, cmin, cmax, thin, _lib.ptr(traj), _lib.ptr(coords.tensor), step, stream,
            )
            return
        flags = clamp_on | (_lib.CHAIN_CONTRACTED if self.fused_arithmetic else 0)  # (ABI 8: a flag word; the bit is a permission)
        if src is not None:
            _lib.call(
                "ebm_langevin_chain_from_f32",
                spec_c, _lib.ptr(src), _lib.ptr(x), n, dim, k, a, sq, coef, _lib.ptr(tab),
                flags, cmin, cmax, thin, _lib.ptr(traj), _lib.ptr(records), None, seed, step, stream,
            )
            return
        entry = "ebm_langevin_heun_chain_f32" if type(self.integrator) is HeunIntegrator else "ebm_langevin_chain_f32"
        _lib.call(
            entry,
            spec_c, _lib.ptr(x), n, dim, k, a, sq, coef, _lib.ptr(tab),
            flags, cmin, cmax, thin, _lib.ptr(traj), _lib.ptr(records), None, seed, step, stream,
        )

    #: Opt-in (an ATTRIBUTE, ``sampler.fused_arithmetic = True``: the constructor keeps the reference's signature, whose own tests pin
    #: ``integrator`` as its last parameter).  ``False``: every kernel rounds each multiply and add of the update on its own, as the
    #: reference's eager torch operations do (core/base_integrator.py:711-731) -- chains are the reference's bit for bit given the
    #: same draws.  ``True`` PERMITS contracted arithmetic where a kernel has that form (the element-wise energies' plain k-step call:
    #: ``x^2 - b^2`` and ``x - eta g`` as fused multiply-adds, ``noise_scale``'s coefficient times ``sqrt(step_size)`` folded into the
    #: Box-Muller radius): the same Philox draws and the same law, states that differ from the default's in the last bits of every
    #: step, 12 % more chain-steps per second on BASELINE config 2 (``EBM_CHAIN_CONTRACTED``, include/ebm_hip.h; bench.py
    #: ``config2_fused_arithmetic``).  Calls without such a kernel run the default arithmetic.
    fused_arithmetic: bool = False

    #: Opt-in, read by ``sample_moments`` only: an ``MLPEnergy`` call that ``sample()`` runs fused (hidden 64 / 128,
    #: ``dim == in_dim <= 128``, CUDA fp32, constant step size and noise scale, no clamp, plain Euler-Maruyama, no autocast) is ONE
    #: launch of ``ebm_chain_moments_mlp_f32`` (docs/design/langevin_moments_mlp.md) instead of ``n_steps`` calls of
    #: ``sample(n_steps=1)``.  Off by default: the energies become the kernel's split-bf16 / exact-f32 values, not autograd's, and
    #: the gradient comes from the general walk evaluation, not from the Langevin chain kernels ``sample()`` runs on the MLP --
    #: ``x_final`` is ``sample()``'s draw for draw and operation for operation in the update, but not guaranteed bit for bit.
    fused_mlp_moments = False

    #: Opt-in: let the fused route update the caller's ``x`` in place and return it.  Off by default: the reference never
    #: mutates its input.  For the plain Euler-Maruyama call this saves the allocation of the returned state (256 MiB at
    #: BASELINE config 2), not a copy: the default call reads the caller's tensor and writes a fresh one in the same launch
    #: (``ebm_langevin_chain_from_f32``).  Heun calls and calls captured by ``utils.GraphedTrainingStep`` still copy first.
    donate_input: bool = False

    #: upper bound on the bytes of per-block diagnostics records held at once; longer runs are cut into several
    #: launches at kept-step boundaries (the state is re-read once per cut)
    DIAG_RECORD_BYTES = 1 << 30

    def _sample_fused(self, x, spec: FusedSpec, n_steps, thin, want_traj, want_diag, generator):
        n, dim = x.shape
        n_kept = n_steps // thin
        state = _lib.dense_f32(x)
        coords = getattr(self, "_graph_coords", None)
        heun = type(self.integrator) is HeunIntegrator
        src = None  # the caller's tensor as the read-only start state of the call's first launch
        if state.data_ptr() == x.data_ptr() and not self.donate_input:
            # Never touch the caller's tensor unless it was donated.  The plain Euler-Maruyama call starts from it out of place
            # (ebm_langevin_chain_from_f32) and writes a fresh tensor, which only a launch fills: a call without one keeps the
            # copy.  So do Heun (ebm_langevin_heun_chain_f32 has no out-of-place entry) and a call under capture in a
            # training-step graph (ebm_langevin_chain_dev_f32 has none either): those kernels update a copy in place.
            if not heun and coords is None and n_steps > 0 and n > 0:
                src, state = state, torch.empty_like(state, memory_format=torch.contiguous_format)
            else:
                state = state.clone()
        traj, diag = new_outputs(self, x.shape, n_kept, want_traj, want_diag)
        _, rows = self._coef_rows(n_steps)
        if coords is not None:
            # utils.graphed_step is capturing this call: coordinates come from device memory (ebm_langevin_chain_dev_f32)
            if want_diag or heun or spec.kind != _lib.ENERGY_MLP or len(rows) != 1:
                raise RuntimeError(
                    "torchebm_amd: only the plain fused call on an MLPEnergy (constant step size / noise scale, no diagnostics) "
                    "can be captured in a training-step graph"
                )
            seed, step0 = 0, coords.take(n_steps)
        else:
            seed, step0 = _rng.reserve(generator, x.device, n_steps)
        stream = _lib.stream_handle(x.device)
        spec_c = spec.to_c()

        if n_steps > 0 and n > 0:
            layout = None
            if want_diag and n_kept > 0:
                layout = _lib.diag_layout(spec_c, _lib.DIAG_LANGEVIN_HEUN if heun else _lib.DIAG_LANGEVIN, n, dim, False, want_traj)
            if not want_diag or n_kept == 0:
                # one launch for the whole call; thinned rows are stored by the kernel
                self._launch_chain(spec_c, state, n, dim, rows, 0, n_steps, thin, traj, seed, step0, stream, src=src)
            elif layout is not None:
                self._fused_with_records(state, n_steps, thin, traj, diag, layout, stream,
                                         self._launcher(spec_c, state, rows, thin, seed, step0, stream, src))
            else:
                self._fused_with_state_passes(spec_c, state, n_steps, thin, traj, diag, stream,
                                              self._launcher(spec_c, state, rows, thin, seed, step0, stream, src))
        self.advance_schedulers(n_steps)
        out = traj if want_traj else state
        return (out, diag) if want_diag else out

    def _launcher(self, spec_c, state, rows, thin, seed, step0, stream, src):
        """``launch(t0, steps, traj_piece, records, first)`` of the drivers of a call with diagnostics: steps
        ``[t0, t0 + steps)`` of the call on ``state``, the first launch alone starting from ``src``."""
        n, dim = state.shape

        def launch(t0, steps, piece, records, first):
            self._launch_chain(spec_c, state, n, dim, rows, t0, steps, thin, piece, seed, step0 + t0, stream,
                               records=records, src=src if first else None)

        return launch

    def _fused_with_records(self, state, n_steps, thin, traj, diag, layout, stream, launch):
        """Diagnostics from inside the chain launch (``_chain_host.run_with_records``)."""
        # slots > dim: PACKED rows (a Gaussian whose width the matrix-layout kernel does not take as is: csrc/gauss_mfma.hip,
        # gauss_pack_factor) -- `pack` consecutive chains are one row of width pack * dim; the records and the merge are those of
        # n / pack rows, and the `pack` columns of every coordinate are pooled afterwards
        slots, dim = layout[1], state.shape[1]
        run_with_records(self, state, n_steps, thin, traj, diag, layout, stream, launch, pack=slots // dim if slots > dim else 1)

    def _fused_with_state_passes(self, spec_c, state, n_steps, thin, traj, diag, stream, launch):
        """Diagnostics for the configurations without in-kernel records (the matrix-layout kernels of the MLP
        energy, rows that neither divide nor are divided by the flat kernel's 1024-element blocks): the energy pass
        of ``_chain_host.run_with_state_passes``."""
        n, dim = state.shape
        energy = torch.empty(n, dtype=torch.float32, device=state.device)
        # a dense Gaussian above 128 dims: ebm_energy_grad_f32 is the lane-group mat-vec there (2 TFLOP/s: at 2^17 x 256 one
        # energy pass would cost more than the 20 chain steps before it)
        from ..core.energies import GaussianModel
        wide_gaussian = type(self.model) is GaussianModel and dim > GaussianModel.CLOSED_FORM_GRADIENT_ABOVE

        def mean_energy():
            if wide_gaussian:
                return self._model_energy(state, {}).mean()   # one library GEMM (GaussianModel.forward, wide CUDA batches)
            _lib.call("ebm_energy_grad_f32", spec_c, _lib.ptr(state), n, dim, _lib.ptr(energy), None, stream)
            return energy.mean()

        run_with_state_passes(state, n_steps, thin, traj, diag, stream, launch, mean_energy)
