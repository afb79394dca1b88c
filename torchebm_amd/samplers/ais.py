r"""Annealed importance sampling (Neal 2001): ``log Z`` of an energy-based model, and with it the log-likelihood
``-E(x) - log Z`` of held-out data.

Every chain walks one state from the base ``p_0 = N(0, sigma_0^2 I)`` to the target ``exp(-E)`` through ``T`` tempered laws
``exp(-U_b)``, ``U_b = (1 - b) E_0 + b E``, ``E_0(x) = |x|^2 / (2 sigma_0^2)``, along a table ``0 = b_0 <= b_1 <= ... <= b_T = 1``.
Step ``t`` first adds ``(b_t - b_{t-1}) (E_0(x) - E(x))`` to the chain's log-weight and then moves the state with one
Metropolis-corrected HMC transition that leaves ``exp(-U_{b_t})`` invariant.  The weights are unbiased for ``Z / Z_0``:
``log Z ~= log Z_0 + logsumexp(logw) - log n``.  ``include/ebm_hip.h`` (``ebm_ais_chain_f32``) states the algorithm exactly.

Two execution routes, chosen once per ``run()`` call (``_route``):

``fused``  CUDA fp32, one of the analytic energies (not the MLP), ``dim <= 256``: the whole estimate -- the start draw, ``T``
           weight updates and transitions, Philox draws, per-temperature accept counters -- is ONE launch of
           ``ebm_ais_chain_f32`` (docs/design/ais.md).  The third member of the tempered family: the replica-exchange
           samplers run the temperatures side by side, this one runs them in time.
``fused_mlp``  opt-in (``sampler.fused_mlp = True``): CUDA fp32, an ``MLPEnergy`` of hidden width 64 / 128 and
           ``dim == in_dim <= 128``: the whole estimate is ONE launch of ``ebm_ais_mlp_chain_f32`` (docs/design/ais_mlp.md), the
           evaluation on the matrix cores inside the transition.  Its energies are the kernel's (fp32-accurate, not autograd's
           rounding), so the default stays ``eager`` for the MLP and an estimate made without the opt-in is bit for bit what it was.
``eager``  everything else (CPU, ``MLPEnergy`` or a hand-written energy, wider states, other dtypes): the same algorithm in
           torch ops, drawing ``randn(n, dim)`` for the start and then ``randn(n, dim)`` and ``rand(n)`` per step.

A fused-eligible call never falls back to eager: a missing library or a failing launch raises.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import torch

from .. import _lib, _rng
from ..core.energies import BaseModel, FusedSpec, fused_spec_for
from ..core.module import TorchEBMModule
from ._chain_host import fused_mlp_walk_fits


def ais_betas(n_temperatures: int, schedule: str = "linear", sharpness: float = 4.0) -> torch.Tensor:
    """The table ``beta[0 .. T]`` as fp32, formed in double and rounded once; ``beta[0] = 0`` and ``beta[T] = 1`` exactly.
    ``"linear"``: ``t / T``.  ``"sigmoid"``: ``s(t) = sigmoid(sharpness (2 t / T - 1))`` rescaled to ``[0, 1]`` -- short steps
    near both ends, where the path's laws change fastest."""
    T = int(n_temperatures)
    if T < 1:
        raise ValueError("n_temperatures must be >= 1")
    t = torch.arange(T + 1, dtype=torch.float64) / T
    if schedule == "linear":
        b = t
    elif schedule == "sigmoid":
        s = torch.sigmoid(float(sharpness) * (2.0 * t - 1.0))
        b = (s - s[0]) / (s[-1] - s[0])
    else:
        raise ValueError(f"schedule must be 'linear' or 'sigmoid', got {schedule!r}")
    b = b.to(torch.float32)
    b[0], b[-1] = 0.0, 1.0
    return b


def ais_estimate(log_weights: torch.Tensor, log_z0: float) -> Tuple[float, float, float, int]:
    """``(log_z, log_z_stderr, ess, n_nonfinite)`` of the log-weights of ``n`` chains, in double:

    ``log_z = log_z0 + logsumexp(logw) - log n``, ``ess = exp(2 lse(logw) - lse(2 logw))`` (Kish), ``log_z_stderr =
    sqrt(1 / ess - 1 / n)`` (the delta-method standard error of ``log mean w``).  A NaN log-weight counts as ``-inf`` (the
    chain contributes nothing); ``n_nonfinite`` counts the log-weights that are NaN or infinite."""
    lw = log_weights.detach().to(torch.float64).flatten()
    n = lw.numel()
    n_nonfinite = int((~torch.isfinite(lw)).sum())
    lw = torch.where(torch.isnan(lw), torch.full_like(lw, -math.inf), lw)
    lse1 = torch.logsumexp(lw, dim=0)
    lse2 = torch.logsumexp(2.0 * lw, dim=0)
    log_z = float(log_z0 + lse1 - math.log(n))
    ess = float(torch.exp(2.0 * lse1 - lse2))
    stderr = math.sqrt(max(1.0 / ess - 1.0 / n, 0.0)) if ess > 0.0 else math.inf
    return log_z, stderr, ess, n_nonfinite


@dataclass
class AISResult:
    """What :meth:`AnnealedImportanceSampling.run` returns."""

    log_weights: torch.Tensor      #: ``[n]``, the chains' log importance weights (against the normalised base)
    samples: torch.Tensor          #: ``[n, dim]``, the final states: approximately target samples that carry those weights
    log_z: float                   #: the estimate of ``log Z``
    log_z_stderr: float            #: its standard error
    ess: float                     #: effective sample size of the weights, ``1 .. n``
    acceptance_rate: torch.Tensor  #: ``[T]``, accepted / proposed transitions at each temperature: what ``step_size`` is tuned with
    n_nonfinite: int               #: log-weights that are NaN or infinite


class AnnealedImportanceSampling(TorchEBMModule):
    r"""Annealed importance sampling with Metropolis-corrected HMC transitions.

    Args:
        model: the energy model whose ``log Z = log \int exp(-E)`` is wanted.
        n_temperatures: ``T``, the number of steps (weight update + transition); ignored when ``betas`` is given.
        betas: the table ``beta[0 .. T]`` itself: ``beta[0] = 0``, ``beta[T] = 1``, non-decreasing.
        schedule: ``"linear"`` or ``"sigmoid"`` (:func:`ais_betas`).
        step_size: leapfrog step size: a float, or a sequence of ``T`` floats (one per transition; ``acceptance_rate`` of a
            run says where it is too long).
        n_leapfrog_steps: leapfrog steps per transition.
        base_std: ``sigma_0`` of the base ``N(0, sigma_0^2 I)``: it should cover the target's mass.
        dtype, device: where the chains live.

    Routes (``_route``): ``fused`` -- CUDA fp32, an analytic energy (not the MLP), ``dim <= 256``: ONE launch of
    ``ebm_ais_chain_f32`` per ``run()``, never a fallback; ``eager`` -- everything else, the same algorithm in torch ops,
    drawing ``randn(n, dim)`` for the start, then ``randn(n, dim)`` and ``rand(n)`` per step; ``fused_mlp`` -- the opt-in below.
    """

    #: opt-in: an ``MLPEnergy`` (hidden 64 / 128, ``dim == in_dim <= 128``, CUDA fp32, no autocast) runs as ONE launch of
    #: ``ebm_ais_mlp_chain_f32`` instead of the eager route.  Off by default: the fused evaluation is three-way-split bf16
    #: arithmetic at fp32 accuracy, not autograd's rounding, and the draws are the Philox field's, not torch's.
    fused_mlp = False

    def __init__(
        self,
        model: BaseModel,
        n_temperatures: int = 100,
        betas: Optional[Sequence[float]] = None,
        schedule: str = "linear",
        step_size: Union[float, Sequence[float]] = 0.1,
        n_leapfrog_steps: int = 5,
        base_std: float = 1.0,
        dtype: torch.dtype = torch.float32,
        device: Optional[Union[str, torch.device]] = None,
    ):
        super().__init__(device=device, dtype=dtype)
        self.model = model
        if betas is not None:
            b = torch.as_tensor([float(v) for v in betas], dtype=torch.float64)
            if b.numel() < 2 or b[0] != 0.0 or b[-1] != 1.0 or bool((b[1:] < b[:-1]).any()):
                raise ValueError("betas must start at 0, end at 1 and never decrease")
            self.betas = b.to(torch.float32)
        else:
            self.betas = ais_betas(n_temperatures, schedule)
        T = self.n_temperatures
        if isinstance(step_size, (float, int)):
            sizes = (float(step_size),) * T
        else:
            sizes = tuple(float(v) for v in step_size)
            if len(sizes) != T:
                raise ValueError(f"step_size must be a float or hold one value per transition ({T}), got {len(sizes)}")
        if any(not v > 0 for v in sizes):
            raise ValueError("step_size must be positive")
        self.step_sizes = torch.tensor(sizes, dtype=torch.float32)
        if int(n_leapfrog_steps) < 1:
            raise ValueError("n_leapfrog_steps must be >= 1")
        self.n_leapfrog_steps = int(n_leapfrog_steps)
        if not float(base_std) > 0:
            raise ValueError("base_std must be positive")
        self.base_std = float(base_std)
        self._tables: Optional[tuple] = None

    @property
    def n_temperatures(self) -> int:
        return self.betas.numel() - 1

    def base_coefficients(self) -> Tuple[float, float]:
        """``(sigma0, inv_var0)``: the fp32 values the algorithm uses, formed in double and rounded once."""
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32))  # noqa: E731
        return f32(self.base_std), f32(1.0 / self.base_std**2)

    def log_z0(self, dim: int) -> float:
        """``log Z_0 = dim / 2 * log(2 pi sigma_0^2)`` of the base's energy ``|x|^2 / (2 sigma_0^2)``."""
        return 0.5 * dim * math.log(2.0 * math.pi * self.base_std**2)

    # ---------------------------------------------------------------------------------
    # routing: decided here and nowhere else
    # ---------------------------------------------------------------------------------
    def _route(self, dim: int) -> Tuple[str, Optional[FusedSpec]]:
        if self.device.type != "cuda" or self.dtype != torch.float32 or dim > 256:
            return "eager", None
        if self.use_mixed_precision and self.autocast_available:
            return "eager", None
        spec = fused_spec_for(self.model, torch.empty(0, dim, dtype=self.dtype, device=self.device), None)
        if spec is None:
            return "eager", None
        if spec.kind == _lib.ENERGY_MLP:
            if self.fused_mlp and spec.hmc and fused_mlp_walk_fits(spec.n_comp, getattr(self.model, "in_dim", None), dim):
                return "fused_mlp", spec
            return "eager", None
        return "fused", spec

    # ---------------------------------------------------------------------------------
    # public API
    # ---------------------------------------------------------------------------------
    @torch.no_grad()
    def run(self, n_chains: int, dim: int, generator: Optional[torch.Generator] = None) -> AISResult:
        """One estimate from ``n_chains`` independent chains on ``dim`` coordinates."""
        n, dim = int(n_chains), int(dim)
        if n < 1 or dim < 1:
            raise ValueError("n_chains and dim must be >= 1")
        route, spec = self._route(dim)
        if route == "fused":
            logw, x, accepted = self._run_fused(spec, n, dim, generator)
        elif route == "fused_mlp":
            logw, x, accepted = self._run_fused(spec, n, dim, generator, entry="ebm_ais_mlp_chain_f32")
        else:
            logw, x, accepted = self._run_eager(n, dim, generator)
        log_z, stderr, ess, bad = ais_estimate(logw, self.log_z0(dim))
        return AISResult(log_weights=logw, samples=x, log_z=log_z, log_z_stderr=stderr, ess=ess,
                         acceptance_rate=(accepted / n).to(torch.float32), n_nonfinite=bad)

    @torch.no_grad()
    def log_likelihood(self, data: torch.Tensor, result: AISResult) -> torch.Tensor:
        """``log p(data) = -E(data) - log Z`` with the estimate of ``result``."""
        return -self.model(data) - result.log_z

    # ---------------------------------------------------------------------------------
    # route: torch ops
    # ---------------------------------------------------------------------------------
    def _run_eager(self, n: int, dim: int, generator):
        dev, dt = self.device, self.dtype
        sigma0, inv_var0 = self.base_coefficients()
        half_inv = 0.5 * inv_var0
        betas, T, L = self.betas, self.n_temperatures, self.n_leapfrog_steps
        x = sigma0 * torch.randn(n, dim, dtype=dt, device=dev, generator=generator)
        logw = torch.zeros(n, dtype=dt, device=dev)
        comp = torch.zeros(n, dtype=dt, device=dev)
        accepted = torch.zeros(T, dtype=torch.float64)
        base = lambda y: half_inv * torch.sum(y.square(), dim=-1)  # noqa: E731
        hamiltonian = lambda u, p: u.clamp(min=-1e10, max=1e10) + (0.5 * torch.sum(p.square(), dim=-1)).clamp_(min=0.0, max=1e10)  # noqa: E731
        with self.autocast_context():
            for t in range(1, T + 1):
                b = float(betas[t])
                db = float(betas[t] - betas[t - 1])   # the difference in fp32
                b0 = float(1.0 - betas[t])            # 1 - beta in fp32
                c0 = b0 * inv_var0
                e0, e = base(x), self.model(x)
                # the weight, a Kahan pair; an infinite sum stays what a plain sum gives
                y = db * (e0 - e) - comp
                s = logw + y
                comp = torch.where(torch.isfinite(s), (s - logw) - y, torch.zeros_like(s))
                logw = s
                force_at = lambda y: (-(c0 * y + b * self.model.gradient(y))).clamp_(min=-1e6, max=1e6)  # noqa: E731
                eps = float(self.step_sizes[t - 1])
                half = 0.5 * eps
                p = torch.randn(n, dim, dtype=dt, device=dev, generator=generator)
                u = torch.rand(n, dtype=dt, device=dev, generator=generator)
                h0 = hamiltonian(b0 * e0 + b * e, p)
                # the safe-mode leapfrog step of HamiltonianMonteCarlo, literally, on U_b
                xp = x
                for _ in range(L):
                    p_half = p + half * force_at(xp)
                    xp = xp + eps * p_half
                    p = p_half + half * force_at(xp)
                    xp = xp.nan_to_num_(nan=0.0)
                    p = p.nan_to_num_(nan=0.0)
                h1 = hamiltonian(b0 * base(xp) + b * self.model(xp), p)
                a = torch.exp((h0 - h1).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
                ok = u < a
                accepted[t - 1] = float(ok.sum())
                x = torch.where(ok[:, None], xp, x)
        return logw, x, accepted.to(dev)

    # ---------------------------------------------------------------------------------
    # routes: one launch of ebm_ais_chain_f32, or (fused_mlp) of ebm_ais_mlp_chain_f32 -- the same parameter list
    # ---------------------------------------------------------------------------------
    def _tables_on(self, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._tables is None or self._tables[0] != device:
            self._tables = (device, self.betas.to(device), self.step_sizes.to(device))
        return self._tables[1], self._tables[2]

    def _run_fused(self, spec: FusedSpec, n: int, dim: int, generator, entry: str = "ebm_ais_chain_f32"):
        dev, T = self.device, self.n_temperatures
        sigma0, inv_var0 = self.base_coefficients()
        betas, eps = self._tables_on(dev)
        x = torch.empty(n, dim, dtype=torch.float32, device=dev)  # written once by the kernel, never read
        logw = torch.empty(n, dtype=torch.float32, device=dev)
        counts = torch.zeros(T, dtype=torch.int32, device=dev)    # (uint32 counters in an int32 tensor)
        seed, step0 = _rng.reserve(generator, dev, 2 * T + 1)
        _lib.call(
            entry,
            spec.to_c(), _lib.ptr(x), _lib.ptr(logw), n, dim, T, self.n_leapfrog_steps, _lib.ptr(betas), _lib.ptr(eps),
            sigma0, inv_var0, None, _lib.ptr(counts), None, None, None, seed, step0, _lib.stream_handle(dev),
        )
        accepted = (counts.to(torch.int64) & 0xFFFFFFFF).to(torch.float64)
        return logw, x, accepted
