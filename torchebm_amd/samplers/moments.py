r"""Per-chain running moments: has a run converged, and how many effective samples did it produce?

``sample_moments`` on :class:`LangevinDynamics` and :class:`HamiltonianMonteCarlo` runs ``n_steps`` transitions, leaves the
first ``burn_in`` out and keeps, per chain and per coordinate, the time average and the sum of squared deviations over the two
halves of the remaining ``2 h`` states -- a Welford pair per half, fp32, beside the state -- and the same for the energy.
:class:`ChainMoments` turns them into split-:math:`\hat R`, a between-sequence effective sample size and pooled posterior
moments.  No trajectory is written: the statistics are taken where the state is (``include/ebm_hip.h``,
``ebm_chain_moments_f32``, states the algorithm exactly; docs/design/moments.md).

Three execution routes, chosen once per call (:func:`fused_moments_eligible`):

``fused``  CUDA fp32, an analytic energy with a fused spec (not the MLP), a 2-D state with ``dim <= 256``, constant schedulers,
           no clamp, no ``model_kwargs``, and for HMC ``mass is None`` with the plain leapfrog integrator: ONE launch of
           ``ebm_chain_moments_f32``; ``_rng.reserve`` of ``k`` Philox steps for Langevin and ``2 k`` for HMC -- the
           coordinates ``sample()`` draws at, so for the element-wise energies under Langevin the final states are
           ``sample()``'s bit for bit.
``fused_mlp``  Langevin on an ``MLPEnergy`` under the sampler's opt-in ``fused_mlp_moments = True``
           (:func:`fused_mlp_moments_eligible`: what ``sample()`` runs fused, hidden width 64 / 128, ``dim == in_dim <= 128``,
           constant schedulers, no clamp, plain Euler-Maruyama, no autocast): ONE launch of ``ebm_chain_moments_mlp_f32``
           (docs/design/langevin_moments_mlp.md) with the reservation of ``sample(n_steps=k)``; the energies are the kernel's,
           not autograd's, and ``x_final`` is ``sample()``'s draw for draw, not guaranteed bit for bit.  Without the opt-in the
           call stays on ``eager`` and returns what it always did.
``eager``  anything else, CPU included: the sampler's own route, one ``sample(n_steps=1)`` per transition, around the same
           Welford recurrence with the same reciprocal table (:class:`RunningMoments`).

A fused-eligible call never falls back to eager: a missing library or a failing launch raises.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from .. import _lib, _rng
from ..core.energies import fused_spec_for
from ._chain_host import fused_mlp_walk_fits

SAMPLER_LANGEVIN, SAMPLER_HMC = 0, 1
FUSED_MAX_DIM = 256


def recip_table(half_len: int) -> torch.Tensor:
    """``float32(1 / c)`` for ``c = 1 .. half_len``, formed in double and rounded once (CPU tensor)."""
    return (1.0 / torch.arange(1, int(half_len) + 1, dtype=torch.float64)).to(torch.float32)


def split_counted(n_steps: int, burn_in: int) -> Tuple[int, int]:
    """``(burn_in, half_len)`` of a call: when ``n_steps - burn_in`` is odd one more step is burnt; ``half_len >= 2``."""
    n_steps, burn_in = int(n_steps), int(burn_in)
    if burn_in < 0 or burn_in > n_steps:
        raise ValueError(f"burn_in must lie in 0 .. n_steps, got {burn_in} of {n_steps}")
    if (n_steps - burn_in) % 2:
        burn_in += 1
    h = (n_steps - burn_in) // 2
    if h < 2:
        raise ValueError(f"at least 4 counted steps are needed (two halves of 2), got {n_steps - burn_in}")
    return burn_in, h


class RunningMoments:
    """The Welford recurrence of ``ebm_chain_moments_f32`` in torch ops, one :meth:`add` per counted state:

    ``d = x - mean;  mean = mean + d * recip[c - 1];  M2 = M2 + d * (x - mean)``, every operation rounded on its own, in the
    dtype of the state; the first ``half_len`` states go to half 0, the next ``half_len`` to half 1."""

    def __init__(self, half_len: int, with_energy: bool = False):
        self.half_len = int(half_len)
        self.recip = recip_table(self.half_len)
        self.with_energy = bool(with_energy)
        self.count = 0
        self.mean = self.m2 = self.e_mean = self.e_m2 = None

    @staticmethod
    def _step(mean, m2, half, x, rc):
        d = x - mean[half]
        mean[half] = mean[half] + d * rc
        m2[half] = m2[half] + d * (x - mean[half])

    @torch.no_grad()
    def add(self, x: torch.Tensor, energy: Optional[torch.Tensor] = None) -> None:
        if self.count >= 2 * self.half_len:
            raise ValueError("both halves are full")
        if self.mean is None:
            self.mean = torch.zeros((2, *x.shape), dtype=x.dtype, device=x.device)
            self.m2 = torch.zeros_like(self.mean)
            if self.with_energy:
                self.e_mean = torch.zeros((2, x.shape[0]), dtype=x.dtype, device=x.device)
                self.e_m2 = torch.zeros_like(self.e_mean)
        half, c = divmod(self.count, self.half_len)
        rc = self.recip[c].to(dtype=x.dtype).item()
        self._step(self.mean, self.m2, half, x, rc)
        if self.with_energy:
            if energy is None:
                raise ValueError("this accumulator was built with_energy: pass the energies of the state")
            self._step(self.e_mean, self.e_m2, half, energy.to(x.dtype), rc)
        self.count += 1

    def result(self, acceptance_rate: Optional[torch.Tensor] = None) -> "ChainMoments":
        if self.count != 2 * self.half_len:
            raise ValueError(f"{self.count} states were added, {2 * self.half_len} are needed")
        return ChainMoments(self.mean, self.m2, self.half_len, self.e_mean, self.e_m2, acceptance_rate)


class ChainMoments:
    r"""Per-chain time moments of a run and the convergence figures that follow from them.

    Holds ``chain_mean`` and ``chain_m2`` of shape ``[2, n, dim]`` (half, chain, coordinate; ``m2`` is the sum of squared
    deviations from the half's mean), when the energy was requested ``energy_mean`` and ``energy_m2`` of shape ``[2, n]``,
    ``half_len``, for HMC and generalized HMC ``acceptance_rate`` (``[n_steps]``, accepted / proposed per transition) and, for
    ``UnderdampedLangevin``, ``velocity_sq_mean`` of shape ``[2, n, dim]``: the time average of ``v^2`` over either half.

    Everything below is computed once, in float64, from ``M = 2 n`` sequences of length ``l = half_len`` (the half-chains).
    Chains with any non-finite moment are left out and counted in ``n_nonfinite``.

    * ``within_var``  :math:`W`, the mean over sequences of ``M2 / (l - 1)``.
    * ``between_var``  :math:`B / l`, the unbiased variance over sequences of the sequence means.
    * ``var_plus = (l - 1) / l * W + B / l``.
    * ``rhat = sqrt(var_plus / W)`` per coordinate (``energy_rhat`` for the energy): split-:math:`\hat R` without rank
      normalisation.
    * ``ess = min(M l, M var_plus / (B / l))`` (``energy_ess``): the between-sequence (batch-means) estimator with the
      half-chains as batches.  Its relative standard error is about ``sqrt(2 / (M - 1))`` (``ess_rel_stderr``): it is meant
      for the many-chain regime this package runs in, and for ``l`` well above the autocorrelation time -- shorter halves
      are still correlated with each other's neighbours inside a chain and the figure is then optimistic.
    * ``mean``, ``var``: the pooled posterior mean and (unbiased) variance per coordinate over all counted states.
    * ``kinetic_temperature``: the mean of ``velocity_sq_mean`` over halves and chains, per coordinate; ``None`` without it.
    """

    def __init__(self, chain_mean, chain_m2, half_len, energy_mean=None, energy_m2=None, acceptance_rate=None,
                 velocity_sq_mean=None):
        self.chain_mean, self.chain_m2 = chain_mean, chain_m2
        self.energy_mean, self.energy_m2 = energy_mean, energy_m2
        self.half_len = int(half_len)
        self.acceptance_rate = acceptance_rate
        self.velocity_sq_mean = velocity_sq_mean
        self._stats = None

    @staticmethod
    def _figures(mean: torch.Tensor, m2: torch.Tensor, ell: int):
        """``mean``, ``m2``: ``[M, ...]`` float64 sequences."""
        M = mean.shape[0]
        nan = torch.full(mean.shape[1:], math.nan, dtype=torch.float64, device=mean.device)
        if M < 2:
            return dict(within_var=nan, between_var=nan, var_plus=nan, rhat=nan, ess=nan, mean=nan, var=nan)
        W = (m2 / (ell - 1)).mean(dim=0)
        grand = mean.mean(dim=0)
        dev2 = ((mean - grand) ** 2).sum(dim=0)
        B_over_l = dev2 / (M - 1)
        var_plus = (ell - 1) / ell * W + B_over_l
        rhat = torch.sqrt(var_plus / W)
        ess = torch.clamp(M * var_plus / B_over_l, max=float(M * ell))
        var = (m2.sum(dim=0) + ell * dev2) / (M * ell - 1)
        return dict(within_var=W, between_var=B_over_l, var_plus=var_plus, rhat=rhat, ess=ess, mean=grand, var=var)

    def _compute(self):
        if self._stats is not None:
            return self._stats
        n = self.chain_mean.shape[1]
        mean = self.chain_mean.detach().to(torch.float64).reshape(2, n, -1)
        m2 = self.chain_m2.detach().to(torch.float64).reshape(2, n, -1)
        good = torch.isfinite(mean).all(dim=2).all(dim=0) & torch.isfinite(m2).all(dim=2).all(dim=0)
        have_e = self.energy_mean is not None
        if have_e:
            e_mean, e_m2 = self.energy_mean.detach().to(torch.float64), self.energy_m2.detach().to(torch.float64)
            good &= torch.isfinite(e_mean).all(dim=0) & torch.isfinite(e_m2).all(dim=0)
        have_v2 = self.velocity_sq_mean is not None
        if have_v2:
            v2 = self.velocity_sq_mean.detach().to(torch.float64).reshape(2, n, -1)
            good &= torch.isfinite(v2).all(dim=2).all(dim=0)
        shape = tuple(self.chain_mean.shape[2:])
        seq = lambda t: t[:, good].reshape(-1, *t.shape[2:])  # noqa: E731  ([2, n', ...] -> [2 n', ...])
        st = {k: v.reshape(shape) for k, v in self._figures(seq(mean), seq(m2), self.half_len).items()}
        if have_e:
            st.update({"energy_" + k: v for k, v in self._figures(seq(e_mean), seq(e_m2), self.half_len).items()})
        if have_v2:
            # both halves hold half_len steps: the mean over halves and chains is the mean over all counted velocities
            st["kinetic_temperature"] = v2[:, good].mean(dim=(0, 1)).reshape(shape)
        st["n_nonfinite"] = int(n - int(good.sum()))
        st["n_sequences"] = 2 * int(good.sum())
        self._stats = st
        return st

    @property
    def kinetic_temperature(self) -> Optional[torch.Tensor]:
        """The time- and chain-averaged ``v^2`` per coordinate (float64, over the chains with finite moments), or ``None``
        when the run kept no ``velocity_sq_mean``.  Under BAOAB on a quadratic energy it estimates ``T (1 - h^2 E'' / 4)``."""
        return self._compute().get("kinetic_temperature")

    def diagonal_mass(self) -> torch.Tensor:
        """``1 / var`` as a float32 ``[dim]`` tensor on the moments' device: the textbook diagonal mass for the ``mass=`` of
        ``HamiltonianMonteCarlo``, ``UnderdampedLangevin`` and ``GeneralizedHMC`` (a coordinate of standard deviation ``s`` then
        moves as one of unit scale).  Raises ``ValueError`` when a pooled variance is not finite and positive."""
        var = self._compute()["var"].reshape(-1)
        if not bool((torch.isfinite(var) & (var > 0)).all()):
            raise ValueError("diagonal_mass: a pooled variance is not finite and positive (run longer, or drop the chains that left)")
        return (1.0 / var).to(torch.float32)

    def __getattr__(self, name):
        if name.startswith("_") or name in ("chain_mean", "chain_m2", "energy_mean", "energy_m2", "half_len", "acceptance_rate",
                                            "velocity_sq_mean"):
            raise AttributeError(name)
        st = self._compute()
        if name in st:
            return st[name]
        raise AttributeError(name)

    @property
    def ess_rel_stderr(self) -> float:
        M = self._compute()["n_sequences"]
        return math.sqrt(2.0 / (M - 1)) if M > 1 else math.inf

    def __repr__(self) -> str:
        st = self._compute()
        return (f"ChainMoments(n={self.chain_mean.shape[1]}, half_len={self.half_len}, max rhat={float(st['rhat'].max()):.4f}, "
                f"min ess={float(st['ess'].min()):.1f}, n_nonfinite={st['n_nonfinite']})")


# ---------------------------------------------------------------------------------
# routing: decided here and nowhere else
# ---------------------------------------------------------------------------------
def fused_moments_eligible(*, is_cuda: bool, dtype: torch.dtype, ndim: int, dim: int, spec_kind: Optional[int], constant: bool,
                           has_model_kwargs: bool, plain_integrator: bool, autocast: bool, extras_ok: bool) -> bool:
    """The routing predicate of ``sample_moments``.  ``spec_kind``: the kind of the model's fused spec, or ``None`` when it
    has none; ``extras_ok``: Langevin -- no clamp; HMC -- ``mass is None``, not ``exact``, the spec has an HMC kernel."""
    return bool(is_cuda and dtype == torch.float32 and ndim == 2 and 1 <= dim <= FUSED_MAX_DIM and spec_kind is not None
                and spec_kind != _lib.ENERGY_MLP and constant and not has_model_kwargs and plain_integrator and not autocast
                and extras_ok)


def fused_mlp_moments_eligible(*, opted_in: bool, dtype: torch.dtype, ndim: int, n: int, dim: int, route: Optional[str],
                               spec_kind: Optional[int], hidden: Optional[int], in_dim: Optional[int], constant: bool,
                               plain_integrator: bool, autocast: bool, has_clamp: bool) -> bool:
    """The routing predicate of ``LangevinDynamics.sample_moments`` to ``ebm_chain_moments_mlp_f32``.  ``opted_in``: the sampler's
    ``fused_mlp_moments``; ``route``, ``spec_kind``, ``hidden``: what ``sampler._route(x, {})`` returned -- the route's name
    (``"fused"`` only for a CUDA fp32 state: the sampler decides that, here as for ``sample()``), the spec's kind and its
    ``n_comp`` (``None`` without a spec); ``in_dim``: the model's."""
    return bool(opted_in and dtype == torch.float32 and ndim == 2 and n > 0 and route == "fused"
                and spec_kind == _lib.ENERGY_MLP and dim >= 1 and fused_mlp_walk_fits(hidden, in_dim, dim) and constant
                and plain_integrator and not autocast and not has_clamp)


def _route_mlp(sampler, x: torch.Tensor):
    """The fused spec of an eligible ``LangevinDynamics`` call on an ``MLPEnergy`` under ``fused_mlp_moments``, or ``None``."""
    from ..integrators.em import EulerMaruyamaIntegrator

    if not getattr(sampler, "fused_mlp_moments", False) or x.ndim != 2:
        return None
    route, spec = sampler._route(x, {})
    ok = fused_mlp_moments_eligible(
        opted_in=True, dtype=x.dtype, ndim=x.ndim, n=x.shape[0], dim=x.shape[1], route=route,
        spec_kind=None if spec is None else spec.kind, hidden=None if spec is None else spec.n_comp,
        in_dim=getattr(sampler.model, "in_dim", None), constant=all(s.is_constant() for s in sampler.schedulers.values()),
        plain_integrator=type(sampler.integrator) is EulerMaruyamaIntegrator,
        autocast=bool(sampler.use_mixed_precision and sampler.autocast_available), has_clamp=sampler.clamp is not None)
    return spec if ok else None


def _route(sampler, hmc: bool, x: torch.Tensor):
    from ..integrators.em import EulerMaruyamaIntegrator
    from ..integrators.symplectic import LeapfrogIntegrator

    if not x.is_cuda or x.dtype != torch.float32 or x.ndim != 2 or x.shape[1] > FUSED_MAX_DIM or x.shape[1] < 1:
        return None
    spec = fused_spec_for(sampler.model, x, {})
    constant = all(s.is_constant() for s in sampler.schedulers.values())
    if hmc:
        plain = type(sampler.integrator) is LeapfrogIntegrator
        extras = sampler.mass is None and not sampler.exact and (spec is None or bool(spec.hmc))
    else:
        plain = type(sampler.integrator) is EulerMaruyamaIntegrator
        extras = sampler.clamp is None
    ok = fused_moments_eligible(
        is_cuda=x.is_cuda, dtype=x.dtype, ndim=x.ndim, dim=x.shape[1], spec_kind=None if spec is None else spec.kind,
        constant=constant, has_model_kwargs=False, plain_integrator=plain,
        autocast=bool(sampler.use_mixed_precision and sampler.autocast_available), extras_ok=extras)
    return spec if ok else None


@torch.no_grad()
def sample_moments(sampler, hmc: bool, x, dim, n_steps, n_samples, burn_in, energy, generator):
    """What ``LangevinDynamics.sample_moments`` and ``HamiltonianMonteCarlo.sample_moments`` run."""
    burn_in, h = split_counted(n_steps, burn_in)
    sampler.reset_schedulers()
    if hmc and x is None and dim is None:
        mean = getattr(sampler.model, "mean", None)
        if not isinstance(mean, torch.Tensor):
            raise ValueError("dim must be provided when x is None and cannot be inferred from model")
        dim = mean.shape[0]
    x = sampler._init_state(x, dim, n_samples, generator)
    spec = _route(sampler, hmc, x) if x.shape[0] > 0 else None
    if spec is not None:
        return _fused(sampler, hmc, spec, x, int(n_steps), burn_in, h, bool(energy), generator)
    spec = None if hmc else _route_mlp(sampler, x)
    if spec is not None:
        return _fused(sampler, False, spec, x, int(n_steps), burn_in, h, bool(energy), generator, entry="ebm_chain_moments_mlp_f32")
    return _eager(sampler, hmc, x, int(n_steps), burn_in, h, bool(energy), generator)


def _eager(sampler, hmc, x, k, burn_in, h, energy, generator):
    acc = RunningMoments(h, with_energy=energy)
    rates = []
    for s in range(k):
        out = sampler.sample(x=x, n_steps=1, return_diagnostics=hmc, reset_schedulers=False, generator=generator)
        if hmc:
            x, diag = out
            rates.append(diag["acceptance_rate"][0])
        else:
            x = out
        if s >= burn_in:
            acc.add(x, sampler._model_energy(x, {}) if energy else None)
    rate = torch.stack(rates).to(torch.float32) if hmc else None
    return x, acc.result(rate)


def _fused(sampler, hmc, spec, x, k, burn_in, h, energy, generator, entry: str = "ebm_chain_moments_f32"):
    from .langevin import em_coefficients

    n, dim = x.shape
    dev = x.device
    state = _lib.dense_f32(x)
    if state.data_ptr() == x.data_ptr():
        state = state.clone()  # the kernel updates in place; the caller's tensor is never touched
    recip = recip_table(h).to(dev)
    mom = torch.empty(4, n, dim, dtype=torch.float32, device=dev)
    e_mom = torch.empty(4, n, dtype=torch.float32, device=dev) if energy else None
    stream = _lib.stream_handle(dev)
    if hmc:
        counts = torch.zeros(k, dtype=torch.int32, device=dev)  # (uint32 counters in an int32 tensor)
        seed, step0 = _rng.reserve(generator, dev, 2 * k)
        eps = float(sampler.schedulers["step_size"].get_value())
        _lib.call("ebm_chain_moments_f32", spec.to_c(), _lib.ptr(state), n, dim, SAMPLER_HMC, k, burn_in, 0.0, 0.0, 0.0,
                  int(sampler.n_leapfrog_steps), eps, _lib.ptr(recip), _lib.ptr(mom), _lib.ptr(e_mom), None, None, None,
                  _lib.ptr(counts), None, None, seed, step0, stream)
        rate = ((counts.to(torch.int64) & 0xFFFFFFFF).to(torch.float64) / n).to(torch.float32)
    else:
        seed, step0 = _rng.reserve(generator, dev, k)
        a, sq, coef = em_coefficients(sampler.schedulers["step_size"].get_value(), sampler.schedulers["noise_scale"].get_value())
        _lib.call(entry, spec.to_c(), _lib.ptr(state), n, dim, SAMPLER_LANGEVIN, k, burn_in, a, sq, coef,
                  0, 0.0, _lib.ptr(recip), _lib.ptr(mom), _lib.ptr(e_mom), None, None, None, None, None, None, seed, step0,
                  stream)
        rate = None
    sampler.advance_schedulers(k)
    res = ChainMoments(torch.stack((mom[0], mom[2])), torch.stack((mom[1], mom[3])), h,
                       torch.stack((e_mom[0], e_mom[2])) if energy else None,
                       torch.stack((e_mom[1], e_mom[3])) if energy else None, rate)
    return state, res
