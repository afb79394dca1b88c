r"""Windowed warm-up for :class:`GeneralizedHMC` and :class:`HamiltonianMonteCarlo` (``sampler.warmup``): the sequence Stan and
NumPyro run before sampling -- alternating step-size and mass windows, then a terminal step-size window -- composed of what the
package has: ``adapt_step_size`` (``samplers/adapt.py``) under the current mass, and a diagonal mass from the pooled variance of
the chains.

For each ``w`` in ``windows``:

1. ``adapt_step_size(x=<previous window's x>, n_steps=w, velocity=None, init_step_size=<previous window's pooled step size>,
   apply=False)`` under the current mass.  The first window starts from the sampler's own step size and its own mass (possibly
   ``None``).  ``velocity=None``: the mass changed, so every window draws fresh momenta.
2. ``var = x.reshape(-1, x.shape[-1]).var(0)`` over the window's final positions, ``N`` rows: an ENSEMBLE estimate across chains,
   the many-chain regime the kernels are built for (fewer than 2 rows raise).
3. With ``regularize``, Stan's shrinkage: ``var <- N/(N+5) var + 1e-3 * 5/(N+5)``.
4. The new mass ``1 / var``, fp32 ``[dim]``; a coordinate whose variance is not finite and positive keeps its previous mass
   (``torch.where``: no host read).

Then one terminal ``adapt_step_size`` window of ``final_steps`` under the final mass.

Every window costs ONE host read, the pooled step size: the next window's ``eps0`` and ``mu = log(mu_factor * eps0)`` are scalar
arguments of the entry.  Under the conditions of the fused routes of ``adapt_step_size`` every window is ONE launch --
``ebm_ghmc_adapt_chain_f32`` while the mass is ``None``, ``ebm_ghmc_adapt_chain_mass_f32`` from then on.  ``warmup()`` is new and
has no earlier bits to keep: it treats the massed fused route as eligible WITHOUT the opt-in ``fused_adapt_mass``.  Written out
with public calls on the GPU, the composition therefore sets ``sampler.fused_adapt_mass = True``; on the eager route nothing
differs.
"""

from __future__ import annotations

import copy
import math
from dataclasses import dataclass, field
from typing import List, Sequence

import torch

from ._chain_host import check_mass

SHRINK_COUNT, SHRINK_TARGET = 5.0, 1e-3  # Stan's regularisation of the variance estimate: towards 1e-3 with the weight of 5 rows


@dataclass
class Warmup:
    """What ``warmup`` returns.

    ``x``: the chains behind the terminal window (``[n, *shape]``).
    ``step_size``: 0-dim, the pooled step size of the terminal window.
    ``mass``: ``[dim]`` fp32, the mass of the terminal window.
    ``step_sizes``, ``acceptances``: per window (the terminal one last, ``len(windows) + 1`` entries), the pooled step size and
    the mean over chains of the acceptance while adapting, 0-dim tensors.
    ``masses``: per mass window (``len(windows)`` entries), the mass it formed."""

    x: torch.Tensor
    step_size: torch.Tensor
    mass: torch.Tensor
    step_sizes: List[torch.Tensor] = field(default_factory=list)
    acceptances: List[torch.Tensor] = field(default_factory=list)
    masses: List[torch.Tensor] = field(default_factory=list)


def mass_from_positions(x: torch.Tensor, previous: torch.Tensor, regularize: bool = True) -> torch.Tensor:
    """Steps 2 - 4 of the module docstring: the diagonal mass ``1 / var`` of the rows of ``x``, fp32 ``[dim]``; ``previous``
    (``[dim]``) where the variance is not finite and positive."""
    rows = x.reshape(-1, x.shape[-1])
    n = rows.shape[0]
    if n < 2:
        raise ValueError(f"warmup needs at least 2 rows for the pooled variance, got {n}")
    var = rows.var(0)
    if regularize:
        var = (n / (n + SHRINK_COUNT)) * var + SHRINK_TARGET * (SHRINK_COUNT / (n + SHRINK_COUNT))
    var = var.to(torch.float32)
    return torch.where(torch.isfinite(var) & (var > 0), 1.0 / var, previous.to(device=var.device, dtype=torch.float32))


def mass_vector(mass, dim: int, device) -> torch.Tensor:
    """A sampler's mass (``None``, a float, a ``[dim]`` tensor) as an fp32 ``[dim]`` tensor."""
    if mass is None:
        return torch.ones(dim, dtype=torch.float32, device=device)
    if isinstance(mass, float):
        return torch.full((dim,), mass, dtype=torch.float32, device=device)
    return mass.to(device=device, dtype=torch.float32).reshape(-1)


def warmup(sampler, x=None, dim=None, n_samples: int = 1, windows: Sequence[int] = (50, 50, 100), final_steps: int = 50,
           target_accept: float = 0.8, regularize: bool = True, generator=None, apply: bool = True,
           **dual_averaging_constants) -> Warmup:
    """What ``GeneralizedHMC.warmup`` and ``HamiltonianMonteCarlo.warmup`` run (their docstrings; the module docstring)."""
    unknown = set(dual_averaging_constants) - {"t0", "gamma", "kappa", "mu_factor", "bounds"}
    if unknown:
        raise TypeError(f"warmup() got unexpected keyword arguments {sorted(unknown)}")
    windows = [int(w) for w in windows]
    with torch.no_grad():
        x = sampler._init_state(x, dim, n_samples, generator)
    if x.ndim < 2 or x.numel() // max(x.shape[-1], 1) < 2:
        raise ValueError("warmup needs at least 2 rows for the pooled variance")
    # a shallow copy carries the windows' masses and the eligibility of the massed launch; the sampler itself is touched by
    # `apply` alone (the step size is passed per window, never set)
    work = copy.copy(sampler)
    work.fused_adapt_mass = True
    step_sizes, acceptances, masses = [], [], []
    eps = None  # the first window: the sampler's own step size
    current = mass_vector(sampler.mass, x.shape[-1], x.device)
    for i, n_steps in enumerate(windows + [int(final_steps)]):
        res = work.adapt_step_size(x=x, n_steps=n_steps, target_accept=target_accept, init_step_size=eps, velocity=None,
                                   generator=generator, apply=False, **dual_averaging_constants)
        x = res.x
        eps = float(res.step_size)  # the one host read of the window
        if not (eps > 0 and math.isfinite(eps)):
            raise RuntimeError(f"warmup: no chain of window {i} ended on a finite step size")
        step_sizes.append(res.step_size)
        acceptances.append(res.acceptance.mean())
        if i < len(windows):
            current = mass_from_positions(x, current, regularize)
            work.mass = check_mass(current, work.device)
            masses.append(current)
    if apply:
        sampler._register_param("step_size", eps, positive=True)
        sampler.mass = check_mass(current, sampler.device)
    return Warmup(x, step_sizes[-1], current, step_sizes, acceptances, masses)
