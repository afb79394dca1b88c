"""Host machinery the chain samplers share: the outputs and kept-state statistics of a call, the step route's HIP-graph
replay, the device table of a scheduled step size, and the two drivers of a fused call with diagnostics (in-kernel
records + merge, or one launch per kept step + passes over the state).  The plain fused call needs none of it.  And the one
rule every sampler's routing asks: which ``MLPEnergy`` shapes the fused walks on the wide MLP energy take."""

from __future__ import annotations

import threading
from typing import Dict, Optional

import torch

from .. import _lib, _rng
from ..core.module import ForwardProbe, graph_blind_spots, warn_once

_RECORD_SCRATCH_KEEP_BYTES = 16 << 20
_CAPTURE_LOCK = threading.Lock()  # serialises graph capture: it toggles the process-wide cyclic GC

#: the shapes of the fused walks on the wide MLP energy (``wide_mlp_check_shape`` / ``wide_mlp_check_ladder_shape`` of
#: csrc/chain_launch.h refuse the rest): the hidden widths, the widest row -- four state tiles of 32 columns -- and the ladder
#: lengths of the two tempered walks, whole ladders per 32-row wave
FUSED_MLP_HIDDEN = (64, 128)
FUSED_MLP_MAX_DIM = 128
FUSED_MLP_LADDERS = (2, 4, 8, 16, 32)


def fused_mlp_walk_fits(hidden: Optional[int], in_dim: Optional[int], dim: int, n_replicas: Optional[int] = None) -> bool:
    """Whether a state of ``dim`` columns on an ``MLPEnergy`` of ``hidden`` (its spec's ``n_comp``) and ``in_dim`` -- and, for a
    tempered walk, a ladder of ``n_replicas`` slots -- fits the fused MLP walks.  Opt-in flags, dtype and device are the caller's."""
    return bool(hidden in FUSED_MLP_HIDDEN and dim == in_dim and dim <= FUSED_MLP_MAX_DIM
                and (n_replicas is None or n_replicas in FUSED_MLP_LADDERS))


# -------------------------------------------------------------------------------------
# the scalar or diagonal mass of the two velocity-carrying samplers (UnderdampedLangevin, GeneralizedHMC)
# -------------------------------------------------------------------------------------
def check_mass(mass, device):
    """The ``mass=`` argument as the sampler keeps it: ``None``, a positive finite float, or a 1-D tensor on ``device``
    (its entries are not inspected: no host sync)."""
    import math

    if mass is None:
        return None
    if torch.is_tensor(mass):
        if mass.ndim != 1:
            raise ValueError(f"mass must be a float or a 1-D tensor, got a tensor of shape {tuple(mass.shape)}")
        return mass.to(device)
    if isinstance(mass, bool) or not isinstance(mass, (int, float)):
        raise ValueError(f"mass must be None, a float or a 1-D tensor, got {type(mass).__name__}")
    if not (mass > 0 and math.isfinite(mass)):
        raise ValueError(f"mass must be positive and finite, got {mass}")
    return float(mass)


def mass_row(mass, x: torch.Tensor):
    """``mass`` as ``p * p / m`` takes it on a state shaped as ``x``: ``None``, the float, or the tensor broadcast along the last
    width.  Raises ``ValueError`` for a tensor whose length is not that width."""
    if mass is None or isinstance(mass, float):
        return mass
    if mass.numel() != x.shape[-1]:
        raise ValueError(f"mass tensor must have {x.shape[-1]} entries, got {mass.numel()}")
    return mass.to(device=x.device, dtype=x.dtype).view((1,) * (x.ndim - 1) + (-1,))


def mass_forms(mass, x: torch.Tensor):
    """``(m_sqrt, m_safe)`` of the contract (include/ebm_hip.h, ebm_kinetic_chain_mass_f32) as tensors of ``x``'s dtype that
    broadcast against ``x``: ``sqrt(m)`` formed in double and rounded once (correctly rounded, as the kernel's), and
    ``max(m, 1e-10)``."""
    if isinstance(mass, float):  # both formed in double, rounded once
        both = torch.tensor([mass, max(mass, 1e-10)], dtype=torch.float64, device=x.device)
        return both[0].sqrt().to(x.dtype), both[1].to(x.dtype)
    m = mass_row(mass, x)
    return m.to(torch.float64).sqrt().to(x.dtype), torch.where(m < 1e-10, torch.full_like(m, 1e-10), m)


def kinetic_temperature(v: torch.Tensor, m=None) -> torch.Tensor:
    """The mean of ``v^2`` -- with a mass ``m`` (``mass_row``) of ``p^2 / m`` -- over chains and coordinates; NaN for no chain."""
    if not v.numel():
        return torch.full((), float("nan"), dtype=v.dtype, device=v.device)
    return v.square().mean() if m is None else (v.square() / m).mean()


# -------------------------------------------------------------------------------------
# kept states: outputs and their statistics
# -------------------------------------------------------------------------------------
def new_outputs(like, shape, n_kept: int, want_traj: bool, want_diag: bool, acceptance: bool = False):
    """``(traj, diag)`` of a call on a state of ``shape`` ``[n, *rest]``, with the dtype and device of ``like`` (a sampler
    or a tensor): ``[n, n_kept, *rest]`` and the ``"mean"`` / ``"var"`` (``[n_kept, *rest]``) / ``"energy"``
    (``[n_kept]``) [/ ``"acceptance_rate"``] dict -- ``None`` where not wanted, and nothing else is done for a plain call."""
    traj = torch.empty((shape[0], n_kept, *shape[1:]), dtype=like.dtype, device=like.device) if want_traj else None
    if not want_diag:
        return traj, None
    kw = dict(dtype=like.dtype, device=like.device)
    diag = {"mean": torch.empty(n_kept, *shape[1:], **kw), "var": torch.empty(n_kept, *shape[1:], **kw),
            "energy": torch.empty(n_kept, **kw)}
    if acceptance:
        diag["acceptance_rate"] = torch.empty(n_kept, **kw)
    return traj, diag


def record_kept(state: torch.Tensor, keep: int, traj, diag, energy, accepted=None) -> None:
    """Record ``state`` ``[n, ...]`` as kept state ``keep`` with torch ops: its trajectory row, the mean and the biased
    variance (clamped to [1e-10, 1e10]; 0 for a single chain) over the chains, the mean of ``energy(state)`` and, with
    the ``accepted`` mask of the transition, the acceptance rate."""
    if traj is not None:
        traj[:, keep] = state
    if diag is not None:
        n = state.shape[0]
        if n > 1:
            diag["mean"][keep] = state.mean(dim=0)
            diag["var"][keep] = state.var(dim=0, unbiased=False).clamp_(min=1e-10, max=1e10)
        else:
            diag["mean"][keep] = state.squeeze(0) if n else state.mean(dim=0)
            diag["var"][keep].zero_()
        diag["energy"][keep] = energy(state).mean()
        if accepted is not None:
            diag["acceptance_rate"][keep] = accepted.float().mean()


def kept_statistics(spec_c, traj: torch.Tensor, diag: Dict[str, torch.Tensor], stream) -> None:
    """mean / var / energy of the kept states ``traj`` ``[n, n_kept, dim]`` of a one-launch call, with the
    column-statistics and energy kernels."""
    n, n_kept, dim = traj.shape
    kept = traj.transpose(0, 1).contiguous()  # [n_kept, n, dim]: one dense population per kept step
    energy = torch.empty(n_kept, n, dtype=torch.float32, device=traj.device)
    _lib.call("ebm_energy_grad_f32", spec_c, _lib.ptr(kept), n_kept * n, dim, _lib.ptr(energy), None, stream)
    diag["energy"].copy_(energy.mean(dim=1))
    if n == 1:
        diag["mean"].copy_(kept[:, 0])
        diag["var"].zero_()
        return
    work = torch.zeros(2 * dim + 1, dtype=torch.float64, device=traj.device)  # the kernel leaves it zeroed
    for keep in range(n_kept):
        _lib.call(
            "ebm_chain_stats_f32",
            _lib.ptr(_lib.dense_f32(kept[keep])), n, dim, _lib.ptr(diag["mean"][keep]), _lib.ptr(diag["var"][keep]), _lib.ptr(work), stream,
        )


# -------------------------------------------------------------------------------------
# the step route replayed from a HIP graph
# -------------------------------------------------------------------------------------
def use_graph(sampler, model_kwargs, n_steps: int) -> bool:
    """Bound as ``_use_graph`` by the samplers with a step route (``_graph_eligible``, ``capture_graph``, ``GRAPH_MIN_STEPS``)."""
    if sampler.capture_graph is False or not sampler._graph_eligible(model_kwargs):
        return False
    return sampler.capture_graph is True or n_steps >= sampler.GRAPH_MIN_STEPS


def _replay_or_step(sampler, g, first: bool, more: bool) -> None:
    """One iteration of the graph route: a replay once the graph exists; until then the step body runs eagerly (a real
    step), and behind the FIRST one of a call the graph is captured -- unless, by default, that step showed side effects
    (``ForwardProbe``) or the model has attributes the cache key cannot see into (``sampler.capture_graph``,
    ``sampler._graph_refused``)."""
    if g["graph"] is not None:
        g["graph"].replay()
        return
    refused = getattr(sampler, "_graph_refused", None)
    if refused is None:
        refused = sampler._graph_refused = {}
    prior = refused.get(g["key"])  # ("probe" | "failed", reasons): a default-mode refusal does not bind capture_graph = True
    decide = first and more and (prior is None or (sampler.capture_graph is True and prior[0] == "probe"))
    probe = ForwardProbe(sampler.model, g["state"].device) if decide and sampler.capture_graph is not True else None
    g["body"]()
    if not decide:
        return
    why = []
    if probe is not None:
        why = probe.side_effects()
        blind = graph_blind_spots(sampler.model)
        if blind:
            why.append("attributes the cache key cannot see into: " + ", ".join(blind[:4]))
    if not why:
        # The cyclic collector must not run inside the capture: finalising a dead sampler's CUDAGraph (or any tensor whose
        # storage goes back to the driver) while this stream records aborts the process.  torch.cuda.graph() collects
        # once on entry; what becomes garbage during the body waits until the capture has ended.
        # The GC switch is process-wide: the lock keeps a second sampler capturing on another thread from re-enabling it in
        # the middle of this capture (and the prior state is read inside the lock).
        import gc

        with _CAPTURE_LOCK:
            gc_was_on = gc.isenabled()
            try:
                graph = torch.cuda.CUDAGraph()
                gc.disable()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    g["body"]()
                g["graph"] = graph
                return
            except RuntimeError as exc:  # the forward cannot be captured (host sync, data-dependent control flow ...)
                if "ebm_" in str(exc):
                    raise
                warn_once("capture-graph-failed", f"torchebm_amd: HIP-graph capture of the step route failed ({exc}); "
                          "continuing with eager launches.", UserWarning)
                probe, why = None, [f"capture failed: {exc}"]
            finally:
                if gc_was_on:
                    gc.enable()
    refused.pop(g["key"], None)
    if len(refused) >= 8:
        refused.pop(next(iter(refused)))
    refused[g["key"]] = ("failed" if probe is None else "probe", why)


def sample_graph(sampler, x, n_steps: int, thin: int, traj, diag, generator, stride: int, energy):
    """The step route of a call as replays of ``sampler._graph_for(x)`` (``{"key", "graph", "state", "rng", "body"}`` and,
    where a step is a Metropolis transition, ``"mask"``); a step consumes ``stride`` Philox steps.  Kept states are
    recorded with torch ops (``record_kept`` with ``energy``)."""
    x = _lib.dense_f32(x)
    g = sampler._graph_for(x)
    seed, step0 = _rng.reserve(generator, x.device, stride * n_steps)
    as_i64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v  # noqa: E731  (bit pattern of a uint64)
    g["state"].copy_(x)
    g["rng"].copy_(torch.tensor([as_i64(seed), as_i64(step0)], dtype=torch.int64), non_blocking=True)
    state, mask, keep = g["state"], g.get("mask"), 0
    for i in range(n_steps):
        _replay_or_step(sampler, g, first=(i == 0), more=(i + 1 < n_steps))
        if (i + 1) % thin == 0:
            record_kept(state, keep, traj, diag, energy, mask)
            keep += 1
    sampler.advance_schedulers(n_steps)
    out = state.clone() if traj is None else traj
    return out if diag is None else (out, diag)


# -------------------------------------------------------------------------------------
# fused route: the schedule table
# -------------------------------------------------------------------------------------
def schedule_table(sampler, rows, device):
    """Device table of a non-constant schedule (``None`` for a constant one), kept on the sampler for the next call with
    the same schedule (a training loop calls ``sample`` with an unchanged scheduler thousands of times): ``float[k]``
    of scalars, ``float[k][4]`` of coefficient triples."""
    if len(rows) == 1:
        return None
    key = (device, tuple(rows))
    cached = getattr(sampler, "_table_cache", None)
    if cached is None or cached[0] != key:
        host = torch.tensor([(*r, 0.0) for r in rows] if isinstance(rows[0], tuple) else rows, dtype=torch.float32)
        cached = (key, host.to(device, non_blocking=True))
        sampler._table_cache = cached
    return cached[1]


# -------------------------------------------------------------------------------------
# fused route with diagnostics: in-kernel records
# -------------------------------------------------------------------------------------
def _record_scratch(sampler, device: torch.device, stream: int, rec_floats: int, work_doubles: int):
    """The record buffer and the merge's fp64 work row of a diagnostics call, kept on the sampler between calls of the same
    size on the same stream: the merge leaves the work row zeroed (include/ebm_hip.h), so nothing has to be allocated or
    filled per call -- on a 0.6 ms sampler call the two allocations and the fill kernel were a tenth of the records' cost.
    Keyed by the stream: calls on different streams do not share (the zeroed-after-merge contract is per stream order).
    Only SMALL buffers are kept (<= 16 MiB: the sub-millisecond calls this was built for); a large run's records (up to
    1 GiB) are per-call temporaries that go back to the caching allocator, as they did before."""
    if rec_floats * 4 > _RECORD_SCRATCH_KEEP_BYTES:
        sampler.__dict__.pop("_record_scratch_held", None)
        return (torch.empty(rec_floats, dtype=torch.float32, device=device),
                torch.zeros(work_doubles, dtype=torch.float64, device=device))
    key = (device, stream, rec_floats, work_doubles)
    held = sampler.__dict__.get("_record_scratch_held")
    if held is None or held[0] != key or sampler.__dict__.get("_record_scratch_open", False):
        # (open: the previous call did not reach its last merge -- an exception in between -- so the work row may not be zero)
        held = (key, torch.empty(rec_floats, dtype=torch.float32, device=device), torch.zeros(work_doubles, dtype=torch.float64, device=device))
        sampler.__dict__["_record_scratch_held"] = held
    sampler.__dict__["_record_scratch_open"] = True   # closed by run_with_records after its last merge
    return held[1], held[2]


def run_with_records(sampler, state, n_steps: int, thin: int, traj, diag, layout, stream, launch, pack: int = 1) -> None:
    """Diagnostics from inside the chain launch (include/ebm_hip.h: ``diag_partials``): every workgroup stores one record
    of its chains' partial sums (and, in a transition kernel, its accept count) per kept step, ``ebm_diag_finish_f32``
    merges them into ``diag`` (``"acceptance_rate"`` where it has one).  One chain launch + one merge launch per call;
    several only when the records of all kept steps would not fit ``sampler.DIAG_RECORD_BYTES``: the call is then cut at
    kept-step boundaries.  ``launch(t0, steps, traj_piece, records, first)`` runs steps ``[t0, t0 + steps)`` on ``state``.
    ``pack > 1``: the records are those of ``n / pack`` rows of ``pack`` consecutive chains each, and the ``pack``
    columns of every coordinate are pooled behind the merge."""
    n, dim = state.shape
    n_blocks, slots, block_elems = layout
    n_kept = n_steps // thin
    m_n, m_dim = n // pack, dim * pack
    rec_floats = n_blocks * (2 * slots + 8)
    chunk = max(1, min(n_kept, sampler.DIAG_RECORD_BYTES // (4 * rec_floats)))
    records, work = _record_scratch(sampler, state.device, stream, chunk * rec_floats, chunk * (3 * m_dim + 3))
    if pack > 1:
        p_mean = torch.empty(chunk, m_dim, dtype=torch.float32, device=state.device)
        p_var = torch.empty_like(p_mean)
        p_energy = torch.empty(chunk, dtype=torch.float32, device=state.device)
    rate = diag.get("acceptance_rate")
    done_keep, done_steps = 0, 0
    while done_keep < n_kept:
        kk = min(chunk, n_kept - done_keep)
        steps = kk * thin
        if done_keep + kk == n_kept:
            steps = n_steps - done_steps  # the trailing n_steps % thin steps ride along (no kept step among them)
        whole = traj is not None and kk == n_kept
        piece = traj if (traj is None or whole) else torch.empty(n, kk, dim, dtype=torch.float32, device=state.device)
        launch(done_steps, steps, piece, records, done_steps == 0)
        if traj is not None and not whole:
            traj[:, done_keep : done_keep + kk] = piece
        sl = slice(done_keep, done_keep + kk)
        mean, var, energy = (diag["mean"][sl], diag["var"][sl], diag["energy"][sl]) if pack == 1 else (p_mean, p_var, p_energy)
        _lib.call(
            "ebm_diag_finish_f32", _lib.ptr(records), kk, n_blocks, slots, block_elems, m_n, m_dim,
            _lib.ptr(mean), _lib.ptr(var), _lib.ptr(energy), None if rate is None else _lib.ptr(rate[sl]), _lib.ptr(work), stream,
        )
        if pack > 1:
            # pool the `pack` equally sized groups of every coordinate: within-group variance + variance of the group means
            gm = mean[:kk].view(kk, pack, dim).double()
            pooled = gm.mean(dim=1)
            var = var[:kk].view(kk, pack, dim).double().mean(dim=1) + (gm - pooled.unsqueeze(1)).square().mean(dim=1)
            diag["mean"][sl] = pooled.to(torch.float32)
            diag["var"][sl] = var.to(torch.float32).clamp_(min=1e-10, max=1e10)
            diag["energy"][sl] = energy[:kk] / pack  # a packed row's energy is the sum of its chains'
        done_keep += kk
        done_steps += steps
    sampler.__dict__["_record_scratch_open"] = False


# -------------------------------------------------------------------------------------
# fused route with diagnostics: passes over the state
# -------------------------------------------------------------------------------------
def run_with_state_passes(state, n_steps: int, thin: int, traj, diag, stream, launch, mean_energy, counts=None) -> None:
    """Diagnostics for the configurations without in-kernel records: one launch per ``thin`` steps, then the
    column-statistics kernel and ``mean_energy()`` on ``state``, and one launch for the trailing ``n_steps % thin`` steps.
    ``launch`` is ``run_with_records``'s (no trajectory piece, no records).  ``counts`` (``int32[n_steps]``): the accepted
    proposals of every transition, as the launches of a transition kernel left them."""
    n, dim = state.shape
    work = torch.zeros(2 * dim + 1, dtype=torch.float64, device=state.device)  # the kernel leaves it zeroed
    done = 0
    for keep in range(n_steps // thin):
        launch(done, thin, None, None, keep == 0)
        done += thin
        if traj is not None:
            traj[:, keep] = state
        if n > 1:
            _lib.call(
                "ebm_chain_stats_f32",
                _lib.ptr(state), n, dim, _lib.ptr(diag["mean"][keep]), _lib.ptr(diag["var"][keep]), _lib.ptr(work), stream,
            )
        else:
            diag["mean"][keep] = state[0]
            diag["var"][keep].zero_()
        diag["energy"][keep] = mean_energy()
        if counts is not None:
            diag["acceptance_rate"][keep] = counts[done - 1].to(torch.float32) / n
    if done < n_steps:
        launch(done, n_steps - done, None, None, False)
