"""The fused descent launch (ebm_descent_chain_f32, csrc/rows_langevin.hip descent_chain_rows_kernel) and the samplers that
drive it (samplers/descent.py _run_fused), against float64: accuracy of k steps at every energy kind and lane geometry,
the exact structure of the call (trajectory / thin bookkeeping, eta table, partial blocks), and the three launch plans of the
host side.  Inputs, references and bars: tests/descent_cases.py; tests/test_descent_bars.py calibrates them on the CPU."""

import pytest
import torch

import descent_cases as dc
import oracle
from helpers import hip_calls, yardstick
from torchebm_amd.core.schedules import LinearScheduler
from torchebm_amd.samplers import GradientDescentSampler, NesterovSampler

pytestmark = pytest.mark.gpu

ENERGY_IDS = [f"{k}{K or ''}" for k, K in dc.ENERGIES]
MODES = pytest.mark.parametrize("nesterov", [False, True], ids=["gd", "nesterov"])


def device_spec(s, dev):
    """(model, spec): the package model on the device; for the Gaussian and the mixtures the parameters the kernel is handed
    are read back and must be the ones the references use"""
    model = dc.package_model(s, dev)
    spec = model.fused_spec()
    assert spec is not None
    if s.kind == "gauss":
        assert torch.equal(spec.dev0.cpu(), s.fp[0]) and torch.equal(spec.dev1.cpu().view(s.dim, s.dim), s.fp[1])
    elif s.kind == "gmm":
        assert torch.equal(spec.dev0.cpu(), s.fp[0]) and torch.equal(spec.dev1.cpu(), s.fp[2])
    return model, spec


# ----------------------------------------------------------------------------------------------------------------
# accuracy: six steps under a non-constant eta table, every energy kind, every width, both update rules
# ----------------------------------------------------------------------------------------------------------------
def _accuracy(kind, dim, K, nesterov, dev):
    s = dc.setup(kind, dim, K)
    model, spec = device_spec(s, dev)
    got, _, _, _ = dc.launch(spec, s.x0, dc.K_STEPS, dev, table=s.etas, nesterov=nesterov)
    r32, r64 = dc.refs(kind, dim, K, nesterov)
    what = f"{kind}{K or ''}-d{dim}-{'nesterov' if nesterov else 'gd'}"
    if kind in dc.EXACT:
        assert torch.equal(got, r32), what
    st = yardstick(got, r32, r64, what=what, **dc.yardstick_factors(kind, K))
    return {"what": what, "med": st["hip_med"] / st["ref_med"], "q90": st["hip_q90"] / st["ref_q90"], "max": st["hip_max"] / st["ref_max"]}


ACCURACY_CASES = [(k, K, d) for k, K in dc.ENERGIES for d in dc.widths(k)]


@MODES
@pytest.mark.parametrize("kind,K,dim", ACCURACY_CASES, ids=[f"{k}{K or ''}-d{d}" for k, K, d in ACCURACY_CASES])
def test_six_steps_against_float64(cuda_device, kind, K, dim, nesterov):
    print("DESCENT %(what)s: kernel error / fp32 reference error: median %(med).2f q90 %(q90).2f max %(max).2f"
          % _accuracy(kind, dim, K, nesterov, cuda_device))


@MODES
def test_padded_mixture_against_float64(cuda_device, nesterov):
    kind, K, dim = dc.GMM_PADDED
    print(_accuracy(kind, dim, K, nesterov, cuda_device))


# ----------------------------------------------------------------------------------------------------------------
# structure (exact)
# ----------------------------------------------------------------------------------------------------------------
def _structure(kind, dim, K, nesterov, dev):
    s = dc.setup(kind, dim, K)
    model, spec = device_spec(s, dev)
    etas = dc.eta_table(s.etas[0], 7)
    kw = dict(nesterov=nesterov)
    tag = (kind, K, dim, nesterov)

    # trajectory and thin: row j of a (k = 7, thin = 2) call is the state after 2 (j + 1) steps; the state returned is the
    # 7-step one; three rows per chain are written and nothing behind them or behind the state
    x7, traj, pad_x, pad_t = dc.launch(spec, s.x0, 7, dev, table=etas, thin=2, traj=True, pad=5, **kw)
    assert traj.shape == (s.n, 3, dim)
    assert bool((pad_x == dc.SENTINEL).all()) and bool((pad_t == dc.SENTINEL).all()), tag
    assert not bool((traj == dc.SENTINEL).any()), tag
    for j in range(3):
        xj, _, _, _ = dc.launch(spec, s.x0, 2 * (j + 1), dev, table=etas[: 2 * (j + 1)], **kw)
        assert torch.equal(traj[:, j], xj), (tag, "trajectory row", j)
    plain7, _, pad_x, _ = dc.launch(spec, s.x0, 7, dev, table=etas, pad=5, **kw)
    assert torch.equal(x7, plain7) and not torch.equal(x7, traj[:, 2]), tag
    assert bool((pad_x == dc.SENTINEL).all()), tag

    # a constant table is the scalar call
    const, _, _, _ = dc.launch(spec, s.x0, 5, dev, table=[etas[1]] * 5, **kw)
    scalar, _, _, _ = dc.launch(spec, s.x0, 5, dev, eta=etas[1], **kw)
    assert torch.equal(const, scalar), (tag, "constant table")

    # plain descent has no state but x: a k-step table call is k one-step scalar calls
    if not nesterov:
        x = s.x0
        for e in etas:
            x, _, _, _ = dc.launch(spec, x, 1, dev, eta=e)
        assert torch.equal(x, plain7), (tag, "step by step")

    # the first 77 chains of the call are a 77-chain call (partial blocks, inactive lanes)
    part, _, _, _ = dc.launch(spec, s.x0[:77], 7, dev, table=etas, **kw)
    assert torch.equal(part, plain7[:77]), (tag, "77 chains")

    # one block holds four chains at G = 64
    if dim == 256:
        for n in (1, 3, 4, 5):
            few, tr, _, _ = dc.launch(spec, s.x0[:n], 7, dev, table=etas, thin=2, traj=True, **kw)
            assert torch.equal(few, plain7[:n]) and torch.equal(tr, traj[:n]), (tag, n, "chains")


@MODES
@pytest.mark.parametrize("kind,K", dc.ENERGIES, ids=ENERGY_IDS)
def test_structure(cuda_device, kind, K, nesterov):
    for dim in dc.widths(kind, dc.STRUCT_WIDTHS):
        _structure(kind, dim, K, nesterov, cuda_device)


# ----------------------------------------------------------------------------------------------------------------
# the samplers: three launch plans (one launch; one launch per `thin` steps on a sliced eta table -- diagnostics without
# momentum; one launch and energies read off the trajectory -- Nesterov with diagnostics) and the trailing launch
# ----------------------------------------------------------------------------------------------------------------
SAMPLER_CASES = [("gauss", 0, 100), ("gmm", 16, 64), ("rosenbrock", 0, 33)]
N_STEPS, THIN = 11, 3


def _sampler(s, nesterov, dev):
    model = dc.package_model(s, dev)
    sched = LinearScheduler(s.etas[0], 0.5 * s.etas[0], N_STEPS)
    if nesterov:
        return NesterovSampler(model, step_size=sched, momentum=dc.MU, device=dev)
    return GradientDescentSampler(model, step_size=sched, device=dev)


@MODES
@pytest.mark.parametrize("kind,K,dim", SAMPLER_CASES, ids=[f"{k}{K or ''}-d{d}" for k, K, d in SAMPLER_CASES])
def test_samplers(cuda_device, kind, K, dim, nesterov):
    s = dc.setup(kind, dim, K)
    device_spec(s, cuda_device)
    smp = _sampler(s, nesterov, cuda_device)
    x0 = s.x0.to(cuda_device)
    keep = x0.clone()
    kept = N_STEPS // THIN
    name = "ebm_descent_chain_f32"

    # trajectory and diagnostics: gradient descent launches once per kept step and once for the two trailing steps,
    # Nesterov once (its velocity lives inside the launch)
    before = hip_calls(name)
    traj, diag = smp.sample(x=x0, n_steps=N_STEPS, thin=THIN, return_trajectory=True, return_diagnostics=True)
    assert hip_calls(name) - before == (1 if nesterov else kept + 1)
    value_after = smp.schedulers["step_size"].get_value()
    # diagnostics only: the same plans without the caller's trajectory; the state returned is the 11-step one
    before = hip_calls(name)
    final, diag2 = smp.sample(x=x0, n_steps=N_STEPS, thin=THIN, return_diagnostics=True)
    assert hip_calls(name) - before == (1 if nesterov else kept + 1)
    # neither: one launch
    before = hip_calls(name)
    final1 = smp.sample(x=x0, n_steps=N_STEPS, thin=THIN)
    assert hip_calls(name) - before == 1
    before = hip_calls(name)
    traj1 = smp.sample(x=x0, n_steps=N_STEPS, thin=THIN, return_trajectory=True)
    assert hip_calls(name) - before == 1
    assert torch.equal(x0, keep), "the caller's x was written"
    assert traj.shape == (s.n, kept, dim) and set(diag) == {"energy"} and diag["energy"].shape == (kept,)
    assert torch.equal(final, final1) and torch.equal(traj, traj1) and torch.equal(diag["energy"], diag2["energy"])

    # float64: trajectory and final state on the yardstick of the direct calls
    cpu = _sampler(s, nesterov, None)
    etas = cpu.schedulers["step_size"].preview(N_STEPS)
    mom = dc.MU if nesterov else None
    x32, t32, _ = oracle.descent_chain(dc.oracle32(s), s.x0, etas, mom, THIN, want_traj=True)
    x64, t64, _ = oracle.descent_chain(dc.oracle64(s), s.x0.double(), etas, mom, THIN, want_traj=True)
    factors = dc.yardstick_factors(kind, K)
    print(yardstick(final.cpu(), x32, x64, what=f"sampler {kind} final", **factors))
    print(yardstick(traj.cpu().reshape(s.n, -1), t32.reshape(s.n, -1), t64.reshape(s.n, -1), what=f"sampler {kind} trajectory", **factors))
    assert not torch.equal(final.cpu(), traj[:, -1].cpu())  # two trailing steps after the last kept one

    # diag["energy"]: the mean energy of the kept states the call itself stored, in float64
    for j in range(kept):
        want, bar = dc.mean_energy_bar(s, traj[:, j].cpu())
        got = diag["energy"][j].item()
        print(kind, "nesterov" if nesterov else "gd", "kept", j, "mean energy", got, "float64", want, "bar", bar)
        assert abs(got - want) <= bar, (kind, j)

    # the scheduler ends where the CPU route's does
    cpu.sample(x=s.x0, n_steps=N_STEPS, thin=THIN)
    assert value_after == cpu.schedulers["step_size"].get_value() == 0.5 * s.etas[0]  # the ramp's end value, reached at step 11

    # two 5-step calls that go on with the schedule are one 10-step call (plain descent: a Nesterov call restarts v at zero)
    if not nesterov:
        ten = smp.sample(x=x0, n_steps=10)
        smp.reset_schedulers()
        half = smp.sample(x=x0, n_steps=5, reset_schedulers=False)
        both = smp.sample(x=half, n_steps=5, reset_schedulers=False)
        assert torch.equal(both, ten)
