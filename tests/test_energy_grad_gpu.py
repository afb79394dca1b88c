"""ebm_energy_grad_f32 on the double well, the harmonic energy, the dense Gaussian and the mixture, against float64: values at
every lane geometry, parameter placement and mixture path (csrc/rows.h eval_small / the online loop / eval_blocks), the kernel
each call launches, the exact structure of the call, rows that are not finite, and the numbers the samplers report from it.
Inputs, references, bars and mutants: tests/energy_grad_cases.py; tests/test_energy_grad_bars.py calibrates them on the CPU."""

import math

import pytest
import torch

import energy_grad_cases as eg
import torchebm_amd as ta
from chain_cases import family_of
from helpers import hip_calls, launched_kernels
from torchebm_amd import _lib

pytestmark = pytest.mark.gpu

KIND_IDS = [eg.kind_id(*k) for k in eg.KINDS]
FILL = 7.0
GUARD = 64  # floats behind every buffer (tests/test_kinetic_gpu.py)


def device_spec(s, dev):
    """(model, spec) on the device; the parameters the kernel is handed are read back and must be the ones the references use"""
    model = eg.package_model(s, dev)
    spec = model.fused_spec()
    assert spec is not None
    if s.kind == "gauss":
        assert torch.equal(spec.dev0.cpu(), s.fp[0]) and torch.equal(spec.dev1.cpu().view(s.dim, s.dim), s.fp[1])
    elif s.kind == "gmm":
        assert torch.equal(spec.dev0.cpu(), s.fp[0]) and torch.equal(spec.dev1.cpu(), s.fp[2]) and spec.n_comp == s.K
        assert tuple(spec.scalars)[:2] == (1.0 / (2.0 * s.fp[1] ** 2), 1.0 / s.fp[1] ** 2)
    return model, spec


def _guarded(dev, shape, src=None, guard=FILL):
    """A tensor of `shape` in front of GUARD floats of `guard` (in one allocation) -> (tensor, guard)."""
    numel = math.prod(shape)
    buf = torch.full((numel + GUARD,), guard, device=dev)
    t = buf[:numel].view(shape)
    if src is None:
        t.fill_(FILL)
    else:
        t.copy_(src)
    return t, buf[numel:]


def _call(spec, x, dev, want_e=True, want_g=True):
    """One ebm_energy_grad_f32 call on guarded buffers: the guard behind x is NaN (a masked slot of the last row that leaked into a
    sum shows as a non-finite output), those behind the outputs keep FILL, every output slot is written, x is untouched."""
    n, dim = x.shape
    xd, gx = _guarded(dev, (n, dim), x, guard=float("nan"))
    before = xd.clone()
    e, ge = _guarded(dev, (n,)) if want_e else (None, None)
    g, gg = _guarded(dev, (n, dim)) if want_g else (None, None)
    _lib.call("ebm_energy_grad_f32", spec.to_c(), xd.data_ptr(), n, dim, _lib.ptr(e), _lib.ptr(g), _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert torch.equal(xd.view(torch.int32), before.view(torch.int32)) and bool(torch.isnan(gx).all()), "the call wrote its input"
    for out, guard in ((e, ge), (g, gg)):
        if out is not None:
            assert bool((guard == FILL).all()), "the call wrote behind an output"
    return (None if e is None else e.cpu()), (None if g is None else g.cpu())


def _written(e, g):
    return bool(torch.isfinite(e).all()) and bool(torch.isfinite(g).all()) and not bool((e == FILL).any()) and not bool((g == FILL).any())


# ----------------------------------------------------------------------------------------------------------------
# values: every width and scale against float64, within the bars; the kernel family of every call
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,uniform", eg.KINDS, ids=KIND_IDS)
def test_energy_and_gradient_meet_the_bars(cuda_device, kind, K, uniform):
    name = eg.kind_id(kind, K, uniform)
    bar = eg.bar(kind, K, uniform)
    worst = {"energy": 0.0, "grad": 0.0}
    report, bad = [], []
    specs = {}
    for dim, scale in eg.all_cases(kind, K, uniform):
        s = eg.setup(kind, dim, K, uniform, scale)
        if dim not in specs:
            specs = {dim: device_spec(s, cuda_device)}
        e, g = _call(specs[dim][1], s.x, cuda_device)
        assert _written(e, g), s.id
        ee, egr = eg.errors(eg.reference(s), e, g)
        if kind in eg.ELEMENTWISE:
            assert torch.equal(g, eg.cpu32(s)[1]), (s.id, "the gradient is not the fp32 oracle's bit for bit")
        else:
            worst["grad"] = max(worst["grad"], egr)
        worst["energy"] = max(worst["energy"], ee)
        report.append((dim, scale, s.route, round(ee, 2), None if egr is None else round(egr, 2)))
        if ee > bar["energy"] or (egr is not None and "grad" in bar and egr > bar["grad"]):
            bad.append(report[-1])
    print("ENERGY_GRAD %s: worst energy %.3f (bar %.3f)" % (name, worst["energy"], bar["energy"]) +
          ("" if kind in eg.ELEMENTWISE else "  worst gradient %.3f (bar %.3f)" % (worst["grad"], bar["grad"])))
    print(report)
    assert not bad, bad


@pytest.mark.parametrize("kind,K,uniform", eg.KINDS, ids=KIND_IDS)
def test_every_call_is_one_kernel_of_the_recorded_family(cuda_device, kind, K, uniform):
    """one profiler session per kind; everything but the calls themselves is prepared in front of it"""
    calls = []
    for dim in eg.widths(kind, K):
        s = eg.setup(kind, dim, K, uniform, n=eg.chains_per_block(kind, dim) + 1)
        _, spec = device_spec(s, cuda_device)
        xd = s.x.to(cuda_device)
        calls.append((s, spec.to_c(), xd, torch.empty(xd.shape[0], device=cuda_device), torch.empty_like(xd)))
    stream = _lib.stream_handle(cuda_device)
    with launched_kernels() as k:
        for s, desc, xd, e, g in calls:
            _lib.call("ebm_energy_grad_f32", desc, xd.data_ptr(), xd.shape[0], s.dim, e.data_ptr(), g.data_ptr(), stream)
    families = [family_of(name).split("<")[0] for name in k.names]
    assert families == [eg.FAMILY[s.route] for s, *_ in calls], list(zip([s.id for s, *_ in calls], k.names))
    assert {s.route for s, *_ in calls} == {eg.route(kind, d) for d in eg.widths(kind, K)}


# ----------------------------------------------------------------------------------------------------------------
# structure (exact)
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,uniform", eg.KINDS, ids=KIND_IDS)
def test_structure(cuda_device, kind, K, uniform):
    dev = cuda_device
    for dim in eg.struct_widths(kind, K):
        s = eg.setup(kind, dim, K, uniform, eg.SCALES[1])
        _, spec = device_spec(s, dev)
        e, g = _call(spec, s.x, dev)
        assert _written(e, g), s.id
        # either output alone is the joint call's
        e1, none = _call(spec, s.x, dev, want_g=False)
        none2, g1 = _call(spec, s.x, dev, want_e=False)
        assert none is None and none2 is None and torch.equal(e1, e) and torch.equal(g1, g), s.id
        # the first n rows alone, n around one block's chains: a chain's outputs depend on its own row only
        for n in eg.n_edges(kind, dim):
            en, gn = _call(spec, s.x[:n], dev)
            assert torch.equal(en, e[:n]) and torch.equal(gn, g[:n]), (s.id, n)
        # rows [lo:hi] alone: other blocks, other places in the wave
        c = eg.chains_per_block(kind, dim)
        for lo, hi in ((1, 2), (c - 1 if c > 1 else 2, 2 * c + 3), (eg.N - 5, eg.N)):
            lo, hi = min(lo, eg.N - 1), min(hi, eg.N)
            el, gl = _call(spec, s.x[lo:hi].contiguous(), dev)
            assert torch.equal(el, e[lo:hi]) and torch.equal(gl, g[lo:hi]), (s.id, lo, hi)


# ----------------------------------------------------------------------------------------------------------------
# rows that are not finite stay where they are
# ----------------------------------------------------------------------------------------------------------------
NONFINITE = [("gauss", 0, 16), ("gauss", 0, 257), ("gauss", 0, 256), ("gmm", 8, 16), ("gmm", 8, 257), ("gmm", 16, 16), ("gmm", 16, 257),
             ("gmm", 9, 16), ("gmm", 9, 257)]


@pytest.mark.parametrize("kind,K,dim", NONFINITE, ids=[f"{eg.kind_id(k, K)}-d{d}" for k, K, d in NONFINITE])
def test_a_row_that_is_not_finite_leaves_the_others_alone(cuda_device, kind, K, dim):
    """one NaN coordinate in one chain, 1e20 in another (its square overflows in a mixture's distance): every other chain's outputs
    are bitwise those of the clean call -- at a width with several chains per wave (16 dims: sixteen) and at one with a chain per wave"""
    s = eg.setup(kind, dim, K)
    _, spec = device_spec(s, cuda_device)
    e, g = _call(spec, s.x, cuda_device)
    x = s.x.clone()
    rows = (1, 34, eg.N - 1)
    x[rows[0], dim // 2] = float("nan")
    x[rows[1], dim - 1] = 1e20
    x[rows[2], 0] = float("nan")
    eb, gb = _call(spec, x, cuda_device)
    clean = torch.ones(eg.N, dtype=torch.bool)
    clean[list(rows)] = False
    assert torch.equal(eb[clean], e[clean]) and torch.equal(gb[clean], g[clean]), s.id
    # (the three rows themselves did change: the inputs took)
    assert bool(torch.isnan(eb[rows[0]])) and bool(torch.isnan(eb[rows[2]])) and eb[rows[1]].item() != e[rows[1]].item(), eb[list(rows)]


# ----------------------------------------------------------------------------------------------------------------
# through the samplers
# ----------------------------------------------------------------------------------------------------------------
SAMPLER_CASES = [("double_well", 0, 5), ("harmonic", 0, 100), ("gauss", 0, 5), ("gauss", 0, 100), ("gmm", 8, 100), ("gmm", 16, 5)]


def _step_sizes(s):
    """(Langevin eta, HMC eps): small enough that a handful of steps keep the states where the inputs are"""
    if s.kind == "gauss":
        lam = torch.linalg.eigvalsh(s.fp[1].double()).max().item()
        return 0.25 / lam, 0.25 / math.sqrt(lam)
    return {"double_well": (0.005, 0.03), "harmonic": (0.05, 0.1), "gmm": (0.02, 0.1)}[s.kind]


@pytest.mark.parametrize("kind,K,dim", SAMPLER_CASES, ids=[f"{eg.kind_id(k, K)}-d{d}" for k, K, d in SAMPLER_CASES])
def test_sampler_diagnostics_report_the_float64_mean_energy(cuda_device, kind, K, dim):
    """diag["energy"][j] is the mean energy of the kept states traj[:, j] the same call returned, in float64, within the energy bar
    of every chain and one fp32 rounding of the mean"""
    dev = cuda_device
    s = eg.setup(kind, dim, K)
    model, _ = device_spec(s, dev)
    eta, eps = _step_sizes(s)
    x0 = s.x.to(dev)
    runs = (("langevin", ta.LangevinDynamics(model, step_size=eta, device=dev), dict(n_steps=7, thin=2)),
            ("hmc", ta.HamiltonianMonteCarlo(model, step_size=eps, n_leapfrog_steps=3, device=dev), dict(n_steps=5, thin=2)))
    for what, sampler, kw in runs:
        traj, diag = sampler.sample(x=x0.clone(), return_trajectory=True, return_diagnostics=True,
                                    generator=torch.Generator(device=dev).manual_seed(5), **kw)
        kept = kw["n_steps"] // kw["thin"]
        assert traj.shape == (eg.N, kept, dim) and diag["energy"].shape == (kept,)
        assert not torch.equal(traj[:, 0], x0)
        for j in range(kept):
            want, bar = eg.mean_energy_bar(s, traj[:, j].cpu())
            got = diag["energy"][j].item()
            print(s.id, what, "kept", j, "mean energy", got, "float64", want, "error / bar %.3f" % (abs(got - want) / bar))
            assert abs(got - want) <= bar, (s.id, what, j, got, want, bar)


@pytest.mark.parametrize("dim,entry", [(128, False), (132, True), (256, True), (260, False)])
def test_gaussian_model_gradient(cuda_device, dim, entry):
    """GaussianModel.gradient() is one ebm_energy_grad_f32 call at 132 and 256 dims and none at 128 (autograd) and 260 (one GEMM);
    the same gradient bar either way"""
    s = eg.setup("gauss", dim)
    model, _ = device_spec(s, cuda_device)
    x = s.x.to(cuda_device)
    before = hip_calls("ebm_energy_grad_f32")
    g = model.gradient(x)
    assert hip_calls("ebm_energy_grad_f32") - before == (1 if entry else 0)
    _, err = eg.errors(eg.reference(s), torch.zeros(eg.N), g.cpu())
    print("GaussianModel.gradient at", dim, "dims: worst error %.3f (bar %.3f)" % (err, eg.bar("gauss")["grad"]))
    assert err <= eg.bar("gauss")["grad"], (dim, err)
