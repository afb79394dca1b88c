"""The tempered kernels (ebm_tempering_chain_f32, ebm_tempering_hmc_chain_f32, ebm_ais_chain_f32) on the two landscapes with a
structure along the row: Rosenbrock, the one kind with a neighbour exchange (DPP row shifts up to G = 16, a __shfl rotation
above, the wrap into the next vector of lane 0), and Ackley, whose mean runs over dim and whose gradient at the origin is NaN
under a finite energy.  Every lane geometry, with the ladder layout's idle groups behind the walkers.

The runs and their bars are the three families' own (test_tempering_gpu.py, test_tempering_hmc_gpu.py, test_ais_gpu.py): the
checks on a run with injected draws are the functions check_langevin / check_hmc / check_ais below, which
tests/test_tempered_landscape_bars.py feeds deliberately wrong energies on the CPU."""

from types import SimpleNamespace

import pytest
import torch

import ais_cases
import tempering_cases
import tempering_hmc_cases
import test_ais_gpu as ais_gpu
import test_landscape_gpu as landscape_gpu
import test_tempering_gpu as lan_gpu
import test_tempering_hmc_gpu as hmc_gpu
import torchebm_amd as ta
from helpers import hip_calls, yardstick
from tempering_cases import MARGIN_BAR, TEMPS, energy_spec, model_of, oracle_of, start_scale
from torchebm_amd import _lib

pytestmark = pytest.mark.gpu

KINDS = ("rosenbrock", "ackley")
DIMS = (2, 5, 12, 32, 64, 100, 256)  # G = 1, 2, 4, 8, 16, 32, 64 with one vector per lane; the Langevin ladder adds 260 (two)


# ---------------------------------------------------------------------------------
# injected draws: what a run is held to (the GPU tests below on the kernels, the CPU bars file on wrong energies)
# ---------------------------------------------------------------------------------
def check_langevin(c, x, counts):
    """test_tempering_gpu.py::test_coupled_energies_against_float64."""
    (n, R, dim), kind = c["shape"], c["spec"]["kind"]
    lan_gpu.check_decisions(c, x, counts)
    rows = lambda t: t.reshape(n * R, dim)  # noqa: E731
    return [yardstick(rows(x), rows(c["ref32"]["x"]), rows(c["ref64"]["x"]), k_med=1.5, what=f"{kind} dim {dim} R {R}")]


def check_hmc(c, got):
    """test_tempering_hmc_gpu.py::test_cases_with_injected_draws."""
    (n, R, dim), kind = c["shape"], c["spec"]["kind"]
    ref32, ref64 = c["ref32"], c["ref64"]
    assert tempering_hmc_cases.closest_call(ref64) > MARGIN_BAR, c["seed"]
    assert torch.equal(ref32["accepted"], ref64["accepted"]) and torch.equal(ref32["mask"], ref64["mask"])
    if n >= 37:  # the case exercises both outcomes of both decisions
        assert 0 < ref32["accepted"].sum() < ref32["accepted"].numel()
        assert 0 < ref32["mask"].sum() < hmc_gpu.want_swap_counts(ref32["mask"], n, R)[: R - 1].sum()
    hmc_gpu.check_decisions(got, ref32, n, R)
    assert torch.equal(hmc_gpu.slot_of_each_state(got["x"], ref32["x"]), torch.arange(R).expand(n, R))
    rows = lambda t: t.reshape(-1, dim)  # noqa: E731
    return [yardstick(rows(got["x"]), rows(ref32["x"]), rows(ref64["x"]), k_med=2.0, what=f"{kind} dim {dim} R {R} states"),
            yardstick(rows(got["traj"]), rows(ref32["traj"]), rows(ref64["traj"]), k_med=2.0, what=f"{kind} dim {dim} R {R} slot 0 kept")]


def check_ais(c, got):
    """test_ais_gpu.py::test_cases_with_injected_draws."""
    (n, dim), T, kind = c["shape"], c["T"], c["spec"]["kind"]
    ref32, ref64 = c["ref32"], c["ref64"]
    assert ref64["margin"].min().item() > MARGIN_BAR, c["seed"]
    assert torch.equal(ref32["accepted"], ref64["accepted"])
    if n >= 37 and T >= 3:  # the case exercises both outcomes of the decision
        assert 0 < ref32["accepted"].sum() < ref32["accepted"].numel()
    assert torch.equal(got["accepted"], ref32["accepted"])
    assert torch.equal(got["counts"], ref32["accepted"].sum(dim=1).long())
    return [yardstick(got["x"], ref32["x"], ref64["x"], k_med=2.0, what=f"{kind} dim {dim} T {T} states"),
            yardstick(got["logw"][:, None], ref32["logw"][:, None], ref64["logw"][:, None], k_med=2.0, what=f"{kind} dim {dim} T {T} logw")]


@pytest.mark.parametrize("kind,dim,R,n,swap_every,k", tempering_cases.LANDSCAPE_CASES)
def test_langevin_ladder_with_injected_draws(cuda_device, kind, dim, R, n, swap_every, k):
    c = tempering_cases.case(kind, dim, R, n, swap_every, k)
    x, counts, _ = lan_gpu.run_kernel(cuda_device, c["spec"], c["x0"], c["temps"], k, swap_every, noise=c["noise"], u=c["u"])
    print(check_langevin(c, x, counts))


@pytest.mark.parametrize("kind,dim,R,n,swap_every,n_mh", tempering_hmc_cases.LANDSCAPE_CASES)
def test_hmc_ladder_with_injected_draws(cuda_device, kind, dim, R, n, swap_every, n_mh):
    c = tempering_hmc_cases.case(kind, dim, R, n, swap_every, n_mh)
    got = hmc_gpu.run_kernel(cuda_device, c["spec"], c["x0"], c["temps"], c["eps"], c["L"], n_mh, swap_every, z=c["z"],
                             ua=c["u_accept"], us=c["u_swap"], thin=2)
    print(check_hmc(c, got))


@pytest.mark.parametrize("kind,dim,n,T", ais_cases.LANDSCAPE_CASES)
def test_ais_with_injected_draws(cuda_device, kind, dim, n, T):
    c = ais_cases.case(kind, dim, n, T)
    got = ais_gpu.run_kernel(cuda_device, c["spec"], n, dim, c["betas"], c["eps"], c["L"], c["base_std"], x0=c["x0"], z=c["z"], u=c["u"])
    print(check_ais(c, got))


# ---------------------------------------------------------------------------------
# bitwise identities against the plain kernels, which test_landscape_gpu.py holds to float64 at every geometry: a wrong
# neighbour or a wrong mean in the ladder layout shows at once
# ---------------------------------------------------------------------------------
def identity_inputs(kind, dim, family):
    """Starts and draws of the identity tests, at the cases' own step sizes.  On the CPU restatement
    (tests/test_tempered_landscape_bars.py) the HMC transitions reject 30 - 153 of 555 proposals (465 and 2169 of 3855 at dim 2)
    and the one AIS transition, which jumps from the base to the target, 7 - 105 of 111."""
    g = torch.Generator().manual_seed(21 + dim)
    n, R = (257 if dim == 2 else 37), 3
    if family == "langevin":
        k = 4
        return {"x0": start_scale(kind) * torch.randn(n, R, dim, generator=g), "noise": torch.randn(k, n, R, dim, generator=g), "k": k}
    if family == "hmc":
        n_mh, L = 5, 4
        return {"x0": start_scale(kind) * torch.randn(n, R, dim, generator=g), "z": torch.randn(n_mh, n, R, dim, generator=g),
                "ua": torch.rand(n_mh, n, R, generator=g), "n_mh": n_mh, "L": L, "eps": tempering_hmc_cases.step_sizes(kind, dim, 1)[0]}
    n, s0 = 111, ais_cases.base_std_of(kind)
    return {"x0": ais_cases.f32(s0) * torch.randn(n, dim, generator=g), "z": torch.randn(1, n, dim, generator=g),
            "u": torch.rand(1, n, generator=g), "L": 4, "eps": ais_cases.step_sizes(kind, dim, 1)[0], "base_std": s0}


@pytest.mark.parametrize("kind", KINDS)
def test_ladder_without_swaps_is_the_langevin_kernel(cuda_device, kind):
    """swap_every > k: slot r's rows are ebm_langevin_chain_f32 on those rows with noise_coef_r, bit for bit.  R = 3: idle lane
    groups sit behind the ladders of a workgroup at every G."""
    dev, R = cuda_device, 3
    for dim in DIMS + (260,):
        i, spec = identity_inputs(kind, dim, "langevin"), energy_spec(kind, dim)
        n, k = i["x0"].shape[0], i["k"]
        x, counts, _ = lan_gpu.run_kernel(dev, spec, i["x0"], TEMPS[R], k, 100, noise=i["noise"], u=torch.zeros(0, n, R))
        assert counts.sum() == 0 and torch.isfinite(x).all() and not torch.equal(x, i["x0"])
        coef, _ = tempering_cases.ladder(tempering_cases.SIGMA, TEMPS[R])
        spec_c = model_of(spec, dev).fused_spec().to_c()
        eta = tempering_cases.ETA
        for r in range(R):
            rows = i["x0"][:, r].contiguous().to(dev)
            eps = i["noise"][:, :, r].contiguous().to(dev)
            _lib.call("ebm_langevin_chain_f32", spec_c, rows.data_ptr(), n, dim, k, eta, eta**0.5, coef[r].item(), None, 0, 0.0, 0.0, 1,
                      None, None, eps.data_ptr(), 0, 0, _lib.stream_handle(dev))
            torch.cuda.synchronize()
            assert torch.equal(rows.cpu(), x[:, r]), (kind, dim, r)


@pytest.mark.parametrize("kind", KINDS)
def test_the_tempered_transition_is_the_hmc_kernels(cuda_device, kind):
    """sqrt_temp = beta = 1 in every slot and no event: the rows are ebm_hmc_chain_f32 chains, bit for bit."""
    dev, R = cuda_device, 3
    ones = (torch.ones(R), torch.ones(R))
    for dim in DIMS:
        i, spec = identity_inputs(kind, dim, "hmc"), energy_spec(kind, dim)
        n, n_mh, L, eps = i["x0"].shape[0], i["n_mh"], i["L"], i["eps"]
        got = hmc_gpu.run_kernel(dev, spec, i["x0"], None, (eps,) * R, L, n_mh, n_mh + 1, z=i["z"], ua=i["ua"], us=torch.zeros(0, n, R),
                                 coefficients=ones)
        assert got["swaps"].sum() == 0
        rows, p_d, u_d = i["x0"].view(n * R, dim).to(dev).clone(), i["z"].view(n_mh, n * R, dim).to(dev), i["ua"].view(n_mh, n * R).to(dev)
        mask = torch.empty(n_mh, n * R, dtype=torch.uint8, device=dev)
        _lib.call("ebm_hmc_chain_f32", model_of(spec, dev).fused_spec().to_c(), rows.data_ptr(), n * R, dim, n_mh, L, ais_cases.f32(eps),
                  None, 0, 0.0, None, 1, None, None, mask.data_ptr(), None, p_d.data_ptr(), u_d.data_ptr(), 0, 0, _lib.stream_handle(dev))
        torch.cuda.synchronize()
        assert torch.equal(mask.cpu().bool().view(n_mh, n, R), got["accepted"]), (kind, dim)
        assert (~got["accepted"]).any() and got["accepted"].any(), (kind, dim)
        assert torch.equal(rows.cpu().view(n, R, dim), got["x"]), (kind, dim)


@pytest.mark.parametrize("kind", KINDS)
def test_ais_at_beta_one_is_the_hmc_kernels_transition(cuda_device, kind):
    """The table (0, 1): the one transition runs at beta = 1, where the mix 0 * a + 1 * b is exact -- the final state is that of
    one ebm_hmc_chain_f32 transition, bit for bit, and the weight is E_0(x0) - E(x0)."""
    dev = cuda_device
    for dim in DIMS:
        i, spec = identity_inputs(kind, dim, "ais"), energy_spec(kind, dim)
        n, L, eps, s0 = i["x0"].shape[0], i["L"], ais_cases.f32(i["eps"]), i["base_std"]
        got = ais_gpu.run_kernel(dev, spec, n, dim, torch.tensor([0.0, 1.0]), (eps,), L, s0, x0=i["x0"], z=i["z"], u=i["u"])
        rows, p_d, u_d = i["x0"].to(dev).clone(), i["z"].to(dev), i["u"].to(dev)
        mask = torch.empty(1, n, dtype=torch.uint8, device=dev)
        _lib.call("ebm_hmc_chain_f32", model_of(spec, dev).fused_spec().to_c(), rows.data_ptr(), n, dim, 1, L, eps, None, 0, 0.0,
                  None, 1, None, None, mask.data_ptr(), None, p_d.data_ptr(), u_d.data_ptr(), 0, 0, _lib.stream_handle(dev))
        torch.cuda.synchronize()
        assert torch.equal(mask.cpu().bool(), got["accepted"]), (kind, dim)
        assert (~got["accepted"]).any() and got["accepted"].any(), (kind, dim)
        assert torch.equal(rows.cpu(), got["x"]), (kind, dim)
        want = 0.5 * ais_cases.f32(1.0 / s0**2) * i["x0"].double().square().sum(dim=1) - oracle_of(spec).energy(i["x0"].double())
        assert torch.allclose(got["logw"].double(), want, rtol=1e-5, atol=1e-5), (kind, dim)


# ---------------------------------------------------------------------------------
# native draws are the materialised Philox fields, and a sub-block run alone reproduces its rows: the three families' own
# tests at a dim with a masked row.  On the CPU restatement with torch's draws (Rosenbrock dim 12 / Ackley dim 100) these accept
# 115 - 132 of 222 / 138 - 146 of 148 swaps (Langevin), reject 147 - 162 of 592 / 34 - 45 of 444 proposals and accept 114 - 117 / 74 - 89
# swaps (HMC), and reject 74 - 80 / 40 - 52 of 148 proposals (AIS)
# ---------------------------------------------------------------------------------
NATIVE = {"rosenbrock": 12, "ackley": 100}


@pytest.mark.parametrize("kind", KINDS)
def test_native_draws_langevin_ladder(cuda_device, kind):
    dim = NATIVE[kind]
    R = 4 if dim == 12 else 3
    lan_gpu.test_native_draws_are_the_materialised_field(cuda_device, kind, dim, R, 37, 1, 4)


@pytest.mark.parametrize("kind", KINDS)
def test_native_draws_hmc_ladder(cuda_device, kind):
    dim = NATIVE[kind]
    R = 4 if dim == 12 else 3
    hmc_gpu.test_native_draws_are_the_materialised_fields(cuda_device, kind, dim, R, 37, (1.0, 2.0, 4.0, 8.0)[:R], 1, 4, 1.0)


@pytest.mark.parametrize("kind", KINDS)
def test_native_draws_ais(cuda_device, kind):
    ais_gpu.test_native_draws_are_the_materialised_fields(cuda_device, kind, NATIVE[kind], 37, 4, 1.5, ais_cases.base_std_of(kind))


@pytest.mark.parametrize("kind,dim,R,n", [("rosenbrock", 12, 4, 37), ("ackley", 100, 3, 37)])
def test_both_ladders_take_the_same_swap_decisions(cuda_device, kind, dim, R, n):
    hmc_gpu.test_both_ladders_take_the_same_swap_decisions(cuda_device, kind, dim, R, n)


# ---------------------------------------------------------------------------------
# check values and safe mode: states whose energy does not vouch for their gradient
# ---------------------------------------------------------------------------------
WILD = (3, 7)  # the ladders / chains that get a wild start


def wild_ladders(kind, x0):
    """x0 [n, R, dim] with the wild starts of the kind put in: Ackley, slot 1 of ladder 3 exactly at the origin (a finite energy
    over a NaN gradient); Rosenbrock, x_0 = 1e13 in slot 1 of ladder 3 (the gradient overflows) and x_{dim-1} = 3e19 in slot 0
    of ladder 7 (an infinite energy over a finite gradient)."""
    x0 = x0.clone()
    if kind == "ackley":
        x0[3, 1] = 0.0
    else:
        x0[3, 1, 0] = 1.0e13
        x0[7, 0, -1] = 3.0e19
    return x0


def wild_chains(kind, x0):
    """The same for the chains x0 [n, dim] of an AIS run: chain 3 at the origin; x_0 = 1e13 in chain 3, x_{dim-1} = 3e19 in chain 7."""
    x0 = x0.clone()
    if kind == "ackley":
        x0[3] = 0.0
    else:
        x0[3, 0] = 1.0e13
        x0[7, -1] = 3.0e19
    return x0


def _safe(want_x, want_accepted, want_margin, got_x, got_accepted, wild):
    """test_landscape_gpu._compare_safe on rows [m, dim] and masks [T, m]."""
    ref = {"x": want_x, "accepted": want_accepted, "margins": want_margin}
    landscape_gpu._compare_safe(ref, SimpleNamespace(x=got_x, mask=got_accepted), wild)


@pytest.mark.parametrize("dim", [5, 100])
@pytest.mark.parametrize("kind", KINDS)
def test_hmc_ladder_safe_mode(cuda_device, kind, dim):
    shape = next(s for s in tempering_hmc_cases.LANDSCAPE_CASES if s[:2] == (kind, dim) and s[3] >= 37)
    _, _, R, n, se, n_mh = shape
    c = tempering_hmc_cases.case(*shape)
    x0 = wild_ladders(kind, c["x0"])
    want = tempering_hmc_cases.restate(oracle_of(c["spec"]), x0, c["z"], c["u_accept"], c["u_swap"], c["eps"], c["L"], c["temps"], se,
                                       torch.float32)
    assert (want["margin"] > MARGIN_BAR).all(), "a swap decision of the restatement is borderline"
    kw = dict(z=c["z"], ua=c["u_accept"], us=c["u_swap"])
    got = hmc_gpu.run_kernel(cuda_device, c["spec"], x0, c["temps"], c["eps"], c["L"], n_mh, se, **kw)
    clean = hmc_gpu.run_kernel(cuda_device, c["spec"], c["x0"], c["temps"], c["eps"], c["L"], n_mh, se, **kw)
    wild = torch.zeros(n, R, dtype=torch.bool)
    wild[list(WILD)] = True
    _safe(want["x"].view(n * R, dim), want["accepted"].view(n_mh, n * R), want["mh_margin"].view(n_mh, n * R), got["x"].view(n * R, dim),
          got["accepted"].view(n_mh, n * R), wild.view(n * R))
    assert torch.equal(got["swaps"], hmc_gpu.want_swap_counts(want["mask"], n, R)), (got["swaps"], hmc_gpu.want_swap_counts(want["mask"], n, R))
    others = [i for i in range(n) if i not in WILD]
    assert torch.equal(got["x"][others], clean["x"][others]) and torch.isfinite(clean["x"]).all()
    assert torch.equal(got["accepted"][:, others], clean["accepted"][:, others])


@pytest.mark.parametrize("dim", [5, 100])
@pytest.mark.parametrize("kind", KINDS)
def test_ais_safe_mode(cuda_device, kind, dim):
    shape = next(s for s in ais_cases.LANDSCAPE_CASES if s[:2] == (kind, dim) and s[2] >= 37)
    _, _, n, T = shape
    c = ais_cases.case(*shape)
    x0 = wild_chains(kind, c["x0"])
    want = ais_cases.restate(oracle_of(c["spec"]), x0, c["z"], c["u"], c["betas"], c["eps"], c["L"], c["base_std"], torch.float32)
    args = (cuda_device, c["spec"], n, dim, c["betas"], c["eps"], c["L"], c["base_std"])
    got = ais_gpu.run_kernel(*args, x0=x0, z=c["z"], u=c["u"])
    clean = ais_gpu.run_kernel(*args, x0=c["x0"], z=c["z"], u=c["u"])
    wild = torch.zeros(n, dtype=torch.bool)
    wild[list(WILD)] = True
    _safe(want["x"], want["accepted"], want["margin"], got["x"], got["accepted"], wild)
    _safe(want["logw"][:, None], want["accepted"], want["margin"], got["logw"][:, None], got["accepted"], wild)
    others = [i for i in range(n) if i not in WILD]
    assert torch.isfinite(clean["x"]).all() and torch.isfinite(clean["logw"]).all()
    assert torch.equal(got["x"][others], clean["x"][others]) and torch.equal(got["logw"][others], clean["logw"][others])
    assert torch.equal(got["accepted"][:, others], clean["accepted"][:, others])


@pytest.mark.parametrize("dim", [5, 100])
@pytest.mark.parametrize("kind", KINDS)
def test_langevin_ladder_wild_start_stays_in_its_ladder(cuda_device, kind, dim):
    """test_tempering_gpu.py::test_wild_start_stays_in_its_ladder with the wild starts above: counts and the NaN pattern are
    the restatement's (Rosenbrock: the NaN walks one column along the row per step, through the neighbour exchange), and no other
    ladder notices."""
    shape = next(s for s in tempering_cases.LANDSCAPE_CASES if s[:2] == (kind, dim) and s[3] >= 37)
    _, _, R, n, se, k = shape
    c = tempering_cases.case(*shape)
    x0 = wild_ladders(kind, c["x0"])
    want = tempering_cases.restate(oracle_of(c["spec"]), x0, c["noise"], c["u"], tempering_cases.ETA, tempering_cases.SIGMA, c["temps"],
                                   se, torch.float32)
    assert (want["margin"] > MARGIN_BAR).all(), "a swap decision of the restatement is borderline"
    x, counts, _ = lan_gpu.run_kernel(cuda_device, c["spec"], x0, c["temps"], k, se, noise=c["noise"], u=c["u"])
    assert torch.equal(counts, lan_gpu.want_counts(want["mask"], n, R)), (counts, lan_gpu.want_counts(want["mask"], n, R))
    assert torch.equal(torch.isnan(x), torch.isnan(want["x"])) and torch.isnan(x).any()
    clean, _, _ = lan_gpu.run_kernel(cuda_device, c["spec"], c["x0"], c["temps"], k, se, noise=c["noise"], u=c["u"])
    others = [i for i in range(n) if i not in WILD]
    assert torch.equal(x[others], clean[others]) and torch.isfinite(clean).all()


# ---------------------------------------------------------------------------------
# through the classes
# ---------------------------------------------------------------------------------
def _model(kind, dev):
    return ta.core.RosenbrockModel(a=1.0, b=4.0, device=dev) if kind == "rosenbrock" else ta.core.AckleyModel(device=dev)


@pytest.mark.parametrize("kind", KINDS)
def test_the_classes_take_the_fused_route(cuda_device, kind):
    dev, (n, dim) = cuda_device, (300, 12)
    x0 = start_scale(kind) * torch.randn(n, dim, generator=torch.Generator().manual_seed(2)).to(dev)
    gen = lambda seed: torch.Generator(device=dev).manual_seed(seed)  # noqa: E731
    temps = (1.0, 2.0, 4.0)

    s = ta.ReplicaExchangeLangevin(_model(kind, dev), step_size=0.004, temperatures=temps, swap_every=2, device=dev)
    assert s._route(torch.zeros(n, 3, dim, device=dev))[0] == "fused"
    before = hip_calls("ebm_tempering_chain_f32")
    out = s.sample(x=x0, n_steps=20, return_replicas=True, generator=gen(5))
    assert hip_calls("ebm_tempering_chain_f32") == before + 1
    assert out.shape == (n, 3, dim) and torch.isfinite(out).all() and not torch.equal(out[:, 0], x0)
    assert torch.equal(out, s.sample(x=x0, n_steps=20, return_replicas=True, generator=gen(5)))
    assert not torch.equal(out, s.sample(x=x0, n_steps=20, return_replicas=True, generator=gen(6)))

    eps = tempering_hmc_cases.step_sizes(kind, dim, 1)[0]
    s = ta.ReplicaExchangeHMC(_model(kind, dev), step_size=eps, n_leapfrog_steps=4, temperatures=temps, swap_every=1, device=dev)
    assert s._route(torch.zeros(n, 3, dim, device=dev))[0] == "fused"
    before = hip_calls("ebm_tempering_hmc_chain_f32")
    out, diag = s.sample(x=x0, n_steps=10, return_replicas=True, return_diagnostics=True, generator=gen(5))
    assert hip_calls("ebm_tempering_hmc_chain_f32") == before + 1
    assert out.shape == (n, 3, dim) and torch.isfinite(out).all() and not torch.equal(out[:, 0], x0)
    assert ((diag["acceptance_rate"] > 0.3) & (diag["acceptance_rate"] <= 1.0)).all(), diag["acceptance_rate"]
    assert torch.equal(out, s.sample(x=x0, n_steps=10, return_replicas=True, generator=gen(5)))
    assert not torch.equal(out, s.sample(x=x0, n_steps=10, return_replicas=True, generator=gen(6)))

    s = ta.AnnealedImportanceSampling(_model(kind, dev), n_temperatures=10, schedule="sigmoid", step_size=ais_cases.step_sizes(kind, dim, 1)[0],
                                      n_leapfrog_steps=4, base_std=ais_cases.base_std_of(kind), device=dev)
    assert s._route(dim)[0] == "fused"
    before = hip_calls("ebm_ais_chain_f32")
    r = s.run(n, dim, generator=gen(5))
    assert hip_calls("ebm_ais_chain_f32") == before + 1
    assert r.samples.shape == (n, dim) and torch.isfinite(r.samples).all() and torch.isfinite(r.log_weights).all() and r.n_nonfinite == 0
    again, other = s.run(n, dim, generator=gen(5)), s.run(n, dim, generator=gen(6))
    assert torch.equal(again.samples, r.samples) and torch.equal(again.log_weights, r.log_weights)
    assert not torch.equal(other.log_weights, r.log_weights)
