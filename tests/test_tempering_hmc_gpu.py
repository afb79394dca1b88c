"""ebm_tempering_hmc_chain_f32 on the GPU: the kernel through the C ABI with injected draws against the restatement of
tempering_hmc_cases.py (decisions exactly, states by the fp64 yardstick), its native draws against the materialised Philox
field, its transition against ebm_hmc_chain_f32, and ReplicaExchangeHMC.sample() on top of it."""

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls, yardstick
import tempering_cases
from tempering_hmc_cases import (CASES, FROZEN_EVENTS, MARGIN_BAR, case, closest_call, energy_spec, frozen_case, ladder,
                                 leapfrog_steps, model_of, oracle_of, restate, slot_permutation, step_sizes)

pytestmark = pytest.mark.gpu
ENTRY = "ebm_tempering_hmc_chain_f32"


def run_kernel(dev, spec, x0, temps, eps, L, n_mh, swap_every, *, z=None, ua=None, us=None, seed=0, step0=0, thin=None,
               coefficients=None):
    """One call of the entry on the ladders x0 [n, R, dim] -> dict of CPU tensors: states [n, R, dim], the accept mask
    [n_mh, n, R], accept counts [R], swap counts [2 (R - 1)], traj or None."""
    n, R, dim = x0.shape
    model = model_of(spec, dev)
    sqrt_temp, beta = (t.to(dev) for t in (coefficients or ladder(temps)))
    eps_d = torch.tensor(list(eps), dtype=torch.float32, device=dev)
    x = x0.to(dev).contiguous().clone()
    mask = torch.full((n_mh, n * R), 7, dtype=torch.uint8, device=dev)
    accepts = torch.zeros(R, dtype=torch.int32, device=dev)
    swaps = torch.zeros(2 * (R - 1), dtype=torch.int32, device=dev)
    traj = torch.empty(n, n_mh // thin, dim, device=dev) if thin else None
    z_d = None if z is None else z.to(dev).contiguous()
    ua_d = None if ua is None else ua.to(dev).contiguous()
    us_d = None if us is None else (us.to(dev).contiguous() if us.numel() else torch.zeros(4, device=dev))
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, model.fused_spec().to_c(), x.data_ptr(), n, R, dim, n_mh, L, eps_d.data_ptr(), sqrt_temp.data_ptr(),
              beta.data_ptr(), swap_every, thin or 1, _lib.ptr(traj), mask.data_ptr(), accepts.data_ptr(), swaps.data_ptr(),
              _lib.ptr(z_d), _lib.ptr(ua_d), _lib.ptr(us_d), seed, step0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    mask = mask.cpu()
    assert int(mask.max()) <= 1, "a slot row of the accept mask was not written"
    return {"x": x.cpu(), "accepted": mask.bool().view(n_mh, n, R), "accepts": accepts.cpu().long(), "swaps": swaps.cpu().long(),
            "traj": traj.cpu() if thin else None}


def want_swap_counts(mask, n, R):
    """[attempts of each pair | accepts of each pair] from the restatement's swap mask [events, n, R - 1]."""
    tried = torch.zeros(R - 1, dtype=torch.long)
    for m in range(mask.shape[0]):
        tried[m % 2 :: 2] += n
    return torch.cat([tried, mask.sum(dim=(0, 1)).long()])


def slot_of_each_state(got, ref):
    """For every ladder and slot of `got`, the slot of `ref` whose state is nearest: the net relabelling the kernel made."""
    d = (got[:, :, None, :].double() - ref[:, None, :, :].double()).abs().amax(dim=-1)  # [n, R got, R ref]
    return d.argmin(dim=-1)


def check_decisions(got, want, n, R):
    assert torch.equal(got["accepted"], want["accepted"])
    assert torch.equal(got["accepts"], want["accepted"].sum(dim=(0, 1)).long())
    assert torch.equal(got["swaps"], want_swap_counts(want["mask"], n, R)), (got["swaps"], want_swap_counts(want["mask"], n, R))


@pytest.mark.parametrize("kind,dim,R,n,swap_every,n_mh", CASES)
def test_cases_with_injected_draws(cuda_device, kind, dim, R, n, swap_every, n_mh):
    c = case(kind, dim, R, n, swap_every, n_mh)
    ref32, ref64 = c["ref32"], c["ref64"]
    assert closest_call(ref64) > MARGIN_BAR, c["seed"]
    assert torch.equal(ref32["accepted"], ref64["accepted"]) and torch.equal(ref32["mask"], ref64["mask"])
    if n >= 37:  # the case exercises both outcomes of both decisions
        assert 0 < ref32["accepted"].sum() < ref32["accepted"].numel()
        assert 0 < ref32["mask"].sum() < want_swap_counts(ref32["mask"], n, R)[: R - 1].sum()
    got = run_kernel(cuda_device, c["spec"], c["x0"], c["temps"], c["eps"], c["L"], n_mh, swap_every, z=c["z"], ua=c["u_accept"],
                     us=c["u_swap"], thin=2)
    check_decisions(got, ref32, n, R)
    assert torch.equal(slot_of_each_state(got["x"], ref32["x"]), torch.arange(R).expand(n, R))
    rows = lambda t: t.reshape(-1, dim)  # noqa: E731
    print(yardstick(rows(got["x"]), rows(ref32["x"]), rows(ref64["x"]), k_med=2.0, what=f"{kind} dim {dim} R {R} states"))
    print(yardstick(rows(got["traj"]), rows(ref32["traj"]), rows(ref64["traj"]), k_med=2.0, what=f"{kind} dim {dim} R {R} slot 0 kept"))


def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


# (kind, dim, R, n, temps, swap_every, n_mh, step-size factor): on the CPU restatement these reject 10 - 30 proposals and
# accept 13 - 90 swaps each (the Gaussian at dim 256 needs a close pair of temperatures to swap at all)
@pytest.mark.parametrize("kind,dim,R,n,temps,swap_every,n_mh,factor", [
    ("double_well", 5, 3, 37, (1.0, 2.0, 4.0), 2, 6, 1.0),
    ("gmm", 32, 4, 70, (1.0, 2.0, 4.0, 8.0), 1, 5, 1.0),
    ("gaussian", 256, 2, 9, (1.0, 1.05), 2, 7, 4.0),
])
def test_native_draws_are_the_materialised_fields(cuda_device, kind, dim, R, n, temps, swap_every, n_mh, factor):
    dev, spec, L = cuda_device, energy_spec(kind, dim), leapfrog_steps(dim)
    eps = tuple(factor * v for v in step_sizes(kind, dim, R))
    x0 = torch.randn(n, R, dim, generator=torch.Generator().manual_seed(8))
    seed, step0 = 0x1234567887654321, 77
    native = run_kernel(dev, spec, x0, temps, eps, L, n_mh, swap_every, seed=seed, step0=step0, thin=1)
    z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, step0 + 3 * t, n * R * dim) for t in range(n_mh)]).view(n_mh, n, R, dim).cpu()
    ua = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, step0 + 3 * t + 1, n * R) for t in range(n_mh)]).view(n_mh, n, R).cpu()
    us = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, step0 + 3 * t + 2, n * R)
                      for t in range(n_mh) if (t + 1) % swap_every == 0]).view(-1, n, R).cpu()
    fed = run_kernel(dev, spec, x0, temps, eps, L, n_mh, swap_every, z=z, ua=ua, us=us, thin=1)
    for key in ("x", "accepted", "accepts", "swaps", "traj"):
        assert torch.equal(native[key], fed[key]), key
    assert native["swaps"][R - 1 :].sum() > 0, "no swap was accepted: the swap uniforms were not exercised"
    assert (~native["accepted"]).any(), "no proposal was rejected: the accept uniforms were not exercised"
    # a sub-block of ladders run alone (another grid, other lanes) reproduces its rows of the full launch
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part = run_kernel(dev, spec, x0[lo:hi], temps, eps, L, n_mh, swap_every, z=z[:, lo:hi], ua=ua[:, lo:hi], us=us[:, lo:hi])
    assert torch.equal(part["x"], fed["x"][lo:hi]) and torch.equal(part["accepted"], fed["accepted"][:, lo:hi])


@pytest.mark.parametrize("dim", [5, 100])
def test_the_transition_is_the_hmc_kernels(cuda_device, dim):
    """sqrt_temp = beta = 1 in every slot and no event: the rows are ebm_hmc_chain_f32 chains, bit for bit (double well at
    dims where that entry runs the lane-group kernel of the same geometry)."""
    dev, (n, R, n_mh, L, eps) = cuda_device, (37, 3, 5, 4, 0.15)
    spec = energy_spec("double_well", dim)
    g = torch.Generator().manual_seed(21)
    x0 = torch.randn(n, R, dim, generator=g)
    z, ua = torch.randn(n_mh, n, R, dim, generator=g), torch.rand(n_mh, n, R, generator=g)
    ones = (torch.ones(R), torch.ones(R))
    got = run_kernel(dev, spec, x0, None, (eps,) * R, L, n_mh, n_mh + 1, z=z, ua=ua, us=torch.zeros(0, n, R), coefficients=ones)
    assert got["swaps"].sum() == 0
    rows, p_d, u_d = x0.view(n * R, dim).to(dev).clone(), z.view(n_mh, n * R, dim).to(dev), ua.view(n_mh, n * R).to(dev)
    mask = torch.empty(n_mh, n * R, dtype=torch.uint8, device=dev)
    _lib.call("ebm_hmc_chain_f32", model_of(spec, dev).fused_spec().to_c(), rows.data_ptr(), n * R, dim, n_mh, L, eps, None, 0, 0.0,
              None, 1, None, None, mask.data_ptr(), None, p_d.data_ptr(), u_d.data_ptr(), 0, 0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert torch.equal(mask.cpu().bool().view(n_mh, n, R), got["accepted"])
    assert (~got["accepted"]).any() and got["accepted"].any()
    assert torch.equal(rows.cpu().view(n, R, dim), got["x"])


# unaligned rows and idle lane groups; a G = 32 that is not full; a ladder spread over several waves
@pytest.mark.parametrize("kind,dim,R,n", [("double_well", 5, 3, 37), ("gmm", 100, 3, 37), ("double_well", 256, 4, 37)])
def test_both_ladders_take_the_same_swap_decisions(cuda_device, kind, dim, R, n):
    """States that cannot move, the same temperatures and the same swap uniforms through ebm_tempering_chain_f32 (eta = 0,
    zero noise) and this entry (eps = 0 in every slot): the same final slot matrix and the same swap counts, bit for bit --
    both kernels run the one swap event of csrc/ladder.h on energies their evaluations give alike (double well, mixture)."""
    dev, c, k = cuda_device, frozen_case(kind, dim, R, n), FROZEN_EVENTS
    x0, u = c["x0"], c["u"]
    coef, beta = (t.to(dev) for t in tempering_cases.ladder(tempering_cases.SIGMA, c["temps"]))
    assert torch.equal(beta.cpu(), ladder(c["temps"])[1])
    x, counts = x0.to(dev).contiguous().clone(), torch.zeros(2 * (R - 1), dtype=torch.int32, device=dev)
    noise_d, u_d = torch.zeros(k, n, R, dim, device=dev), u.to(dev).contiguous()
    _lib.call("ebm_tempering_chain_f32", model_of(c["spec"], dev).fused_spec().to_c(), x.data_ptr(), n, R, dim, k, 0.0, 0.0,
              coef.data_ptr(), beta.data_ptr(), 1, 1, None, counts.data_ptr(), noise_d.data_ptr(), u_d.data_ptr(), 0, 0,
              _lib.stream_handle(dev))
    torch.cuda.synchronize()
    got = run_kernel(dev, c["spec"], x0, c["temps"], (0.0,) * R, c["L"], k, 1, z=c["z"], ua=c["u_accept"], us=u)
    assert got["accepted"].all(), "dH = 0 exactly: every proposal is taken"
    assert torch.equal(got["x"], x.cpu())
    assert torch.equal(got["swaps"], counts.cpu().long())
    assert 0 < int(got["swaps"][R - 1 :].sum()) < int(got["swaps"][: R - 1].sum()) == c["attempts"]
    assert (slot_permutation(got["x"], x0) != torch.arange(R)).any()


def test_wild_start_stays_in_its_ladder(cuda_device):
    """A NaN coordinate in slot 1 of one ladder and a 1e20 coordinate (a +inf energy) in slot 0 of another: masks, counters
    and the NaN pattern are the restatement's, and no other ladder notices."""
    dev, (kind, dim, R, n, se, n_mh) = cuda_device, ("double_well", 5, 3, 37, 2, 6)
    c = case(kind, dim, R, n, se, n_mh)
    x0 = c["x0"].clone()
    x0[3, 1, 2] = float("nan")
    x0[7, 0, 4] = 1e20  # x^2 overflows: the energy is +inf
    assert torch.isinf(oracle_of(c["spec"]).energy(x0[7, :1])).all()
    want = restate(oracle_of(c["spec"]), x0, c["z"], c["u_accept"], c["u_swap"], c["eps"], c["L"], c["temps"], se, torch.float32)
    args = (dev, c["spec"])
    kw = dict(z=c["z"], ua=c["u_accept"], us=c["u_swap"])
    got = run_kernel(*args, x0, c["temps"], c["eps"], c["L"], n_mh, se, **kw)
    check_decisions(got, want, n, R)
    assert torch.equal(torch.isnan(got["x"]), torch.isnan(want["x"])) and torch.isnan(got["x"]).any()
    clean = run_kernel(*args, c["x0"], c["temps"], c["eps"], c["L"], n_mh, se, **kw)
    others = [i for i in range(n) if i not in (3, 7)]
    assert torch.equal(got["x"][others], clean["x"][others]) and torch.isfinite(clean["x"]).all()
    assert torch.equal(got["accepted"][:, others], clean["accepted"][:, others])


# ---------------------------------------------------------------------------------
# through sample()
# ---------------------------------------------------------------------------------
def test_sample_is_one_launch_with_the_documented_shapes(cuda_device):
    dev, (n, dim, k) = cuda_device, (300, 6, 40)
    s = ta.ReplicaExchangeHMC(ta.DoubleWellModel(device=dev), step_size=(0.2, 0.18, 0.15, 0.12), n_leapfrog_steps=4, swap_every=2,
                              device=dev)
    x0 = torch.randn(n, dim, device=dev)
    g = torch.Generator(device=dev).manual_seed(5)
    before = hip_calls(ENTRY)
    traj, diag = s.sample(x=x0, n_steps=k, thin=4, return_trajectory=True, return_diagnostics=True, generator=g)
    assert hip_calls(ENTRY) == before + 1
    want_g = torch.Generator(device=dev).manual_seed(5)
    _rng.reserve(want_g, dev, 3 * k)
    assert _rng._get_offset(g) == _rng._get_offset(want_g) == 4 * 3 * k
    assert traj.shape == (n, 10, dim) and diag["mean"].shape == diag["var"].shape == (10, dim)
    assert diag["energy"].shape == (10,) and diag["swap_acceptance"].shape == (3,) and diag["acceptance_rate"].shape == (4,)
    assert ((diag["acceptance_rate"] > 0.5) & (diag["acceptance_rate"] < 1.0)).all(), diag["acceptance_rate"]
    assert ((diag["swap_acceptance"] > 0.0) & (diag["swap_acceptance"] < 1.0)).all(), diag["swap_acceptance"]
    assert torch.allclose(diag["mean"], traj.mean(dim=0), atol=1e-5)
    assert torch.allclose(diag["var"], traj.var(dim=0, unbiased=False), rtol=1e-4, atol=1e-6)
    e = ta.DoubleWellModel(device=dev)(traj.transpose(0, 1).reshape(-1, dim)).view(10, n).mean(dim=1)
    assert torch.allclose(diag["energy"], e, rtol=1e-5)
    # the same generator state: the trajectory's last kept state is the final state, which is slot 0 of the ladders
    final = s.sample(x=x0, n_steps=k, generator=torch.Generator(device=dev).manual_seed(5))
    ladders = s.sample(x=x0, n_steps=k, return_replicas=True, generator=torch.Generator(device=dev).manual_seed(5))
    assert hip_calls(ENTRY) == before + 3
    assert final.shape == (n, dim) and ladders.shape == (n, 4, dim)
    assert torch.equal(traj[:, -1], final) and torch.equal(ladders[:, 0], final)
    assert not torch.equal(x0, final) and torch.isfinite(ladders).all()
    # continuing a ladder: two calls of k == one call of 2 k (k an even multiple of swap_every)
    g2 = torch.Generator(device=dev).manual_seed(5)
    half = s.sample(x=x0, n_steps=k, return_replicas=True, generator=g2)
    both = s.sample(x=half, n_steps=k, return_replicas=True, generator=g2)
    whole = s.sample(x=x0, n_steps=2 * k, return_replicas=True, generator=torch.Generator(device=dev).manual_seed(5))
    assert torch.equal(both, whole)


def test_other_configurations_take_the_eager_route_on_the_gpu(cuda_device):
    dev = cuda_device
    model = ta.DoubleWellModel(device=dev)
    sched = ta.core.schedules.ExponentialDecayScheduler(0.1, 0.99)
    before = hip_calls(ENTRY)
    for sampler, dim in [
        (ta.ReplicaExchangeHMC(model, step_size=sched, n_leapfrog_steps=3, temperatures=(1.0, 2.0), swap_every=2, device=dev), 4),
        (ta.ReplicaExchangeHMC(model, step_size=0.02, n_leapfrog_steps=3, temperatures=(1.0, 2.0), device=dev), 300),
        (ta.ReplicaExchangeHMC(model, step_size=0.02, n_leapfrog_steps=3, temperatures=(1.0, 2.0, 3.0, 4.0, 5.0), device=dev), 256),
    ]:
        R = sampler.n_replicas
        assert sampler._route(torch.zeros(2, R, dim, device=dev))[0] == "eager"
        out, diag = sampler.sample(dim=dim, n_samples=16, n_steps=4, return_diagnostics=True, generator=torch.Generator(device=dev).manual_seed(1))
        assert out.shape == (16, dim) and out.is_cuda and torch.isfinite(out).all()
        assert diag["acceptance_rate"].shape == (R,) and diag["acceptance_rate"].is_cuda
    assert hip_calls(ENTRY) == before
    wide = ta.ReplicaExchangeHMC(model, temperatures=(1.0, 2.0, 3.0, 4.0, 5.0), device=dev)
    assert wide._route(torch.zeros(2, 5, 32, device=dev))[0] == "fused"


def test_it_mixes_exactly_where_hmc_does_not(cuda_device):
    """DoubleWell(h = 10), dim 2, 4096 chains that start in the left well, eps = 0.05, L = 5, 400 transitions.  The CPU
    restatement ends with 0.510 of slot 0 at x_0 > 0 (binomial sigma 0.008), swap rates 0.60 - 0.72 and a per-slot MH
    acceptance of 0.98; plain HMC with 0.004."""
    dev, n = cuda_device, 4096
    model = ta.DoubleWellModel(barrier_height=10.0, device=dev)
    x0 = torch.full((n, 2), -1.0, device=dev)
    s = ta.ReplicaExchangeHMC(model, step_size=0.05, n_leapfrog_steps=5, temperatures=(1.0, 2.0, 4.0, 8.0), swap_every=1, device=dev)
    ladders, diag = s.sample(x=x0, n_steps=400, thin=400, return_replicas=True, return_diagnostics=True,
                             generator=torch.Generator(device=dev).manual_seed(0))
    frac = (ladders[:, 0, 0] > 0).float().mean().item()
    print("tempered fraction right", frac, "swap acceptance", diag["swap_acceptance"].tolist(), "MH acceptance", diag["acceptance_rate"].tolist())
    assert torch.isfinite(ladders).all()
    assert 0.45 <= frac <= 0.55
    assert ((diag["swap_acceptance"] >= 0.4) & (diag["swap_acceptance"] <= 0.85)).all()
    plain = ta.HamiltonianMonteCarlo(model, step_size=0.05, n_leapfrog_steps=5, device=dev).sample(
        x=x0, n_steps=400, generator=torch.Generator(device=dev).manual_seed(0))
    frac_plain = (plain[:, 0] > 0).float().mean().item()
    print("plain HMC fraction right", frac_plain)
    assert frac_plain < 0.03


def test_each_slot_keeps_its_own_law_without_bias(cuda_device):
    """Harmonic(k = 1): the slot at temperature T has variance T per coordinate, exactly -- no 1 / (1 - eta / 2) factor as
    the Euler-Maruyama slots of the Langevin ladder carry.  8192 ladders x 8 coordinates: the estimator's sigma is 0.55 %;
    the CPU restatement gives ratios 1.003 / 0.997 / 0.992."""
    dev, n, dim, temps = cuda_device, 8192, 8, (1.0, 2.0, 4.0)
    s = ta.ReplicaExchangeHMC(ta.HarmonicModel(k=1.0, device=dev), step_size=0.3, n_leapfrog_steps=5, temperatures=temps, swap_every=5,
                              device=dev)
    ladders, diag = s.sample(x=torch.zeros(n, dim, device=dev), n_steps=300, thin=300, return_replicas=True, return_diagnostics=True,
                             generator=torch.Generator(device=dev).manual_seed(0))
    print("MH acceptance", diag["acceptance_rate"].tolist())
    for r, t in enumerate(temps):
        ratio = ladders[:, r].var(unbiased=False).item() / t
        print("slot", r, "variance ratio", ratio)
        assert abs(ratio - 1.0) <= 0.03, (r, ratio)
