"""ebm_tempering_chain_f32 on the GPU: the kernel through the C ABI with injected draws against the restatement of
tempering_cases.py (decisions exactly; states bit for bit for the element-wise energies, by the fp64 yardstick for the rest),
its native draws against the materialised Philox field, and ReplicaExchangeLangevin.sample() on top of it."""

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls, yardstick
from tempering_cases import (ETA, EXACT_CASES, MARGIN_BAR, SIGMA, YARDSTICK_CASES, case, energy_spec, ladder, model_of,
                             oracle_of, restate)

pytestmark = pytest.mark.gpu


def run_kernel(dev, spec, x0, temps, k, swap_every, *, noise=None, u=None, seed=0, step0=0, thin=None, eta=ETA, sigma=SIGMA):
    """One call of the entry on the ladders x0 [n, R, dim] -> (states [n, R, dim], counts [2 (R - 1)], traj or None), on the CPU."""
    n, R, dim = x0.shape
    model = model_of(spec, dev)
    coef, beta = (t.to(dev) for t in ladder(sigma, temps))
    x = x0.to(dev).contiguous().clone()
    counts = torch.zeros(2 * (R - 1), dtype=torch.int32, device=dev)
    traj = torch.empty(n, k // thin, dim, device=dev) if thin else None
    noise_d = None if noise is None else noise.to(dev).contiguous()
    u_d = None if u is None else (u.to(dev).contiguous() if u.numel() else torch.zeros(4, device=dev))
    before = hip_calls("ebm_tempering_chain_f32")
    _lib.call("ebm_tempering_chain_f32", model.fused_spec().to_c(), x.data_ptr(), n, R, dim, k, eta, eta**0.5, coef.data_ptr(),
              beta.data_ptr(), swap_every, thin or 1, _lib.ptr(traj), counts.data_ptr(), _lib.ptr(noise_d), _lib.ptr(u_d), seed, step0,
              _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls("ebm_tempering_chain_f32") == before + 1
    return x.cpu(), counts.cpu().long(), (traj.cpu() if thin else None)


def want_counts(mask, n, R):
    """[attempts of each pair | accepts of each pair] from the restatement's decision mask [events, n, R - 1]."""
    tried = torch.zeros(R - 1, dtype=torch.long)
    for m in range(mask.shape[0]):
        tried[m % 2 :: 2] += n
    return torch.cat([tried, mask.sum(dim=(0, 1)).long()])


def slot_of_each_state(got, ref):
    """For every ladder and slot of `got`, the slot of `ref` whose state is nearest: the net relabelling the kernel made."""
    d = (got[:, :, None, :].double() - ref[:, None, :, :].double()).abs().amax(dim=-1)  # [n, R got, R ref]
    return d.argmin(dim=-1)


def check_decisions(c, x, counts):
    n, R, _ = c["shape"]
    assert c["ref64"]["margin"].numel() == 0 or c["ref64"]["margin"].min().item() > MARGIN_BAR, c["seed"]
    assert torch.equal(c["ref32"]["mask"], c["ref64"]["mask"])
    assert torch.equal(counts, want_counts(c["ref32"]["mask"], n, R)), (counts, want_counts(c["ref32"]["mask"], n, R))
    assert torch.equal(slot_of_each_state(x, c["ref32"]["x"]), torch.arange(R).expand(n, R))
    events = c["k"] // c["swap_every"]
    if events >= 2 and n >= 37:  # the case exercises both outcomes
        want = want_counts(c["ref32"]["mask"], n, R)
        assert 0 < want[R - 1 :].sum() < want[: R - 1].sum()


@pytest.mark.parametrize("kind,dim,R,n,swap_every,k", EXACT_CASES)
def test_elementwise_energies_bit_for_bit(cuda_device, kind, dim, R, n, swap_every, k):
    c = case(kind, dim, R, n, swap_every, k)
    x, counts, traj = run_kernel(cuda_device, c["spec"], c["x0"], c["temps"], k, swap_every, noise=c["noise"], u=c["u"], thin=2)
    check_decisions(c, x, counts)
    assert torch.equal(x, c["ref32"]["x"])
    want = restate(oracle_of(c["spec"]), c["x0"], c["noise"], c["u"], ETA, SIGMA, c["temps"], swap_every, torch.float32, thin=2)
    assert torch.equal(traj, want["traj"])


@pytest.mark.parametrize("kind,dim,R,n,swap_every,k", YARDSTICK_CASES)
def test_coupled_energies_against_float64(cuda_device, kind, dim, R, n, swap_every, k):
    c = case(kind, dim, R, n, swap_every, k)
    x, counts, _ = run_kernel(cuda_device, c["spec"], c["x0"], c["temps"], k, swap_every, noise=c["noise"], u=c["u"])
    check_decisions(c, x, counts)
    rows = lambda t: t.reshape(n * R, dim)  # noqa: E731
    print(yardstick(rows(x), rows(c["ref32"]["x"]), rows(c["ref64"]["x"]), k_med=1.5, what=f"{kind} dim {dim} R {R}"))


def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


@pytest.mark.parametrize("kind,dim,R,n,swap_every,k", [("double_well", 5, 3, 37, 2, 8), ("gmm", 32, 4, 70, 1, 5),
                                                       ("gaussian", 260, 2, 9, 3, 7)])
def test_native_draws_are_the_materialised_field(cuda_device, kind, dim, R, n, swap_every, k):
    dev, spec, temps = cuda_device, energy_spec(kind, dim), (1.0, 2.0, 4.0, 8.0)[:R]
    x0 = torch.randn(n, R, dim, generator=torch.Generator().manual_seed(8))
    seed, step0 = 0x1234567887654321, 77
    native, counts_n, traj_n = run_kernel(dev, spec, x0, temps, k, swap_every, seed=seed, step0=step0, thin=1)
    noise = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, step0 + 2 * s, n * R * dim) for s in range(k)]).view(k, n, R, dim).cpu()
    u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, step0 + 2 * s + 1, n * R)
                     for s in range(k) if (s + 1) % swap_every == 0]).view(-1, n, R).cpu()
    fed, counts_f, traj_f = run_kernel(dev, spec, x0, temps, k, swap_every, noise=noise, u=u, thin=1)
    assert torch.equal(native, fed) and torch.equal(counts_n, counts_f) and torch.equal(traj_n, traj_f)
    assert counts_n[R - 1 :].sum() > 0, "no swap was accepted: the uniform field was not exercised"
    # a sub-block of ladders run alone (another grid, other lanes) reproduces its rows of the full launch
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part, _, _ = run_kernel(dev, spec, x0[lo:hi], temps, k, swap_every, noise=noise[:, lo:hi], u=u[:, lo:hi])
    assert torch.equal(part, fed[lo:hi])


def test_no_swaps_are_independent_langevin_chains(cuda_device):
    """swap_every > k: slot r's rows are ebm_langevin_chain_f32 on those rows with noise_coef_r, bit for bit."""
    dev, (n, R, dim, k) = cuda_device, (37, 4, 32, 6)
    c = case("double_well", dim, R, n, 100, k)
    x, counts, _ = run_kernel(dev, c["spec"], c["x0"], c["temps"], k, 100, noise=c["noise"], u=c["u"])
    assert counts.sum() == 0
    coef, _ = ladder(SIGMA, c["temps"])
    spec_c = model_of(c["spec"], dev).fused_spec().to_c()
    for r in range(R):
        rows = c["x0"][:, r].contiguous().to(dev)
        eps = c["noise"][:, :, r].contiguous().to(dev)
        _lib.call("ebm_langevin_chain_f32", spec_c, rows.data_ptr(), n, dim, k, ETA, ETA**0.5, coef[r].item(), None, 0, 0.0, 0.0, 1,
                  None, None, eps.data_ptr(), 0, 0, _lib.stream_handle(dev))
        assert torch.equal(rows.cpu(), x[:, r]), r


def test_wild_start_stays_in_its_ladder(cuda_device):
    """A NaN coordinate in slot 1 of one ladder and a +inf energy in slot 0 of another: decisions and the NaN pattern are the
    restatement's, and no other ladder notices."""
    dev, (n, R, dim, k, se) = cuda_device, (37, 3, 5, 6, 1)
    c = case("double_well", dim, R, n, se, k)
    x0 = c["x0"].clone()
    x0[3, 1, 2] = float("nan")
    x0[7, 0, 4] = 1e20  # x^2 overflows: the energy is +inf
    assert torch.isinf(oracle_of(c["spec"]).energy(x0[7, :1])).all()
    want = restate(oracle_of(c["spec"]), x0, c["noise"], c["u"], ETA, SIGMA, c["temps"], se, torch.float32)
    x, counts, _ = run_kernel(dev, c["spec"], x0, c["temps"], k, se, noise=c["noise"], u=c["u"])
    assert torch.equal(counts, want_counts(want["mask"], n, R))
    assert torch.equal(torch.isnan(x), torch.isnan(want["x"])) and torch.isnan(x).any()
    assert torch.allclose(x, want["x"], rtol=0, atol=0, equal_nan=True)
    clean, _, _ = run_kernel(dev, c["spec"], c["x0"], c["temps"], k, se, noise=c["noise"], u=c["u"])
    others = [i for i in range(n) if i not in (3, 7)]
    assert torch.equal(x[others], clean[others]) and torch.isfinite(clean).all()


# ---------------------------------------------------------------------------------
# through sample()
# ---------------------------------------------------------------------------------
def test_sample_is_one_launch_with_the_documented_shapes(cuda_device):
    dev, (n, dim, k) = cuda_device, (300, 6, 40)
    s = ta.ReplicaExchangeLangevin(ta.DoubleWellModel(device=dev), step_size=0.01, swap_every=5, device=dev)
    x0 = torch.randn(n, dim, device=dev)
    g = torch.Generator(device=dev).manual_seed(5)
    before = hip_calls("ebm_tempering_chain_f32")
    traj, diag = s.sample(x=x0, n_steps=k, thin=4, return_trajectory=True, return_diagnostics=True, generator=g)
    assert hip_calls("ebm_tempering_chain_f32") == before + 1
    assert _rng._get_offset(g) == 4 * 2 * k
    assert traj.shape == (n, 10, dim) and diag["mean"].shape == diag["var"].shape == (10, dim)
    assert diag["energy"].shape == (10,) and diag["swap_acceptance"].shape == (3,)
    assert torch.allclose(diag["mean"], traj.mean(dim=0), atol=1e-5)
    assert torch.allclose(diag["var"], traj.var(dim=0, unbiased=False), rtol=1e-4, atol=1e-6)
    e = ta.DoubleWellModel(device=dev)(traj.transpose(0, 1).reshape(-1, dim)).view(10, n).mean(dim=1)
    assert torch.allclose(diag["energy"], e, rtol=1e-5)
    # the same generator state: the trajectory's last kept state is the final state, which is slot 0 of the ladders
    final = s.sample(x=x0, n_steps=k, generator=torch.Generator(device=dev).manual_seed(5))
    ladders = s.sample(x=x0, n_steps=k, return_replicas=True, generator=torch.Generator(device=dev).manual_seed(5))
    assert hip_calls("ebm_tempering_chain_f32") == before + 3
    assert final.shape == (n, dim) and ladders.shape == (n, 4, dim)
    assert torch.equal(traj[:, -1], final) and torch.equal(ladders[:, 0], final)
    assert not torch.equal(x0, final) and torch.isfinite(ladders).all()
    # continuing a ladder: two calls of k == one call of 2 k (k an even multiple of swap_every)
    g2 = torch.Generator(device=dev).manual_seed(5)
    half = s.sample(x=x0, n_steps=k, return_replicas=True, generator=g2)
    both = s.sample(x=half, n_steps=k, return_replicas=True, generator=g2)
    whole = s.sample(x=x0, n_steps=2 * k, return_replicas=True, generator=torch.Generator(device=dev).manual_seed(5))
    assert torch.equal(both, whole)


def test_it_mixes_where_langevin_does_not(cuda_device):
    """DoubleWell(h = 10), dim 2, 4096 chains that start in the left well, 2000 steps at eta = 0.004.  The CPU restatement ends
    with 0.497 / 0.507 of slot 0 at x_0 > 0 (binomial sigma 0.008) and swap rates 0.60 - 0.67; plain Langevin with 0.003 - 0.008."""
    dev, n = cuda_device, 4096
    model = ta.DoubleWellModel(barrier_height=10.0, device=dev)
    x0 = torch.full((n, 2), -1.0, device=dev)
    s = ta.ReplicaExchangeLangevin(model, step_size=0.004, temperatures=(1.0, 2.0, 4.0, 8.0), swap_every=5, device=dev)
    ladders, diag = s.sample(x=x0, n_steps=2000, thin=2000, return_replicas=True, return_diagnostics=True,
                             generator=torch.Generator(device=dev).manual_seed(0))
    frac = (ladders[:, 0, 0] > 0).float().mean().item()
    print("tempered fraction right", frac, "swap acceptance", diag["swap_acceptance"].tolist())
    assert torch.isfinite(ladders).all()
    assert 0.45 <= frac <= 0.55
    assert ((diag["swap_acceptance"] >= 0.4) & (diag["swap_acceptance"] <= 0.8)).all()
    plain = ta.LangevinDynamics(model, step_size=0.004, device=dev).sample(x=x0, n_steps=2000, generator=torch.Generator(device=dev).manual_seed(0))
    frac_plain = (plain[:, 0] > 0).float().mean().item()
    print("plain Langevin fraction right", frac_plain)
    assert frac_plain < 0.03


def test_each_slot_keeps_its_own_law(cuda_device):
    """Harmonic(k = 1): the Euler-Maruyama chain at temperature T has stationary variance T / (1 - eta / 2) per coordinate.
    8192 ladders x 8 coordinates: the estimator's sigma is 0.55 %; the CPU restatement gives ratios 1.005 / 0.998 / 0.999."""
    dev, n, dim, temps, eta = cuda_device, 8192, 8, (1.0, 2.0, 4.0), 0.01
    s = ta.ReplicaExchangeLangevin(ta.HarmonicModel(k=1.0, device=dev), step_size=eta, temperatures=temps, swap_every=5, device=dev)
    ladders = s.sample(x=torch.zeros(n, dim, device=dev), n_steps=1500, return_replicas=True,
                       generator=torch.Generator(device=dev).manual_seed(0))
    for r, t in enumerate(temps):
        ratio = ladders[:, r].var(unbiased=False).item() / (t / (1.0 - eta / 2.0))
        print("slot", r, "variance ratio", ratio)
        assert abs(ratio - 1.0) <= 0.03, (r, ratio)


def test_other_configurations_take_the_eager_route_on_the_gpu(cuda_device):
    dev = cuda_device
    sched = ta.core.schedules.ExponentialDecayScheduler(0.01, 0.99)
    s = ta.ReplicaExchangeLangevin(ta.DoubleWellModel(device=dev), step_size=sched, temperatures=(1.0, 2.0), swap_every=2, device=dev)
    before = hip_calls("ebm_tempering_chain_f32")
    out = s.sample(dim=4, n_samples=64, n_steps=6, generator=torch.Generator(device=dev).manual_seed(1))
    assert hip_calls("ebm_tempering_chain_f32") == before and out.shape == (64, 4) and out.is_cuda and torch.isfinite(out).all()
    wide = ta.ReplicaExchangeLangevin(ta.DoubleWellModel(device=dev), temperatures=(1.0, 2.0, 3.0, 4.0, 5.0), device=dev)
    assert wide._route(torch.zeros(2, 5, 256, device=dev))[0] == "eager" and wide._route(torch.zeros(2, 5, 32, device=dev))[0] == "fused"
