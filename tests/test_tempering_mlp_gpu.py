"""ebm_tempering_mlp_chain_f32 on the GPU: the kernel through the C ABI with injected draws against the restatements of
tempering_mlp_cases.py (the fp64 referee: the counters equal, the states within the fp32 restatement's own error), what it writes
and what it does not, its native draws against the materialised Philox fields, a run cut in two, a kept last step with no event
behind it, its step against ebm_chain_moments_mlp_f32, frozen states, a wild start, the refusals with real buffers,
ReplicaExchangeLangevin.sample() with the ``fused_mlp_ladder`` opt-in, and the law of a confining 2-D network against the CPU
eager route."""

import copy
import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls
from moments_cases import recip_table
from tempering_mlp_cases import (CASES, ETA, FROZEN_EVENTS, SIGMA, case, frozen_case, ladder, net, slot_permutation, tail_case,
                                 temperatures, want_swap_counts)

pytestmark = pytest.mark.gpu
ENTRY = "ebm_tempering_mlp_chain_f32"
ANALYTIC = "ebm_tempering_chain_f32"
MOMENTS = "ebm_chain_moments_mlp_f32"
FILL = 7.0
GUARD = 64  # elements behind every output that must keep their fill


def _guarded(dev, shape, src=None, dtype=torch.float32, fill=FILL):
    """A tensor of `shape` in front of GUARD elements of `fill` (in one allocation) -> (tensor, guard)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + GUARD,), fill, device=dev, dtype=dtype)
    t = buf[:numel].view(shape)
    if src is not None:
        t.copy_(src)
    return t, buf[numel:]


def run_entry(dev, cpu_model, x0, temps, k, swap_every, *, eta=ETA, sqrt_eta=None, sigma=SIGMA, z=None, u=None, seed=0, step0=0,
              thin=None, counters=True):
    """One call of the entry on the ladders x0 [n, R, dim] -> dict of CPU tensors: x [n, R, dim], swaps [2 (R - 1)],
    traj [n, k // thin, dim] (thin None: no trajectory).  Outputs start from their fill and sit in front of a guard: a slot the
    call did not write keeps it, and so must the guards."""
    n, R, dim = x0.shape
    spec = copy.deepcopy(cpu_model).to(dev).fused_spec()
    assert spec is not None
    coef, beta = (t.to(dev) for t in ladder(sigma, temps))
    x, gx = _guarded(dev, (n * R, dim), x0.reshape(n * R, dim))
    tr, gt = _guarded(dev, (n, k // thin, dim)) if thin else (None, None)
    swaps = torch.zeros(2 * (R - 1), dtype=torch.int32, device=dev) if counters else None
    z_d = None if z is None else z.to(dev).contiguous()
    u_d = None if u is None else (u.to(dev).contiguous() if u.numel() else torch.zeros(4, device=dev))
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, spec.to_c(), x.data_ptr(), n, R, dim, k, eta, eta**0.5 if sqrt_eta is None else sqrt_eta, coef.data_ptr(),
              beta.data_ptr(), swap_every, thin or 1, _lib.ptr(tr), _lib.ptr(swaps), _lib.ptr(z_d), _lib.ptr(u_d), seed, step0,
              _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    for guard in (gx, gt):
        assert guard is None or bool((guard == FILL).all()), "the call wrote behind an output"
    return {"x": x.cpu().view(n, R, dim).clone(), "traj": None if tr is None else tr.cpu().clone(),
            "swaps": None if swaps is None else swaps.cpu().long()}


def _run_case(dev, c, **kw):
    kw.setdefault("thin", c.get("thin"))
    return run_entry(dev, c["cpu"], c["x0"], c["temps"], c["k"], c["swap_every"], eta=c["eta"], sigma=c["sigma"], z=c["z"], u=c["u"], **kw)


def _check_against_fp64(got, ref32, ref64, what):
    """The sibling's bar: no further from fp64 than max(4 x the fp32 restatement's own max error, 4e-6 x max |ref|)."""
    figures = {}
    for key in ("x", "traj"):
        ref = ref64[key]
        err_hip = (got[key].double() - ref).abs().max().item()
        err_torch = (ref32[key].double() - ref).abs().max().item()
        figures[key] = (err_hip, err_torch, ref.abs().max().item())
        print(f"{what}: {key} kernel err {err_hip:.3e}, fp32 restatement err {err_torch:.3e} "
              f"({err_hip / max(err_torch, 1e-30):.2f} x), max|ref| {figures[key][2]:.3e}")
    for key, (err_hip, err_torch, scale) in figures.items():
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
        assert err_hip <= max(4.0 * err_torch, 4e-6 * scale), (key, err_hip, err_torch, scale)


# ---------------------------------------------------------------------------------
# the steps and the events against the restatements
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,R,n,swap_every,k", CASES)
def test_cases_with_injected_draws(cuda_device, in_dim, hidden, R, n, swap_every, k):
    """The counters are the fp64 restatement's (no decision of a case is closer than MARGIN_BAR to its threshold); the final slot
    matrix and the kept slot-0 states are no further from fp64 than max(4 x the fp32 restatement's own max error,
    4e-6 x max |ref|), the bar test_tempering_hmc_mlp_gpu.py gives the same evaluation; every row written, nothing behind them.

    Measured on an MI355X (kernel error / fp32 restatement error per case): see docs/design/tempering_mlp.md."""
    c = case(in_dim, hidden, R, n, swap_every, k)
    got = _run_case(cuda_device, c)  # (run_entry checks the guards behind x and traj)
    ref32, ref64 = c["ref32"], c["ref64"]
    assert got["traj"].shape == (n, k // c["thin"], in_dim)
    want = want_swap_counts(ref64["mask"], n, R)
    print(f"dim {in_dim} H {hidden} R {R} n {n} swap_every {swap_every} k {k}: swap counters {got['swaps'].tolist()}, fp64 {want.tolist()}")
    assert torch.equal(got["swaps"], want), (got["swaps"], want)
    _check_against_fp64(got, ref32, ref64, f"dim {in_dim} H {hidden} R {R} n {n} swap_every {swap_every} k {k}")


@pytest.mark.parametrize("in_dim,hidden,R,n,swap_every,k", [(5, 128, 2, 19, 2, 6), (100, 64, 4, 10, 1, 4)])
def test_a_call_without_trajectory_and_counters(cuda_device, in_dim, hidden, R, n, swap_every, k):
    c = case(in_dim, hidden, R, n, swap_every, k)
    got = _run_case(cuda_device, c)
    lean = _run_case(cuda_device, c, thin=None, counters=False)
    assert lean["traj"] is None and lean["swaps"] is None and torch.equal(lean["x"], got["x"])
    only_counters = _run_case(cuda_device, c, thin=None)
    assert torch.equal(only_counters["swaps"], got["swaps"]) and torch.equal(only_counters["x"], got["x"])
    only_traj = _run_case(cuda_device, c, counters=False)
    assert torch.equal(only_traj["traj"], got["traj"]) and torch.equal(only_traj["x"], got["x"])


@pytest.mark.parametrize("in_dim,hidden,R,n", [(5, 64, 4, 10), (64, 128, 8, 5)])
def test_a_kept_last_step_with_no_event_behind_it(cuda_device, in_dim, hidden, R, n):
    """k = 4, thin = 2, swap_every = 3: the one event follows step 2, the last step is kept and no event is due behind it -- the
    kernel evaluates nothing there (4 evaluations) and stores slot 0's state as it stands.  The counters are the fp64
    restatement's, the kept states and the slot matrix are within its bar, the last kept state is slot 0's final row bit for bit,
    and x does not depend on whether a trajectory is asked for."""
    c = tail_case(in_dim, hidden, R, n)
    assert c["found"] and (c["k"], c["thin"], c["swap_every"]) == (4, 2, 3)
    got = _run_case(cuda_device, c)
    assert got["traj"].shape == (n, 2, in_dim) and torch.equal(got["traj"][:, -1], got["x"][:, 0])
    assert torch.equal(got["swaps"], want_swap_counts(c["ref64"]["mask"], n, R))
    _check_against_fp64(got, c["ref32"], c["ref64"], f"kept last step, dim {in_dim} H {hidden} R {R}")
    bare = _run_case(cuda_device, c, thin=None)
    assert torch.equal(bare["x"], got["x"]) and torch.equal(bare["swaps"], got["swaps"])


# ---------------------------------------------------------------------------------
# native draws
# ---------------------------------------------------------------------------------
def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


def _fields(dev, seed, step0, n, R, dim, k, swap_every):
    """z and u of a call at (seed, step0): normals at step0 + 2 s, uniforms for the events at step0 + 2 s + 1."""
    z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, step0 + 2 * s, n * R * dim) for s in range(k)]).view(k, n, R, dim).cpu()
    u = [_field(dev, _lib.NOISE_UNIFORM, seed, step0 + 2 * s + 1, n * R) for s in range(k) if (s + 1) % swap_every == 0]
    u = torch.stack(u).view(-1, n, R).cpu() if u else torch.zeros(0, n, R)
    return z, u


@pytest.mark.parametrize("in_dim,hidden,R,n,swap_every", [(5, 64, 4, 10, 2), (33, 128, 2, 19, 1), (40, 128, 8, 9, 1), (128, 64, 16, 3, 1)])
def test_native_draws_are_the_materialised_fields(cuda_device, in_dim, hidden, R, n, swap_every):
    dev, k, cpu = cuda_device, 5, net(in_dim, hidden)
    temps = temperatures(R)
    x0 = torch.randn(n, R, in_dim, generator=torch.Generator().manual_seed(5))
    seed, step0 = 0x1234567887654321, 77
    z, u = _fields(dev, seed, step0, n, R, in_dim, k, swap_every)
    native = run_entry(dev, cpu, x0, temps, k, swap_every, seed=seed, step0=step0, thin=1)
    fed = run_entry(dev, cpu, x0, temps, k, swap_every, z=z, u=u, thin=1)
    for key in ("x", "traj", "swaps"):
        assert torch.equal(native[key], fed[key]), key
    assert torch.isfinite(native["x"]).all() and torch.isfinite(native["traj"]).all()
    assert 0 < int(native["swaps"][R - 1 :].sum()) < int(native["swaps"][: R - 1].sum())  # both branches of the swap ran
    # a sub-block of ladders run alone (another grid, other lanes) reproduces its rows of the full launch
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part = run_entry(dev, cpu, x0[lo:hi], temps, k, swap_every, z=z[:, lo:hi], u=u[:, lo:hi], thin=1)
    assert torch.equal(part["x"], fed["x"][lo:hi]) and torch.equal(part["traj"], fed["traj"][lo:hi])


@pytest.mark.parametrize("in_dim,hidden,R,swap_every,n1,n2", [(5, 64, 4, 1, 2, 2), (64, 128, 8, 1, 2, 2), (100, 128, 2, 1, 2, 2),
                                                              (33, 64, 4, 2, 4, 3), (128, 128, 16, 2, 4, 2)])
def test_two_calls_are_one(cuda_device, in_dim, hidden, R, swap_every, n1, n2):
    """(n1, step0) then (n2, step0 + 2 n1) with an even number of events in the first call is one call of n1 + n2: nothing but x
    passes from one call to the next -- the first call's last evaluation (made for its last event's energies alone) and the
    second call's first are the same function of the same rows -- and the parity of the events restarts with every call."""
    dev, n, cpu = cuda_device, 9, net(in_dim, hidden)
    temps = temperatures(R)
    x0 = torch.randn(n, R, in_dim, generator=torch.Generator().manual_seed(6))
    seed, step0 = 0x0123456789ABCDEF, 41
    whole = run_entry(dev, cpu, x0, temps, n1 + n2, swap_every, seed=seed, step0=step0, thin=1)
    first = run_entry(dev, cpu, x0, temps, n1, swap_every, seed=seed, step0=step0, thin=1)
    second = run_entry(dev, cpu, first["x"], temps, n2, swap_every, seed=seed, step0=step0 + 2 * n1, thin=1)
    assert torch.equal(second["x"], whole["x"])
    assert torch.equal(torch.cat((first["traj"], second["traj"]), dim=1), whole["traj"])
    assert torch.equal(first["swaps"] + second["swaps"], whole["swaps"])
    assert torch.equal(whole["traj"][:, -1], whole["x"][:, 0]) and not torch.equal(whole["x"], x0)
    assert int(whole["swaps"][R - 1 :].sum()) > 0 and int(first["swaps"][: R - 1].sum()) > 0


# ---------------------------------------------------------------------------------
# the step is the running-moments kernel's
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,R", [(5, 64, 4), (40, 64, 2), (64, 128, 8), (100, 128, 16), (128, 64, 32)])
def test_the_step_is_the_langevin_moments_kernels(cuda_device, in_dim, hidden, R):
    """swap_every > k: no event, and slot r's rows, gathered together with their injected noise, are ebm_chain_moments_mlp_f32
    chains at noise_coef[r] (k = 4, burn_in = 0, no energies), bit for bit in x and in the kept states: both calls make the same
    evaluation and spell the same update."""
    dev, (n, k, thin), cpu = cuda_device, (3 if R == 32 else 11, 4, 2), net(in_dim, hidden)
    temps = temperatures(R)
    g = torch.Generator().manual_seed(21)
    x0 = torch.randn(n, R, in_dim, generator=g)
    z = torch.randn(k, n, R, in_dim, generator=g)
    got = run_entry(dev, cpu, x0, temps, k, k + 1, z=z, u=torch.zeros(0, n, R), thin=thin)
    assert int(got["swaps"].sum()) == 0 and torch.isfinite(got["x"]).all()
    coef, _ = ladder(SIGMA, temps)
    spec = copy.deepcopy(cpu).to(dev).fused_spec()
    recip = recip_table(k // 2).to(dev)
    for r in range(R):
        rows = x0[:, r].contiguous().to(dev)
        z_d = z[:, :, r].contiguous().to(dev)
        mom = torch.empty(4, n, in_dim, device=dev)
        traj = torch.empty(n, k, in_dim, device=dev)
        _lib.call(MOMENTS, spec.to_c(), rows.data_ptr(), n, in_dim, 0, k, 0, ETA, ETA**0.5, float(coef[r]), 0, 0.0, recip.data_ptr(),
                  mom.data_ptr(), None, traj.data_ptr(), None, None, None, z_d.data_ptr(), None, 0, 0, _lib.stream_handle(dev))
        torch.cuda.synchronize()
        assert torch.equal(rows.cpu(), got["x"][:, r]), r
        if r == 0:
            assert torch.equal(traj.cpu()[:, thin - 1 :: thin], got["traj"])


# ---------------------------------------------------------------------------------
# states that cannot move
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,R,n", [(5, 64, 4, 19), (33, 128, 8, 5), (100, 64, 2, 19), (40, 128, 32, 2)])
def test_frozen_states_are_permuted_as_the_restatement_permutes_them(cuda_device, in_dim, hidden, R, n):
    """eta = sqrt_eta = 0: no step moves a state, so the final slot matrix is a bit-exact permutation of the start, made by the
    swap decisions alone -- the fp64 restatement's."""
    c = frozen_case(in_dim, hidden, R, n)
    assert c["found"]
    got = _run_case(cuda_device, c, thin=1, sqrt_eta=0.0)
    perm = slot_permutation(got["x"], c["x0"])
    assert torch.equal(perm, slot_permutation(c["ref64"]["x"].float(), c["x0"]))
    assert (perm != torch.arange(R)).any()
    assert torch.equal(got["swaps"], want_swap_counts(c["ref64"]["mask"], n, R))
    assert torch.equal(got["traj"][:, -1], got["x"][:, 0]) and got["traj"].shape == (n, FROZEN_EVENTS, in_dim)


# ---------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,R,n,swap_every,k", [(5, 128, 2, 19, 2, 6), (32, 64, 8, 5, 1, 4), (2, 64, 4, 65, 1, 4)])
def test_wild_start_stays_in_its_ladder(cuda_device, in_dim, hidden, R, n, swap_every, k):
    """A NaN coordinate in one slot of one ladder and a 1e20 coordinate in a slot of another, both in the first wave: every other
    LADDER's outputs are bitwise the clean run's."""
    c = case(in_dim, hidden, R, n, swap_every, k)
    x0 = c["x0"].clone()
    x0[1, 1, in_dim - 1] = float("nan")
    x0[2, 0, 0] = 1e20
    got = run_entry(cuda_device, c["cpu"], x0, c["temps"], k, swap_every, eta=c["eta"], z=c["z"], u=c["u"], thin=c["thin"])
    clean = _run_case(cuda_device, c)
    others = [i for i in range(n) if i not in (1, 2)]
    for key in ("x", "traj"):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][others], clean[key][others]), key
    assert not torch.isfinite(got["x"][1]).all()  # (the NaN stayed in its ladder, and stayed)
    assert torch.equal(clean["swaps"], want_swap_counts(c["ref64"]["mask"], n, R))


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_tempering_mlp.py with real buffers: each raises its code and no buffer is touched."""
    from test_tempering_mlp import EINVAL, _abi_call

    dev, dim = cuda_device, 8
    x = torch.full((16, 132), FILL, device=dev)
    consts = torch.full((2, 64), FILL, device=dev)
    draws = torch.full((2, 4 * 4 * 132), FILL, device=dev)
    traj = torch.full((4 * 3 * 132,), FILL, device=dev)
    real = dict(x=x.data_ptr(), coef=consts[0].data_ptr(), beta=consts[1].data_ptr())
    given = dict(noise=draws[0].data_ptr(), u=draws[1].data_ptr(), traj=traj.data_ptr())
    desc = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
    pointers = {**real, **given}
    for kw, match in EINVAL:
        # the stand-in addresses of the CPU test become real ones: 16 the buffer itself, anything else the buffer off its alignment
        kw = {k: (v if v is None or k not in pointers else pointers[k] + (v - 16) % 16) for k, v in kw.items()}
        with pytest.raises(ValueError, match=match):
            _abi_call(desc, **{**real, **kw})
    with pytest.raises(ValueError, match="bad shape"):
        _abi_call(desc, n=-1, **real)
    with pytest.raises(ValueError, match="energy descriptor is NULL"):
        _abi_call(None, **real)
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
        _abi_call(ta.DoubleWellModel(device=dev).fused_spec().to_c(), **real)
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
        _abi_call(ta.GaussianModel(torch.zeros(dim), torch.eye(dim), device=dev).fused_spec().to_c(), **real)
    with pytest.raises(RuntimeError, match=r"code -2.*no replica-exchange kernel"):
        _abi_call(desc, entry=ANALYTIC, **real)
    with pytest.raises(RuntimeError, match=r"code -3.*got 64, 129, 4"):
        _abi_call(desc, dim=129, **real)
    with pytest.raises(RuntimeError, match=r"code -3.*got 64, 0, 4"):
        _abi_call(desc, dim=0, **real)
    for R in (1, 3, 6, 64):
        with pytest.raises(RuntimeError, match=rf"code -3.*got 64, 8, {R}\)"):
            _abi_call(desc, R=R, **real)
    wide = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
    wide.n_comp = 96
    with pytest.raises(RuntimeError, match=r"code -3.*got 96, 8, 4"):
        _abi_call(wide, **real)
    torch.cuda.synchronize()
    for t in (x, consts, draws, traj):
        assert bool((t == FILL).all())


# ---------------------------------------------------------------------------------
# through ReplicaExchangeLangevin.sample()
# ---------------------------------------------------------------------------------
def test_sample_with_the_opt_in_is_one_launch(cuda_device):
    dev, (n, R, dim, k) = cuda_device, (75, 4, 6, 8)
    cpu = net(dim, 64)
    model = copy.deepcopy(cpu).to(dev)
    temps = temperatures(R)
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    s = ta.ReplicaExchangeLangevin(model, step_size=ETA, noise_scale=SIGMA, temperatures=temps, swap_every=2, device=dev)
    ladders0 = x0.unsqueeze(1).expand(-1, R, -1).contiguous()
    assert s._route(ladders0)[0] == "eager"  # the default
    s.fused_mlp_ladder = True
    assert s._route(ladders0)[0] == "fused_mlp"
    g = torch.Generator(device=dev).manual_seed(5)
    before, before_analytic = hip_calls(ENTRY), hip_calls(ANALYTIC)
    ladders = s.sample(x=x0, n_steps=k, return_replicas=True, generator=g)
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1 and hip_calls(ANALYTIC) == before_analytic
    want_g = torch.Generator(device=dev).manual_seed(5)
    _rng.reserve(want_g, dev, 2 * k)
    assert _rng._get_offset(g) == _rng._get_offset(want_g) == 4 * 2 * k  # as the analytic fused route advances it
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    assert ladders.is_cuda and ladders.shape == (n, R, dim) and torch.isfinite(ladders).all()
    # the states are the entry's at the generator's coordinates
    want = run_entry(dev, cpu, ladders0.cpu(), temps, k, 2, seed=_rng.kernel_seed(5), step0=0, thin=4)
    assert torch.equal(ladders.cpu(), want["x"])
    assert 0 < int(want["swaps"][R - 1 :].sum()) < int(want["swaps"][: R - 1].sum())
    # the three return modes and the diagnostics
    before = hip_calls(ENTRY)
    final = s.sample(x=x0, n_steps=k, generator=torch.Generator(device=dev).manual_seed(5))
    traj, diag = s.sample(x=x0, n_steps=k, thin=4, return_trajectory=True, return_diagnostics=True,
                          generator=torch.Generator(device=dev).manual_seed(5))
    assert hip_calls(ENTRY) == before + 2
    assert final.shape == (n, dim) and torch.equal(final, ladders[:, 0]) and torch.equal(traj[:, -1], final)
    assert traj.shape == (n, k // 4, dim) and torch.equal(traj.cpu(), want["traj"])
    assert sorted(diag) == ["energy", "mean", "swap_acceptance", "var"]
    assert diag["mean"].shape == diag["var"].shape == (k // 4, dim) and diag["energy"].shape == (k // 4,)
    assert diag["swap_acceptance"].shape == (R - 1,)
    assert torch.allclose(diag["mean"], traj.mean(dim=0), atol=1e-5)
    assert torch.allclose(diag["var"], traj.var(dim=0, unbiased=False), rtol=1e-4, atol=1e-6)
    with torch.no_grad():
        assert torch.allclose(diag["energy"], torch.stack([model(traj[:, j].contiguous()).mean() for j in range(k // 4)]), rtol=1e-4)
    assert torch.equal(diag["swap_acceptance"].cpu(), (want["swaps"][R - 1 :].double() / want["swaps"][: R - 1].double()).float())
    # continuing a ladder: two calls of k == one call of 2 k (k an even multiple of swap_every)
    g2 = torch.Generator(device=dev).manual_seed(5)
    half = s.sample(x=x0, n_steps=k, return_replicas=True, generator=g2)
    half_keep = half.clone()
    both = s.sample(x=half, n_steps=k, return_replicas=True, generator=g2)
    whole = s.sample(x=x0, n_steps=2 * k, return_replicas=True, generator=torch.Generator(device=dev).manual_seed(5))
    assert torch.equal(both, whole) and torch.equal(half, half_keep)
    # no step, no ladder: no launch
    before = hip_calls(ENTRY)
    same = s.sample(x=x0, n_steps=0, return_replicas=True, generator=torch.Generator(device=dev).manual_seed(5))
    none = s.sample(x=x0[:0], n_steps=3, generator=torch.Generator(device=dev).manual_seed(5))
    assert hip_calls(ENTRY) == before and torch.equal(same, ladders0) and none.shape == (0, dim)


def test_without_the_opt_in_and_off_its_shapes_sample_stays_eager(cuda_device):
    dev = cuda_device
    before = hip_calls(ENTRY)
    torch.manual_seed(3)
    plain = ta.ReplicaExchangeLangevin(ta.MLPEnergy(6, 64, device=dev), step_size=0.05, device=dev)
    x0 = torch.randn(16, 6, device=dev)
    assert plain._route(torch.zeros(16, 4, 6, device=dev)) == ("eager", None)
    out = plain.sample(x=x0, n_steps=3, generator=torch.Generator(device=dev).manual_seed(1))
    assert out.shape == (16, 6) and out.is_cuda and torch.isfinite(out).all()
    # three slots, a width without kernels, a state of another width than the network's, a scheduled step size: eager with the opt-in
    three = ta.ReplicaExchangeLangevin(ta.MLPEnergy(6, 64, device=dev), step_size=0.05, temperatures=(1.0, 2.0, 4.0), swap_every=1, device=dev)
    three.fused_mlp_ladder = True
    assert three._route(torch.zeros(16, 3, 6, device=dev))[0] == "eager"
    out, diag = three.sample(x=x0, n_steps=3, return_diagnostics=True, generator=torch.Generator(device=dev).manual_seed(1))
    assert out.shape == (16, 6) and torch.isfinite(out).all() and diag["swap_acceptance"].shape == (2,)
    odd = ta.ReplicaExchangeLangevin(ta.MLPEnergy(8, 32, device=dev), step_size=0.05, device=dev)
    odd.fused_mlp_ladder = True
    assert odd._route(torch.zeros(4, 4, 8, device=dev))[0] == "eager"
    plain.fused_mlp_ladder = True
    assert plain._route(torch.zeros(16, 4, 6, device=dev))[0] == "fused_mlp"
    assert plain._route(torch.zeros(16, 4, 7, device=dev))[0] == "eager" and plain._route(torch.zeros(16, 4, 6, device=dev).double())[0] == "eager"
    sched = ta.ReplicaExchangeLangevin(ta.MLPEnergy(6, 64, device=dev), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10), device=dev)
    sched.fused_mlp_ladder = True
    assert sched._route(torch.zeros(16, 4, 6, device=dev))[0] == "eager"
    # an analytic energy keeps its own one-launch route with the opt-in set
    well = ta.ReplicaExchangeLangevin(ta.DoubleWellModel(device=dev), step_size=0.01, device=dev)
    well.fused_mlp_ladder = True
    assert well._route(torch.zeros(16, 4, 6, device=dev))[0] == "fused"
    assert hip_calls(ENTRY) == before


# ---------------------------------------------------------------------------------
# the law
# ---------------------------------------------------------------------------------
def test_the_law_of_a_confining_network_is_the_eager_routes(cuda_device):
    """The confining 2-D network of test_ais_mlp_gpu.py, n = 2048 ladders, T = (1, 2, 4, 8), eta = 0.05, swap_every = 1, 200 steps,
    seed 0, on the fused-MLP route and on the CPU eager route: the mean energy of slot 0 differs by at most 4.5 standard errors of
    the difference (from the ladders' sample variances), the per-pair swap acceptances by at most 4.5 binomial standard errors of
    the difference.  Both routes run the same biased discretisation, so the step-size bias cancels."""
    from test_ais_mlp_gpu import _confining_net

    cpu = _confining_net()
    referee = copy.deepcopy(cpu).double()
    n, dim, k, temps = 2048, 2, 200, (1.0, 2.0, 4.0, 8.0)
    R = len(temps)
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(0))
    tried = torch.tensor([n * len(range(p % 2, k, 2)) for p in range(R - 1)], dtype=torch.float64)
    stats = {}
    for dev in (cuda_device, torch.device("cpu")):
        model = copy.deepcopy(cpu).to(dev)
        s = ta.ReplicaExchangeLangevin(model, step_size=0.05, noise_scale=1.0, temperatures=temps, swap_every=1, device=dev)
        s.fused_mlp_ladder = True
        before = hip_calls(ENTRY)
        x, diag = s.sample(x=x0.to(dev), n_steps=k, thin=k, return_diagnostics=True, generator=torch.Generator(device=dev).manual_seed(0))
        assert hip_calls(ENTRY) == before + (1 if dev.type == "cuda" else 0)
        with torch.no_grad():
            e = referee(x.cpu().double())
        assert torch.isfinite(e).all()
        swp = diag["swap_acceptance"].double().cpu()
        stats[dev.type] = {"e": [(e.mean().item(), e.std().item() / math.sqrt(n))],
                           "swap": [(a, math.sqrt(a * (1.0 - a) / t)) for a, t in zip(swp.tolist(), tried.tolist())]}
    for key in ("e", "swap"):
        for i, ((m1, se1), (m2, se2)) in enumerate(zip(stats["cuda"][key], stats["cpu"][key])):
            z = (m1 - m2) / math.sqrt(se1**2 + se2**2)
            print(f"{key}[{i}]: fused-MLP route {m1:.4f} +- {se1:.4f}, CPU eager route {m2:.4f} +- {se2:.4f}, z = {z:+.2f}")
    assert all(0.0 < a < 1.0 for a, _ in stats["cuda"]["swap"])
    for key in ("e", "swap"):
        for (m1, se1), (m2, se2) in zip(stats["cuda"][key], stats["cpu"][key]):
            assert abs(m1 - m2) <= 4.5 * math.sqrt(se1**2 + se2**2), (key, stats)
