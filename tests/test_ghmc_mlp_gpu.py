"""ebm_ghmc_mlp_chain_f32 on the GPU: the kernel through the C ABI with injected draws against the restatements of
ghmc_mlp_cases.py (the fp64 referee: the decisions equal, the states within the fp32 restatement's own error), what it writes and
what it does not, its native draws against the materialised Philox fields, a run cut in two, a wild start, the refusals with real
buffers, GeneralizedHMC.sample() / sample_moments() and ContrastiveDivergence with the ``fused_mlp`` opt-in, and the law of a
confining 2-D network against the CPU eager route."""

import copy
import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from ghmc_mlp_cases import CASES, EPS, GAMMA, INF_CASE, TEMP, case, constants, net
from helpers import hip_calls
from torchebm_amd.utils.synthetic import two_moons

pytestmark = pytest.mark.gpu
ENTRY = "ebm_ghmc_mlp_chain_f32"
FILL = 7.0
MASK_FILL = 9
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


def run_entry(dev, cpu_model, x0, v0, n_mh, thin, L, eps=EPS, *, gamma=GAMMA, temp=TEMP, z=None, u=None, traj=True, mask=True, seed=0,
              offset=0):
    """One call of the entry -> dict of CPU tensors x, v [n, dim], traj [n, n_mh // thin, dim], accepted [n_mh, n] (bool).  v0
    None: draw_v0 = 1 and v starts from FILL.  Outputs start from their fill and sit in front of a guard: a slot the call did not
    write keeps it, and so must the guards."""
    n, dim = x0.shape
    spec = copy.deepcopy(cpu_model).to(dev).fused_spec()
    assert spec is not None
    x, gx = _guarded(dev, (n, dim), x0)
    v, gv = _guarded(dev, (n, dim), v0)
    tr, gt = _guarded(dev, (n, n_mh // thin, dim)) if traj else (None, None)
    mk, gm = _guarded(dev, (n_mh, n), dtype=torch.uint8, fill=MASK_FILL) if mask else (None, None)
    z_d = None if z is None else z.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, spec.to_c(), x.data_ptr(), v.data_ptr(), n, dim, n_mh, L, eps, gamma, temp, int(v0 is None), thin,
              _lib.ptr(tr), _lib.ptr(mk), _lib.ptr(z_d), _lib.ptr(u_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    for guard, fill in ((gx, FILL), (gv, FILL), (gt, FILL), (gm, MASK_FILL)):
        assert guard is None or bool((guard == fill).all()), "the call wrote behind an output"
    if mk is not None:
        assert bool((mk <= 1).all()), "a slot of the accept mask was not written"
    return {"x": x.cpu(), "v": v.cpu(), "traj": None if tr is None else tr.cpu(), "accepted": None if mk is None else mk.cpu().bool()}


def _run_case(dev, c, **kw):
    return run_entry(dev, c["cpu"], c["x0"], c["v0"], c["n_mh"], c["thin"], c["L"], c["eps"], gamma=c["gamma"], temp=c["temp"],
                     z=c["z"], u=c["u"], **kw)


# ---------------------------------------------------------------------------------
# the transition against the restatements
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,n,n_mh,thin,L,gamma", [(*c, GAMMA) for c in CASES] + [(*INF_CASE, math.inf)])
def test_cases_with_injected_draws(cuda_device, in_dim, hidden, n, n_mh, thin, L, gamma):
    """The decisions are the fp64 restatement's (no decision of a case is closer than MARGIN_BAR to its threshold); x, v and the
    kept positions are no further from fp64 than max(4 x the fp32 restatement's own max error, 4e-6 x max |ref|), the bar
    test_kinetic_mlp_gpu.py and test_ais_mlp_gpu.py give the same evaluation; every row written, nothing behind them.

    Measured on an MI355X (kernel error / fp32 restatement error, the largest of x, v, traj per case): see
    docs/design/ghmc_mlp.md."""
    c = case(in_dim, hidden, n, n_mh, thin, L, gamma)
    got = _run_case(cuda_device, c)  # (run_entry checks the guards behind x, v, traj and the mask)
    ref32, ref64 = c["ref32"], c["ref64"]
    assert got["traj"].shape == (n, n_mh // thin, in_dim) and got["accepted"].shape == (n_mh, n)
    figures = {}
    for key in ("x", "v", "traj"):
        ref = ref64[key]
        err_hip = (got[key].double() - ref).abs().max().item()
        err_torch = (ref32[key].double() - ref).abs().max().item()
        figures[key] = (err_hip, err_torch, ref.abs().max().item())
        print(f"dim {in_dim} H {hidden} n {n} n_mh {n_mh} L {L} gamma {gamma}: {key} kernel err {err_hip:.3e}, fp32 restatement err "
              f"{err_torch:.3e} ({err_hip / max(err_torch, 1e-30):.2f} x), max|ref| {figures[key][2]:.3e}")
    wrong = int((got["accepted"] != ref64["accepted"]).sum())
    print(f"    decisions that differ from fp64: {wrong} of {ref64['accepted'].numel()}")
    assert wrong == 0
    for key, (err_hip, err_torch, scale) in figures.items():
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
        assert err_hip <= max(4.0 * err_torch, 4e-6 * scale), (key, err_hip, err_torch, scale)


@pytest.mark.parametrize("in_dim,hidden,n,n_mh,thin,L", [(5, 128, 37, 4, 2, 1), (100, 64, 129, 4, 2, 3)])
def test_a_call_without_trajectory_and_mask_and_a_drawn_start(cuda_device, in_dim, hidden, n, n_mh, thin, L):
    c = case(in_dim, hidden, n, n_mh, thin, L)
    got = _run_case(cuda_device, c)
    lean = _run_case(cuda_device, c, traj=False, mask=False)
    assert lean["traj"] is None and lean["accepted"] is None and torch.equal(lean["x"], got["x"]) and torch.equal(lean["v"], got["v"])
    only_mask = _run_case(cuda_device, c, traj=False)
    assert torch.equal(only_mask["accepted"], got["accepted"]) and torch.equal(only_mask["x"], got["x"])
    # draw_v0: v is output only, every row written
    drawn = run_entry(cuda_device, c["cpu"], c["x0"], None, n_mh, thin, L, z=c["z"], u=c["u"], seed=3, offset=9)
    assert not bool((drawn["v"] == FILL).any()) and torch.isfinite(drawn["v"]).all()


# ---------------------------------------------------------------------------------
# native draws
# ---------------------------------------------------------------------------------
def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


def _fields(dev, seed, offset, n, dim, n_mh, L, eps=EPS):
    """v0, z, u of a call at (seed, offset): step `offset` scaled by sqrt_temp, normals at offset + 1 + 2 t, uniforms at
    offset + 2 + 2 t."""
    sqrt_temp = constants(eps, L, GAMMA, TEMP)[2]
    v0 = (sqrt_temp * _field(dev, _lib.NOISE_NORMAL, seed, offset, n * dim)).view(n, dim).cpu()
    z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + 2 * t, n * dim) for t in range(n_mh)]).view(n_mh, n, dim).cpu()
    u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, offset + 2 + 2 * t, n) for t in range(n_mh)]).view(n_mh, n).cpu()
    return v0, z, u


@pytest.mark.parametrize("in_dim,hidden,n", [(5, 64, 37), (2, 64, 70), (33, 128, 37), (40, 128, 70), (128, 64, 37)])
def test_native_draws_are_the_materialised_fields(cuda_device, in_dim, hidden, n):
    dev, (n_mh, thin, L), cpu = cuda_device, (5, 2, 2), net(in_dim, hidden)
    x0 = torch.randn(n, in_dim, generator=torch.Generator().manual_seed(5))
    seed, offset = 0x1234567887654321, 77
    v0, z, u = _fields(dev, seed, offset, n, in_dim, n_mh, L)
    native = run_entry(dev, cpu, x0, None, n_mh, thin, L, seed=seed, offset=offset)
    fed = run_entry(dev, cpu, x0, v0, n_mh, thin, L, z=z, u=u)
    keys = ("x", "v", "traj", "accepted")
    for key in keys:
        assert torch.equal(native[key], fed[key]), key
    assert all(torch.isfinite(native[key]).all() for key in ("x", "v", "traj"))
    assert native["accepted"].any() and (~native["accepted"]).any()  # both branches ran
    # either draw injected without the other, and injected draws with draw_v0: the rest still comes from the fields
    for kw in (dict(z=z), dict(u=u), dict(z=z, u=u)):
        mixed = run_entry(dev, cpu, x0, None, n_mh, thin, L, seed=seed, offset=offset, **kw)
        for key in keys:
            assert torch.equal(mixed[key], fed[key]), (key, sorted(kw))
    # a sub-block of chains run alone (another grid, other lanes) reproduces its rows of the full launch
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part = run_entry(dev, cpu, x0[lo:hi], v0[lo:hi], n_mh, thin, L, z=z[:, lo:hi], u=u[:, lo:hi])
    for key in ("x", "v", "traj"):
        assert torch.equal(part[key], fed[key][lo:hi]), key
    assert torch.equal(part["accepted"], fed["accepted"][:, lo:hi])


@pytest.mark.parametrize("in_dim,hidden", [(5, 64), (64, 128), (100, 128)])
def test_two_calls_are_one(cuda_device, in_dim, hidden):
    """(n1, offset) then (n2, offset + 2 n1) with draw_v0 = 0 is one call of n1 + n2: nothing but x and v passes from one
    transition to the next."""
    dev, (n, n1, n2, L), cpu = cuda_device, (37, 3, 4, 2), net(in_dim, hidden)
    x0 = torch.randn(n, in_dim, generator=torch.Generator().manual_seed(6))
    seed, offset = 0x0123456789ABCDEF, 41
    whole = run_entry(dev, cpu, x0, None, n1 + n2, 1, L, seed=seed, offset=offset)
    first = run_entry(dev, cpu, x0, None, n1, 1, L, seed=seed, offset=offset)
    second = run_entry(dev, cpu, first["x"], first["v"], n2, 1, L, seed=seed, offset=offset + 2 * n1)
    assert torch.equal(second["x"], whole["x"]) and torch.equal(second["v"], whole["v"])
    assert torch.equal(torch.cat((first["accepted"], second["accepted"])), whole["accepted"])
    assert torch.equal(torch.cat((first["traj"], second["traj"]), dim=1), whole["traj"])
    assert torch.equal(whole["traj"][:, -1], whole["x"]) and not torch.equal(whole["x"], x0)
    assert whole["accepted"].any() and (~whole["accepted"]).any()


# ---------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,n,n_mh,thin,L", [(5, 128, 37, 4, 2, 1), (32, 64, 129, 6, 3, 1), (33, 128, 37, 4, 2, 3)])
def test_wild_start_stays_in_its_chain(cuda_device, in_dim, hidden, n, n_mh, thin, L):
    """A NaN coordinate in one chain and a 1e20 coordinate in another, both in the first wave (which then takes the literal path of
    the trajectory): every other chain's outputs are bitwise the clean run's."""
    c = case(in_dim, hidden, n, n_mh, thin, L)
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    got = run_entry(cuda_device, c["cpu"], x0, c["v0"], n_mh, thin, L, c["eps"], z=c["z"], u=c["u"])
    clean = _run_case(cuda_device, c)
    others = [i for i in range(n) if i not in (3, 7)]
    for key in ("x", "v", "traj"):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][others], clean[key][others]), key
    assert torch.equal(got["accepted"][:, others], clean["accepted"][:, others])
    assert torch.equal(clean["accepted"], c["ref64"]["accepted"])


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_ghmc_mlp.py with real buffers: each raises its code and no buffer is touched."""
    from test_ghmc_mlp import EINVAL, _abi_call

    dev, (n, dim) = cuda_device, (4, 8)
    x = torch.full((n, 132), FILL, device=dev)
    v = torch.full((n, 132), FILL, device=dev)
    real = dict(x=x.data_ptr(), v=v.data_ptr())
    desc = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
    for kw, match in EINVAL:
        with pytest.raises(ValueError, match=match):
            _abi_call(desc, **{**real, **kw})
    with pytest.raises(ValueError, match="bad shape"):
        _abi_call(desc, n=-1, **real)
    with pytest.raises(ValueError, match="16-byte aligned"):
        _abi_call(desc, **{**real, "v": v.data_ptr() + 4})
    with pytest.raises(ValueError, match="energy descriptor is NULL"):
        _abi_call(None, **real)
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
        _abi_call(ta.DoubleWellModel(device=dev).fused_spec().to_c(), **real)
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
        _abi_call(ta.GaussianModel(torch.zeros(dim), torch.eye(dim), device=dev).fused_spec().to_c(), **real)
    with pytest.raises(RuntimeError, match=r"code -2.*no generalized-HMC kernel"):
        _abi_call(desc, entry="ebm_ghmc_chain_f32", **real)
    with pytest.raises(RuntimeError, match=r"code -3.*got 64, 129"):
        _abi_call(desc, dim=129, **real)
    with pytest.raises(RuntimeError, match=r"code -3.*got 64, 0"):
        _abi_call(desc, dim=0, **real)
    wide = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
    wide.n_comp = 96
    with pytest.raises(RuntimeError, match=r"code -3.*got 96, 8"):
        _abi_call(wide, **real)
    torch.cuda.synchronize()
    for t in (x, v):
        assert bool((t == FILL).all())


# ---------------------------------------------------------------------------------
# through GeneralizedHMC.sample()
# ---------------------------------------------------------------------------------
def test_sample_with_the_opt_in_is_one_launch(cuda_device):
    dev, (n, dim, k1, k2, L) = cuda_device, (300, 6, 3, 5, 2)
    k = k1 + k2
    cpu = net(dim, 64)
    model = copy.deepcopy(cpu).to(dev)
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    s = ta.GeneralizedHMC(model, step_size=EPS, n_leapfrog_steps=L, friction=GAMMA, temperature=TEMP, device=dev)
    assert s._route(x0)[0] == "eager"  # the default
    s.fused_mlp = True
    assert s._route(x0)[0] == "fused_mlp"
    g = torch.Generator(device=dev).manual_seed(5)
    before, before_analytic = hip_calls(ENTRY), hip_calls("ebm_ghmc_chain_f32")
    x, v = s.sample(x=x0, n_steps=k, return_velocity=True, generator=g)
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1 and hip_calls("ebm_ghmc_chain_f32") == before_analytic
    assert _rng._get_offset(g) == 4 * (2 * k + 1)  # as the analytic fused route advances it
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    assert x.is_cuda and v.is_cuda and x.shape == v.shape == (n, dim) and torch.isfinite(x).all() and torch.isfinite(v).all()
    # the states are the entry's at the generator's coordinates
    want = run_entry(dev, cpu, x0.cpu(), None, k, 1, L, seed=_rng.kernel_seed(5), offset=0)
    assert torch.equal(x.cpu(), want["x"]) and torch.equal(v.cpu(), want["v"])
    assert want["accepted"].any() and (~want["accepted"]).any()
    # cut in two: the second call continues from the returned velocity at the Philox step the first one stopped at
    g = torch.Generator(device=dev).manual_seed(5)
    xa, va = s.sample(x=x0, n_steps=k1, return_velocity=True, generator=g)
    assert _rng._get_offset(g) == 4 * (2 * k1 + 1)
    _rng._set_offset(g, 4 * 2 * k1)  # (a call owns 2 k + 1 steps; the uncut run drew step 2 k1 + 1 + 2 t where this one draws its step 1 + 2 t)
    va_keep = va.clone()
    xb, vb = s.sample(x=xa, n_steps=k2, velocity=va, return_velocity=True, reset_schedulers=False, generator=g)
    assert torch.equal(va, va_keep), "the caller's velocity was touched"
    assert torch.equal(xb, x) and torch.equal(vb, v)
    # trajectory and diagnostics: the kept positions and their statistics, the energy the model's, the rate from the mask
    traj, diag = s.sample(x=x0, n_steps=k, thin=4, return_trajectory=True, return_diagnostics=True,
                          generator=torch.Generator(device=dev).manual_seed(5))
    assert traj.shape == (n, k // 4, dim) and diag["mean"].shape == diag["var"].shape == (k // 4, dim)
    assert diag["energy"].shape == diag["acceptance_rate"].shape == (k // 4,) and diag["kinetic_temperature"].shape == ()
    assert torch.allclose(diag["mean"], traj.mean(dim=0), atol=1e-5)
    assert torch.allclose(diag["var"], traj.var(dim=0, unbiased=False), rtol=1e-4, atol=1e-6)
    with torch.no_grad():
        assert torch.allclose(diag["energy"], torch.stack([model(traj[:, j].contiguous()).mean() for j in range(k // 4)]), rtol=1e-4)
    assert torch.allclose(diag["kinetic_temperature"], v.square().mean())
    want_rate = want["accepted"][3::4][: k // 4].float().mean(dim=1)
    assert torch.allclose(diag["acceptance_rate"].cpu(), want_rate, rtol=1e-6, atol=0) and bool(((want_rate > 0) & (want_rate < 1)).all())
    assert torch.equal(traj.cpu()[:, -1], run_entry(dev, cpu, x0.cpu(), None, k, 4, L, seed=_rng.kernel_seed(5), offset=0)["traj"][:, -1])
    # no transition: the start and its drawn velocities, no launch of the entry
    before = hip_calls(ENTRY)
    x, v = s.sample(x=x0, n_steps=0, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(5))
    assert hip_calls(ENTRY) == before and torch.equal(x, x0) and x.data_ptr() != x0.data_ptr() and v.shape == (n, dim)
    sqrt_temp = constants(EPS, L, GAMMA, TEMP)[2]
    assert torch.equal(v.cpu(), (sqrt_temp * _field(dev, _lib.NOISE_NORMAL, _rng.kernel_seed(5), 0, n * dim)).view(n, dim).cpu())


def test_without_the_opt_in_and_off_its_shapes_sample_stays_eager(cuda_device):
    dev = cuda_device
    before = hip_calls(ENTRY)
    torch.manual_seed(3)
    plain = ta.GeneralizedHMC(ta.MLPEnergy(6, 64, device=dev), step_size=0.1, n_leapfrog_steps=2, device=dev)
    x0 = torch.randn(64, 6, device=dev)
    assert plain._route(x0)[0] == "eager"
    out = plain.sample(x=x0, n_steps=3, generator=torch.Generator(device=dev).manual_seed(1))
    assert out.shape == (64, 6) and out.is_cuda and torch.isfinite(out).all()
    # a width without kernels, a state of another width than the network's, a scheduled step size, conditioning: eager with the opt-in
    odd = ta.GeneralizedHMC(ta.MLPEnergy(8, 96, device=dev), step_size=0.1, device=dev)
    odd.fused_mlp = True
    assert odd._route(torch.zeros(4, 8, device=dev))[0] == "eager"
    plain.fused_mlp = True
    assert plain._route(x0)[0] == "fused_mlp" and plain._route(torch.zeros(4, 7, device=dev))[0] == "eager"
    assert plain._route(x0, {"label": 1})[0] == "eager" and plain._route(x0.double())[0] == "eager"
    sched = ta.GeneralizedHMC(ta.MLPEnergy(6, 64, device=dev), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10), device=dev)
    sched.fused_mlp = True
    assert sched._route(x0)[0] == "eager"
    # an analytic energy keeps its own one-launch route with the opt-in set
    well = ta.GeneralizedHMC(ta.DoubleWellModel(device=dev), step_size=0.1, device=dev)
    well.fused_mlp = True
    assert well._route(x0)[0] == "fused"
    assert hip_calls(ENTRY) == before


def test_sample_moments_of_an_opted_in_sampler_launches_neither_fused_entry(cuda_device):
    """kinetic_moments.sample_moments fuses on the route "fused" only: an opted-in MLP sampler runs its step-by-step recurrence,
    every step a sample() of one transition -- neither ebm_kinetic_moments_f32 nor ebm_ghmc_chain_f32 is launched."""
    dev = cuda_device
    torch.manual_seed(3)
    s = ta.GeneralizedHMC(ta.MLPEnergy(6, 64, device=dev), step_size=0.3, n_leapfrog_steps=2, device=dev)
    s.fused_mlp = True
    x0 = torch.randn(32, 6, device=dev)
    assert s._route(x0)[0] == "fused_mlp"
    before = hip_calls("ebm_kinetic_moments_f32"), hip_calls("ebm_ghmc_chain_f32")
    x, mom = s.sample_moments(x=x0, n_steps=8, burn_in=2, generator=torch.Generator(device=dev).manual_seed(1))
    assert (hip_calls("ebm_kinetic_moments_f32"), hip_calls("ebm_ghmc_chain_f32")) == before
    assert x.shape == (32, 6) and x.is_cuda and torch.isfinite(x).all() and torch.isfinite(mom.mean).all()
    assert mom.acceptance_rate.shape == (8,)


@pytest.mark.parametrize("persistent", [False, True], ids=["cd_k", "persistent"])
def test_contrastive_divergence_makes_one_launch_per_call(cuda_device, persistent):
    dev = cuda_device
    torch.manual_seed(6)
    model = ta.MLPEnergy(2, 64, device=dev)
    sampler = ta.GeneralizedHMC(model, step_size=0.1, n_leapfrog_steps=2, friction=1.0, temperature=1.0, device=dev)
    sampler.fused_mlp = True
    cd = ta.losses.ContrastiveDivergence(model=model, sampler=sampler, k_steps=5, persistent=persistent, buffer_size=512, init_steps=0,
                                         device=dev)
    data = two_moons(n_samples=256, noise=0.05, seed=0, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    for _ in range(3):
        before = hip_calls(ENTRY)
        model.zero_grad()
        loss, negatives = cd(data, generator=g)
        assert hip_calls(ENTRY) == before + 1
        assert torch.isfinite(loss) and negatives.shape == data.shape and negatives.is_cuda and torch.isfinite(negatives).all()
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


# ---------------------------------------------------------------------------------
# the law
# ---------------------------------------------------------------------------------
def test_the_law_of_a_confining_network_is_the_eager_routes(cuda_device):
    """The confining 2-D network of test_ais_mlp_gpu.py, n = 4096, eps = 0.3, L = 2, gamma = 1, T = 1, 300 transitions, seed 0, on
    the fused-MLP route and on the CPU eager route: the mean energy of the final positions and the kinetic temperature differ by at
    most 4.5 standard errors of the difference (from the chains' sample variances), the acceptance rates over all n x 300
    decisions by at most 4.5 binomial standard errors of the difference."""
    from test_ais_mlp_gpu import _confining_net

    cpu = _confining_net()
    referee = copy.deepcopy(cpu).double()
    n, dim, k = 4096, 2, 300
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(0))
    stats = {}
    for dev in (cuda_device, torch.device("cpu")):
        model = copy.deepcopy(cpu).to(dev)
        s = ta.GeneralizedHMC(model, step_size=0.3, n_leapfrog_steps=2, friction=1.0, temperature=1.0, device=dev)
        s.fused_mlp = True
        assert s._route(x0.to(dev))[0] == ("fused_mlp" if dev.type == "cuda" else "eager")
        before = hip_calls(ENTRY)
        x, diag, v = s.sample(x=x0.to(dev), n_steps=k, return_diagnostics=True, return_velocity=True,
                              generator=torch.Generator(device=dev).manual_seed(0))
        assert hip_calls(ENTRY) == before + (1 if dev.type == "cuda" else 0)
        with torch.no_grad():
            e = referee(x.cpu().double())
        kt = v.cpu().double().square().mean(dim=1)
        assert torch.isfinite(e).all() and torch.isfinite(kt).all()
        assert math.isclose(kt.mean().item(), diag["kinetic_temperature"].item(), rel_tol=1e-5)
        rate = diag["acceptance_rate"].double().mean().item()  # thin = 1: every transition is kept
        assert diag["acceptance_rate"].shape == (k,)
        stats[dev.type] = {"e": (e.mean().item(), e.std().item() / math.sqrt(n)), "kt": (kt.mean().item(), kt.std().item() / math.sqrt(n)),
                           "acc": (rate, math.sqrt(rate * (1.0 - rate) / (n * k)))}
    for key in ("e", "kt", "acc"):
        (m1, se1), (m2, se2) = stats["cuda"][key], stats["cpu"][key]
        z = (m1 - m2) / math.sqrt(se1**2 + se2**2)
        print(f"{key}: fused-MLP route {m1:.4f} +- {se1:.4f}, CPU eager route {m2:.4f} +- {se2:.4f}, z = {z:+.2f}")
    assert 0.0 < stats["cuda"]["acc"][0] < 1.0
    for key in ("e", "kt", "acc"):
        (m1, se1), (m2, se2) = stats["cuda"][key], stats["cpu"][key]
        assert abs(m1 - m2) <= 4.5 * math.sqrt(se1**2 + se2**2), (key, stats)
