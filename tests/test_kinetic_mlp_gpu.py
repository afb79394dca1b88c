"""ebm_kinetic_mlp_chain_f32 on the GPU: the kernel through the C ABI with injected noise against the restatements of
kinetic_mlp_cases.py (the fp64 referee), what it writes and what it does not, its native draws against the materialised Philox
fields, a run cut in two, a wild start, the refusals with real buffers, UnderdampedLangevin.sample() and ContrastiveDivergence
with the ``fused_mlp`` opt-in, and the law of a confining 2-D network against the CPU eager route."""

import copy
import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls
from kinetic_mlp_cases import CASES, GAMMA, STEP, TEMP, case, constants, net
from torchebm_amd.utils.synthetic import two_moons

pytestmark = pytest.mark.gpu
ENTRY = "ebm_kinetic_mlp_chain_f32"
FILL = 7.0
GUARD = 64  # floats behind every output that must keep FILL


def _guarded(dev, shape, src=None):
    """A tensor of `shape` in front of GUARD floats of FILL (in one allocation) -> (tensor, guard)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + GUARD,), FILL, device=dev)
    t = buf[:numel].view(shape)
    if src is not None:
        t.copy_(src)
    return t, buf[numel:]


def run_entry(dev, cpu_model, x0, v0, k, thin, h=STEP, *, gamma=GAMMA, temp=TEMP, noise=None, traj=True, seed=0, offset=0):
    """One call of the entry -> dict of CPU tensors x, v [n, dim], traj [n, k // thin, dim].  v0 None: draw_v0 = 1 and v starts
    from FILL.  Outputs start from FILL and sit in front of a guard: a slot the call did not write keeps it, and so must the guards."""
    n, dim = x0.shape
    spec = copy.deepcopy(cpu_model).to(dev).fused_spec()
    assert spec is not None
    x, gx = _guarded(dev, (n, dim), x0)
    v, gv = _guarded(dev, (n, dim), v0)
    tr, gt = _guarded(dev, (n, k // thin, dim)) if traj else (None, None)
    noise_d = None if noise is None else noise.to(dev).contiguous()
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, spec.to_c(), x.data_ptr(), v.data_ptr(), n, dim, k, h, gamma, temp, int(v0 is None), thin,
              _lib.ptr(tr), _lib.ptr(noise_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    for guard in (gx, gv, gt):
        assert guard is None or bool((guard == FILL).all()), "the call wrote behind an output"
    return {"x": x.cpu(), "v": v.cpu(), "traj": None if tr is None else tr.cpu()}


def _run_case(dev, c, **kw):
    return run_entry(dev, c["cpu"], c["x0"], c["v0"], c["k"], c["thin"], c["h"], noise=c["noise"], **kw)


# ---------------------------------------------------------------------------------
# the recurrence against the restatements
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,n,k,thin", CASES)
def test_cases_with_injected_noise(cuda_device, in_dim, hidden, n, k, thin):
    """The bar test_mlp_wide_gpu.py and test_ais_mlp_gpu.py give the same evaluation: x, v and the kept positions no further
    from fp64 than max(4 x the fp32 restatement's own max error, 4e-6 x max |ref|); every row written, nothing behind them."""
    c = case(in_dim, hidden, n, k, thin)
    got = _run_case(cuda_device, c)  # (run_entry checks the guards behind x, v and traj)
    ref32, ref64 = c["ref32"], c["ref64"]
    assert got["traj"].shape == (n, k // thin, in_dim)
    figures = {}
    for key in ("x", "v", "traj"):
        ref = ref64[key]
        err_hip = (got[key].double() - ref).abs().max().item()
        err_torch = (ref32[key].double() - ref).abs().max().item()
        figures[key] = (err_hip, err_torch, ref.abs().max().item())
        print(f"dim {in_dim} H {hidden} n {n} k {k}: {key} kernel err {err_hip:.3e}, fp32 restatement err {err_torch:.3e}"
              f" ({err_hip / max(err_torch, 1e-30):.2f} x), max|ref| {figures[key][2]:.3e}")
    for key, (err_hip, err_torch, scale) in figures.items():
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
        assert err_hip <= max(4.0 * err_torch, 4e-6 * scale), (key, err_hip, err_torch, scale)


@pytest.mark.parametrize("in_dim,hidden,n,k,thin", [(5, 128, 37, 4, 2), (100, 64, 129, 4, 2)])
def test_a_call_without_a_trajectory_and_a_drawn_start(cuda_device, in_dim, hidden, n, k, thin):
    c = case(in_dim, hidden, n, k, thin)
    got = _run_case(cuda_device, c)
    lean = _run_case(cuda_device, c, traj=False)
    assert lean["traj"] is None and torch.equal(lean["x"], got["x"]) and torch.equal(lean["v"], got["v"])
    # draw_v0: v is output only, every row written
    drawn = run_entry(cuda_device, c["cpu"], c["x0"], None, k, thin, noise=c["noise"], seed=3, offset=9)
    assert not bool((drawn["v"] == FILL).any()) and torch.isfinite(drawn["v"]).all()


# ---------------------------------------------------------------------------------
# native draws
# ---------------------------------------------------------------------------------
def _field(dev, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, _lib.NOISE_NORMAL, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


@pytest.mark.parametrize("in_dim,hidden,n", [(5, 64, 37), (2, 64, 70), (33, 128, 37), (40, 128, 70), (128, 64, 37)])
def test_native_draws_are_the_materialised_fields(cuda_device, in_dim, hidden, n):
    dev, (k, thin), cpu = cuda_device, (7, 3), net(in_dim, hidden)
    x0 = torch.randn(n, in_dim, generator=torch.Generator().manual_seed(5))
    seed, offset = 0x1234567887654321, 77
    sqrt_temp = constants(STEP, GAMMA, TEMP)[3]
    v0 = (sqrt_temp * _field(dev, seed, offset, n * in_dim)).view(n, in_dim).cpu()  # the start velocity: step `offset`
    noise = torch.stack([_field(dev, seed, offset + 1 + s, n * in_dim) for s in range(k)]).view(k, n, in_dim).cpu()
    native = run_entry(dev, cpu, x0, None, k, thin, seed=seed, offset=offset)
    fed = run_entry(dev, cpu, x0, v0, k, thin, noise=noise)
    for key in ("x", "v", "traj"):
        assert torch.equal(native[key], fed[key]), key
        assert torch.isfinite(native[key]).all()
    # injected noise with draw_v0: the start velocity still comes from the field
    mixed = run_entry(dev, cpu, x0, None, k, thin, noise=noise, seed=seed, offset=offset)
    assert torch.equal(mixed["x"], fed["x"]) and torch.equal(mixed["v"], fed["v"])
    # a sub-block of chains run alone (another grid, other lanes) reproduces its rows of the full launch
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part = run_entry(dev, cpu, x0[lo:hi], v0[lo:hi], k, thin, noise=noise[:, lo:hi])
    for key in ("x", "v", "traj"):
        assert torch.equal(part[key], fed[key][lo:hi]), key


@pytest.mark.parametrize("in_dim,hidden", [(5, 64), (64, 128), (100, 128)])
def test_two_calls_are_one(cuda_device, in_dim, hidden):
    """(k1, offset) then (k2, offset + k1) with draw_v0 = 0 is one call of k1 + k2: the closing and the opening kick are not
    merged, and the evaluation the second call starts with is the one the first call ended with."""
    dev, (n, k1, k2), cpu = cuda_device, (37, 4, 7), net(in_dim, hidden)
    x0 = torch.randn(n, in_dim, generator=torch.Generator().manual_seed(6))
    seed, offset = 0x0123456789ABCDEF, 41
    whole = run_entry(dev, cpu, x0, None, k1 + k2, 1, seed=seed, offset=offset)
    first = run_entry(dev, cpu, x0, None, k1, 1, seed=seed, offset=offset)
    second = run_entry(dev, cpu, first["x"], first["v"], k2, 1, seed=seed, offset=offset + k1)
    assert torch.equal(second["x"], whole["x"]) and torch.equal(second["v"], whole["v"])
    assert torch.equal(torch.cat((first["traj"], second["traj"]), dim=1), whole["traj"])
    assert torch.equal(whole["traj"][:, -1], whole["x"]) and not torch.equal(whole["x"], x0)


# ---------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,n,k,thin", [(5, 128, 37, 4, 2), (32, 64, 129, 11, 3)])
def test_wild_start_stays_in_its_chain(cuda_device, in_dim, hidden, n, k, thin):
    """A NaN coordinate in one chain and a 1e20 coordinate in another, both in the first wave: every other chain's outputs are
    bitwise the clean run's."""
    c = case(in_dim, hidden, n, k, thin)
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    got = run_entry(cuda_device, c["cpu"], x0, c["v0"], k, thin, noise=c["noise"])
    clean = _run_case(cuda_device, c)
    others = [i for i in range(n) if i not in (3, 7)]
    for key in ("x", "v", "traj"):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][others], clean[key][others]), key
    assert torch.isnan(got["x"][3]).any() and not bool((got["x"][7].abs() < 1e10).all())


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_kinetic_mlp.py with real buffers: each raises its code and no buffer is touched."""
    from test_kinetic_mlp import EINVAL, _abi_call

    dev, (n, dim) = cuda_device, (4, 8)
    x = torch.full((n, 132), FILL, device=dev)
    v = torch.full((n, 132), FILL, device=dev)
    real = dict(x=x.data_ptr(), v=v.data_ptr())
    desc = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
    for kw, match in EINVAL:
        with pytest.raises(ValueError, match=match):
            _abi_call(desc, **{**real, **kw})
    with pytest.raises(ValueError, match="energy descriptor is NULL"):
        _abi_call(None, **real)
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
        _abi_call(ta.DoubleWellModel(device=dev).fused_spec().to_c(), **real)
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
        _abi_call(ta.GaussianModel(torch.zeros(dim), torch.eye(dim), device=dev).fused_spec().to_c(), **real)
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
# through UnderdampedLangevin.sample()
# ---------------------------------------------------------------------------------
def test_sample_with_the_opt_in_is_one_launch(cuda_device):
    dev, (n, dim, k1, k2) = cuda_device, (300, 6, 5, 8)
    k = k1 + k2
    cpu = net(dim, 64)
    model = copy.deepcopy(cpu).to(dev)
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    s = ta.UnderdampedLangevin(model, step_size=STEP, friction=GAMMA, temperature=TEMP, device=dev)
    assert s._route(x0)[0] == "eager"  # the default
    s.fused_mlp = True
    assert s._route(x0)[0] == "fused_mlp"
    g = torch.Generator(device=dev).manual_seed(5)
    before, before_analytic = hip_calls(ENTRY), hip_calls("ebm_kinetic_chain_f32")
    x, v = s.sample(x=x0, n_steps=k, return_velocity=True, generator=g)
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1 and hip_calls("ebm_kinetic_chain_f32") == before_analytic
    assert _rng._get_offset(g) == 4 * (k + 1)
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    assert x.is_cuda and v.is_cuda and x.shape == v.shape == (n, dim) and torch.isfinite(x).all() and torch.isfinite(v).all()
    # the states are the entry's at the generator's coordinates
    want = run_entry(dev, cpu, x0.cpu(), None, k, 1, seed=_rng.kernel_seed(5), offset=0)
    assert torch.equal(x.cpu(), want["x"]) and torch.equal(v.cpu(), want["v"])
    # cut in two: the second call continues from the returned velocity at the Philox step the first one stopped at
    g = torch.Generator(device=dev).manual_seed(5)
    xa, va = s.sample(x=x0, n_steps=k1, return_velocity=True, generator=g)
    assert _rng._get_offset(g) == 4 * (k1 + 1)
    _rng._set_offset(g, 4 * k1)  # (a call owns k + 1 steps; the uncut run drew step k1 + 1 + s where this one draws its step 1 + s)
    va_keep = va.clone()
    xb, vb = s.sample(x=xa, n_steps=k2, velocity=va, return_velocity=True, reset_schedulers=False, generator=g)
    assert torch.equal(va, va_keep), "the caller's velocity was touched"
    assert torch.equal(xb, x) and torch.equal(vb, v)
    # trajectory and diagnostics: the kept positions and their statistics, the energy the model's
    traj, diag = s.sample(x=x0, n_steps=k, thin=4, return_trajectory=True, return_diagnostics=True,
                          generator=torch.Generator(device=dev).manual_seed(5))
    assert traj.shape == (n, k // 4, dim) and diag["mean"].shape == diag["var"].shape == (k // 4, dim)
    assert diag["energy"].shape == (k // 4,) and diag["kinetic_temperature"].shape == ()
    assert torch.allclose(diag["mean"], traj.mean(dim=0), atol=1e-5)
    assert torch.allclose(diag["var"], traj.var(dim=0, unbiased=False), rtol=1e-4, atol=1e-6)
    with torch.no_grad():
        assert torch.allclose(diag["energy"], torch.stack([model(traj[:, j].contiguous()).mean() for j in range(k // 4)]), rtol=1e-4)
    assert torch.allclose(diag["kinetic_temperature"], v.square().mean())
    # no step: the start and its drawn velocities, no launch of the entry
    before = hip_calls(ENTRY)
    x, v = s.sample(x=x0, n_steps=0, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(5))
    assert hip_calls(ENTRY) == before and torch.equal(x, x0) and x.data_ptr() != x0.data_ptr() and v.shape == (n, dim)
    assert torch.equal(v.cpu(), (constants(STEP, GAMMA, TEMP)[3] * _field(dev, _rng.kernel_seed(5), 0, n * dim)).view(n, dim).cpu())


def test_without_the_opt_in_and_off_its_shapes_sample_stays_eager(cuda_device):
    dev = cuda_device
    before = hip_calls(ENTRY)
    torch.manual_seed(3)
    plain = ta.UnderdampedLangevin(ta.MLPEnergy(6, 64, device=dev), step_size=0.1, device=dev)
    x0 = torch.randn(64, 6, device=dev)
    assert plain._route(x0)[0] == "eager"
    out = plain.sample(x=x0, n_steps=3, generator=torch.Generator(device=dev).manual_seed(1))
    assert out.shape == (64, 6) and out.is_cuda and torch.isfinite(out).all()
    # a width without kernels, a state of another width than the network's, a scheduled step size, conditioning: eager with the opt-in
    odd = ta.UnderdampedLangevin(ta.MLPEnergy(8, 96, device=dev), step_size=0.1, device=dev)
    odd.fused_mlp = True
    assert odd._route(torch.zeros(4, 8, device=dev))[0] == "eager"
    plain.fused_mlp = True
    assert plain._route(x0)[0] == "fused_mlp" and plain._route(torch.zeros(4, 7, device=dev))[0] == "eager"
    assert plain._route(x0, {"label": 1})[0] == "eager" and plain._route(x0.double())[0] == "eager"
    sched = ta.UnderdampedLangevin(ta.MLPEnergy(6, 64, device=dev), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10), device=dev)
    sched.fused_mlp = True
    assert sched._route(x0)[0] == "eager"
    assert hip_calls(ENTRY) == before


@pytest.mark.parametrize("persistent", [False, True], ids=["cd_k", "persistent"])
def test_contrastive_divergence_makes_one_launch_per_call(cuda_device, persistent):
    dev = cuda_device
    torch.manual_seed(6)
    model = ta.MLPEnergy(2, 64, device=dev)
    sampler = ta.UnderdampedLangevin(model, step_size=0.1, friction=1.0, temperature=1.0, device=dev)
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
    """The confining 2-D network of test_ais_mlp_gpu.py, n = 4096, h = 0.3, gamma = 1, T = 1, 300 steps, seed 0, on the fused-MLP
    route and on the CPU eager route: the mean energy of the final positions and the kinetic temperature differ by at most 4.5
    standard errors of the difference (from the chains' sample variances).  Both routes carry the same step-size bias."""
    from test_ais_mlp_gpu import _confining_net

    cpu = _confining_net()
    referee = copy.deepcopy(cpu).double()
    n, dim, k = 4096, 2, 300
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(0))
    stats = {}
    for dev in (cuda_device, torch.device("cpu")):
        model = copy.deepcopy(cpu).to(dev)
        s = ta.UnderdampedLangevin(model, step_size=0.3, friction=1.0, temperature=1.0, device=dev)
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
        stats[dev.type] = {"e": (e.mean().item(), e.std().item() / math.sqrt(n)), "kt": (kt.mean().item(), kt.std().item() / math.sqrt(n))}
    for key in ("e", "kt"):
        (m1, se1), (m2, se2) = stats["cuda"][key], stats["cpu"][key]
        z = (m1 - m2) / math.sqrt(se1**2 + se2**2)
        print(f"{key}: fused-MLP route {m1:.4f} +- {se1:.4f}, CPU eager route {m2:.4f} +- {se2:.4f}, z = {z:+.2f}")
    for key in ("e", "kt"):
        (m1, se1), (m2, se2) = stats["cuda"][key], stats["cpu"][key]
        assert abs(m1 - m2) <= 4.5 * math.sqrt(se1**2 + se2**2), (key, stats)
