"""ebm_kinetic_moments_mlp_f32 on the GPU: the kernels through the C ABI with injected draws -- the accumulators against the fp32
recurrences on the entry's own trajectories bit for bit, the walk against the plain MLP entries bit for bit and against the fp64
restatements of kinetic_moments_mlp_cases.py --, what a call writes and what it does not, its native draws against the
materialised Philox fields, a sub-block of chains, a wild start, the counters, the refusals with real buffers,
UnderdampedLangevin / GeneralizedHMC.sample_moments() with both opt-ins, and the law of a confining 2-D network against the CPU
eager route."""

import copy
import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls
from kinetic_moments_mlp_cases import (BAOAB_CASES, EPS, GAMMA, GHMC_CASES, STEP, TEMP, baoab_case, ghmc_case, moments_of, recip_table)
from kinetic_mlp_cases import constants as baoab_constants
from kinetic_mlp_cases import net as flat_net
from ghmc_mlp_cases import constants as ghmc_constants
from ghmc_mlp_cases import net as sharp_net

pytestmark = pytest.mark.gpu
ENTRY = "ebm_kinetic_moments_mlp_f32"
PLAIN_BAOAB, PLAIN_GHMC = "ebm_kinetic_mlp_chain_f32", "ebm_ghmc_mlp_chain_f32"
BAOAB, GHMC = 0, 1
FILL = 7.0
MASK_FILL = 9
GUARD = 64  # elements behind every buffer that must keep their fill


def _guarded(dev, shape, src=None, dtype=torch.float32, fill=FILL, guard=None):
    """A tensor of `shape` holding `fill` (or `src`) in front of GUARD elements of `guard` (default: the fill, FILL where the fill
    is NaN), in one allocation -> (tensor, guard elements, guard value)."""
    numel = 1
    for s in shape:
        numel *= s
    if guard is None:
        guard = fill if fill == fill else FILL
    buf = torch.full((numel + GUARD,), guard, device=dev, dtype=dtype)
    t = buf[:numel].view(shape)
    t.fill_(fill)
    if src is not None:
        t.copy_(src)
    return t, buf[numel:], guard


def _spec(dev, cpu_model):
    spec = copy.deepcopy(cpu_model).to(dev).fused_spec()
    assert spec is not None
    return spec


def run_entry(dev, cpu_model, sampler, x0, v0, k, burn_in, step, *, L=0, gamma=GAMMA, temp=TEMP, noise=None, u=None, trajs=True,
              energy=True, v2=True, mask=True, counts=None, prefill=FILL, seed=0, offset=0):
    """One call of the entry -> dict of CPU tensors: x, v [n, dim], mom [4, n, dim], e_mom [4, n], v2_mom [2, n, dim] (BAOAB),
    traj / v_traj [n, 2 h, dim], e_traj [n, 2 h], accepted [k, n] (bool), counts [k].  v0 None: draw_v0 = 1 and v starts from FILL.
    Every buffer starts from a fill and sits in front of a guard: a slot the call did not write keeps it, and so must the guards.
    `prefill`: what mom, e_mom and v2_mom hold before the call (the contract: never read at c == 1)."""
    n, dim = x0.shape
    h = (k - burn_in) // 2
    ghmc = sampler == GHMC
    spec = _spec(dev, cpu_model)
    recip = recip_table(h).to(dev)
    bufs = {"x": _guarded(dev, (n, dim), x0), "v": _guarded(dev, (n, dim), v0), "mom": _guarded(dev, (4, n, dim), fill=prefill)}
    if energy:
        bufs["e_mom"] = _guarded(dev, (4, n), fill=prefill)
    if v2 and not ghmc:
        bufs["v2_mom"] = _guarded(dev, (2, n, dim), fill=prefill)
    if trajs:
        bufs["traj"] = _guarded(dev, (n, 2 * h, dim))
        bufs["e_traj"] = _guarded(dev, (n, 2 * h))
        if not ghmc:
            bufs["v_traj"] = _guarded(dev, (n, 2 * h, dim))
    if mask and ghmc:
        bufs["mask"] = _guarded(dev, (k, n), dtype=torch.uint8, fill=MASK_FILL)
    if counts is not None:
        bufs["counts"] = _guarded(dev, (k,), counts, dtype=torch.int32, fill=0, guard=77)
    p = lambda key: _lib.ptr(bufs[key][0]) if key in bufs else None  # noqa: E731
    z_d = None if noise is None else noise.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, spec.to_c(), p("x"), p("v"), n, dim, sampler, k, burn_in, L, step, gamma, temp, int(v0 is None), _lib.ptr(recip),
              p("mom"), p("e_mom"), p("v2_mom"), p("traj"), p("e_traj"), p("v_traj"), p("mask"), p("counts"), _lib.ptr(z_d),
              _lib.ptr(u_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    for key, (_, guard, guard_fill) in bufs.items():
        assert bool((guard == guard_fill).all()), f"the call wrote behind {key}"
    out = {key: t.cpu() for key, (t, _, _) in bufs.items()}
    if "mask" in out:
        assert bool((out["mask"] <= 1).all()), "a slot of the accept mask was not written"
        out["accepted"] = out.pop("mask").bool()
    return out


def run_plain(dev, cpu_model, sampler, x0, v0, k, step, *, L=0, gamma=GAMMA, temp=TEMP, noise=None, u=None, seed=0, offset=0):
    """The plain MLP entry of the sampler on the same inputs -> x, v (and accepted)."""
    n, dim = x0.shape
    spec = _spec(dev, cpu_model)
    x = x0.to(dev).contiguous().clone()
    v = torch.full((n, dim), FILL, device=dev) if v0 is None else v0.to(dev).contiguous().clone()
    z_d = None if noise is None else noise.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    out = {}
    if sampler == BAOAB:
        _lib.call(PLAIN_BAOAB, spec.to_c(), x.data_ptr(), v.data_ptr(), n, dim, k, step, gamma, temp, int(v0 is None), 1, None,
                  _lib.ptr(z_d), seed, offset, _lib.stream_handle(dev))
    else:
        mk = torch.full((k, n), MASK_FILL, dtype=torch.uint8, device=dev)
        _lib.call(PLAIN_GHMC, spec.to_c(), x.data_ptr(), v.data_ptr(), n, dim, k, L, step, gamma, temp, int(v0 is None), 1, None,
                  mk.data_ptr(), _lib.ptr(z_d), _lib.ptr(u_d), seed, offset, _lib.stream_handle(dev))
        out["accepted"] = mk.cpu().bool()
    torch.cuda.synchronize()
    out.update(x=x.cpu(), v=v.cpu())
    return out


def _check_accumulators(got, h, ghmc):
    """mom, e_mom and v2_mom are the fp32 recurrences of the contract on the entry's OWN trajectories, bit for bit."""
    mom, e_mom, v2 = moments_of(got["traj"], got["e_traj"], None if ghmc else got["v_traj"], h)
    assert torch.equal(got["mom"], mom), "mom"
    assert torch.equal(got["e_mom"], e_mom), "e_mom"
    if not ghmc:
        assert torch.equal(got["v2_mom"], v2), "v2_mom"


def _check_variants(dev, run, got, ghmc):
    """A call with the three trajectory pointers NULL, and one whose accumulator planes hold NaN before the call, return the same
    x, v, mom, e_mom and v2_mom."""
    keys = ("x", "v", "mom", "e_mom") + (() if ghmc else ("v2_mom",))
    lean = run(trajs=False)
    assert "traj" not in lean and "e_traj" not in lean and "v_traj" not in lean
    poisoned = run(prefill=float("nan"))
    for key in keys:
        assert torch.equal(lean[key], got[key]), ("no trajectories", key)
        assert torch.equal(poisoned[key], got[key]), ("NaN pre-fill", key)
    for key in ("traj", "e_traj") + (() if ghmc else ("v_traj",)):
        assert torch.equal(poisoned[key], got[key]), ("NaN pre-fill", key)


def _check_against_fp64(tag, got, c, keys):
    """No further from fp64 than max(4 x the fp32 restatement's own max error, 4e-6 x max |ref|): the bar of the plain MLP tests."""
    figures = {}
    for key in keys:
        ref = c["ref64"][key]
        err_hip = (got[key].double() - ref).abs().max().item()
        err_torch = (c["ref32"][key].double() - ref).abs().max().item()
        figures[key] = (err_hip, err_torch, ref.abs().max().item())
        print(f"{tag}: {key} kernel err {err_hip:.3e}, fp32 restatement err {err_torch:.3e} ({err_hip / max(err_torch, 1e-30):.2f} x), "
              f"max|ref| {figures[key][2]:.3e}")
    for key, (err_hip, err_torch, scale) in figures.items():
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
        assert err_hip <= max(4.0 * err_torch, 4e-6 * scale), (key, err_hip, err_torch, scale)


# ---------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,n,k,burn_in", BAOAB_CASES)
def test_baoab_cases_with_injected_draws(cuda_device, in_dim, hidden, n, k, burn_in):
    """Measured on an MI355X (kernel error / fp32 restatement error per case): docs/design/kinetic_moments_mlp.md."""
    dev, c = cuda_device, baoab_case(in_dim, hidden, n, k, burn_in)
    h = c["half"]
    run = lambda **kw: run_entry(dev, c["cpu"], BAOAB, c["x0"], c["v0"], k, burn_in, STEP, noise=c["noise"], **kw)  # noqa: E731
    got = run()
    assert got["traj"].shape == got["v_traj"].shape == (n, 2 * h, in_dim) and got["e_traj"].shape == (n, 2 * h)
    for key in ("x", "v", "mom", "e_mom", "v2_mom", "traj", "e_traj", "v_traj"):
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
    _check_accumulators(got, h, False)
    _check_variants(dev, run, got, False)
    plain = run_plain(dev, c["cpu"], BAOAB, c["x0"], c["v0"], k, STEP, noise=c["noise"])
    assert torch.equal(got["x"], plain["x"]) and torch.equal(got["v"], plain["v"]), "the walk is not the plain entry's"
    assert torch.equal(got["traj"][:, -1], got["x"]) and torch.equal(got["v_traj"][:, -1], got["v"])
    _check_against_fp64(f"baoab dim {in_dim} H {hidden} n {n} k {k} burn_in {burn_in}", got, c, ("x", "v", "traj", "v_traj", "e_traj"))


@pytest.mark.parametrize("in_dim,hidden,n,k,burn_in,L", GHMC_CASES)
def test_ghmc_cases_with_injected_draws(cuda_device, in_dim, hidden, n, k, burn_in, L, gamma=GAMMA):
    """Measured on an MI355X (kernel error / fp32 restatement error per case): docs/design/kinetic_moments_mlp.md."""
    dev, c = cuda_device, ghmc_case(in_dim, hidden, n, k, burn_in, L, gamma)
    h = c["half"]
    run = lambda **kw: run_entry(dev, c["cpu"], GHMC, c["x0"], c["v0"], k, burn_in, c["eps"], L=L, gamma=gamma, noise=c["z"],  # noqa: E731
                                 u=c["u"], **kw)
    got = run()
    assert got["traj"].shape == (n, 2 * h, in_dim) and got["e_traj"].shape == (n, 2 * h) and got["accepted"].shape == (k, n)
    for key in ("x", "v", "mom", "e_mom", "traj", "e_traj"):
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
    _check_accumulators(got, h, True)
    _check_variants(dev, run, got, True)
    plain = run_plain(dev, c["cpu"], GHMC, c["x0"], c["v0"], k, c["eps"], L=L, gamma=gamma, noise=c["z"], u=c["u"])
    assert torch.equal(got["x"], plain["x"]) and torch.equal(got["v"], plain["v"]), "the walk is not the plain entry's"
    assert torch.equal(got["accepted"], plain["accepted"])
    assert torch.equal(got["traj"][:, -1], got["x"])
    wrong = int((got["accepted"] != c["ref64"]["accepted"]).sum())
    print(f"ghmc dim {in_dim} H {hidden} n {n} k {k} burn_in {burn_in} L {L} gamma {gamma}: decisions that differ from fp64: {wrong} of "
          f"{c['ref64']['accepted'].numel()}")
    assert wrong == 0
    _check_against_fp64(f"ghmc dim {in_dim} H {hidden} n {n} k {k} burn_in {burn_in} L {L} gamma {gamma}", got, c,
                        ("x", "v", "traj", "e_traj"))


@pytest.mark.parametrize("sampler", [BAOAB, GHMC], ids=["baoab", "ghmc"])
def test_a_call_without_energies_and_a_drawn_start(cuda_device, sampler):
    dev = cuda_device
    if sampler == BAOAB:
        c = baoab_case(5, 128, 37, 11, 3)
        kw = dict(noise=c["noise"])
        args = (c["cpu"], BAOAB, c["x0"], c["v0"], 11, 3, STEP)
    else:
        c = ghmc_case(100, 64, 129, 4, 0, 3)
        kw = dict(L=3, noise=c["z"], u=c["u"])
        args = (c["cpu"], GHMC, c["x0"], c["v0"], 4, 0, c["eps"])
    got = run_entry(dev, *args, **kw)
    bare = run_entry(dev, *args, energy=False, v2=False, trajs=False, mask=False, **kw)
    assert set(bare) == {"x", "v", "mom"}
    for key in bare:
        assert torch.equal(bare[key], got[key]), key
    # draw_v0: v is output only, every row written
    drawn = run_entry(dev, args[0], sampler, args[2], None, *args[4:], seed=3, offset=9, **kw)
    assert not bool((drawn["v"] == FILL).any()) and torch.isfinite(drawn["v"]).all() and torch.isfinite(drawn["mom"]).all()


# ---------------------------------------------------------------------------------
# native draws
# ---------------------------------------------------------------------------------
def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


def _fields(dev, sampler, seed, offset, n, dim, k, sqrt_temp):
    """v0, z (and u) of a call at (seed, offset): step `offset` scaled by sqrt_temp; BAOAB: normals at offset + 1 + i; GHMC: normals
    at offset + 1 + 2 t, uniforms at offset + 2 + 2 t."""
    stride = 2 if sampler == GHMC else 1
    v0 = (sqrt_temp * _field(dev, _lib.NOISE_NORMAL, seed, offset, n * dim)).view(n, dim).cpu()
    z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + stride * t, n * dim) for t in range(k)]).view(k, n, dim).cpu()
    u = None
    if sampler == GHMC:
        u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, offset + 2 + 2 * t, n) for t in range(k)]).view(k, n).cpu()
    return v0, z, u


@pytest.mark.parametrize("sampler", [BAOAB, GHMC], ids=["baoab", "ghmc"])
@pytest.mark.parametrize("in_dim,hidden,n", [(5, 64, 37), (33, 128, 70), (40, 128, 37), (128, 64, 70)])
def test_native_draws_are_the_materialised_fields(cuda_device, sampler, in_dim, hidden, n):
    """Per-element dims (5, 33) and per-quad ones (40, 128); then a sub-block of chains run alone reproduces its rows."""
    dev, (k, burn_in, L) = cuda_device, (7, 1, 2)
    ghmc = sampler == GHMC
    cpu = sharp_net(in_dim, hidden) if ghmc else flat_net(in_dim, hidden)
    step = EPS if ghmc else STEP
    sqrt_temp = ghmc_constants(step, L, GAMMA, TEMP)[2] if ghmc else baoab_constants(step, GAMMA, TEMP)[3]
    x0 = torch.randn(n, in_dim, generator=torch.Generator().manual_seed(5))
    seed, offset = 0x1234567887654321, 77
    v0, z, u = _fields(dev, sampler, seed, offset, n, in_dim, k, sqrt_temp)
    native = run_entry(dev, cpu, sampler, x0, None, k, burn_in, step, L=L, seed=seed, offset=offset)
    fed = run_entry(dev, cpu, sampler, x0, v0, k, burn_in, step, L=L, noise=z, u=u)
    for key in fed:
        assert torch.equal(native[key], fed[key]), key
    assert all(torch.isfinite(native[key]).all() for key in native if key != "accepted")
    if ghmc:
        assert native["accepted"].any() and (~native["accepted"]).any()  # both branches ran
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part = run_entry(dev, cpu, sampler, x0[lo:hi], v0[lo:hi], k, burn_in, step, L=L, noise=z[:, lo:hi], u=None if u is None else u[:, lo:hi])
    for key in ("x", "v", "traj", "e_traj"):
        assert torch.equal(part[key], fed[key][lo:hi]), key
    for key in ("mom", "e_mom") + (() if ghmc else ("v2_mom",)):
        assert torch.equal(part[key], fed[key][:, lo:hi]), key
    if ghmc:
        assert torch.equal(part["accepted"], fed["accepted"][:, lo:hi])


# ---------------------------------------------------------------------------------
# non-finite inputs, the counters
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,shape", [(BAOAB, (5, 128, 37, 11, 3)), (BAOAB, (32, 64, 129, 7, 3)), (GHMC, (5, 128, 37, 4, 0, 1)),
                                           (GHMC, (32, 64, 129, 6, 2, 1)), (GHMC, (33, 128, 37, 4, 0, 3))])
def test_wild_start_stays_in_its_chain(cuda_device, sampler, shape):
    """A NaN coordinate in one chain and a 1e20 coordinate in another, both in the first wave: every other chain's outputs are
    bitwise the clean run's."""
    dev = cuda_device
    if sampler == BAOAB:
        c = baoab_case(*shape)
        run = lambda x0: run_entry(dev, c["cpu"], BAOAB, x0, c["v0"], shape[3], shape[4], STEP, noise=c["noise"])  # noqa: E731
    else:
        c = ghmc_case(*shape)
        run = lambda x0: run_entry(dev, c["cpu"], GHMC, x0, c["v0"], shape[3], shape[4], c["eps"], L=shape[5], noise=c["z"],  # noqa: E731
                                   u=c["u"])
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    got, clean = run(x0), run(c["x0"])
    others = [i for i in range(shape[2]) if i not in (3, 7)]
    for key in ("x", "v", "traj", "e_traj") + (("v_traj",) if sampler == BAOAB else ()):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][others], clean[key][others]), key
    for key in ("mom", "e_mom") + (("v2_mom",) if sampler == BAOAB else ()):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][:, others], clean[key][:, others]), key
    if sampler == GHMC:
        assert torch.equal(got["accepted"][:, others], clean["accepted"][:, others])


def test_accept_count_adds_to_what_it_held(cuda_device):
    c = ghmc_case(30, 128, 257, 7, 3, 3)
    held = torch.arange(7, dtype=torch.int32) * 1000 + 5
    got = run_entry(cuda_device, c["cpu"], GHMC, c["x0"], c["v0"], 7, 3, c["eps"], L=3, noise=c["z"], u=c["u"], counts=held)
    assert torch.equal(got["counts"].long(), held.long() + got["accepted"].sum(dim=1))
    assert torch.equal(got["accepted"], c["ref64"]["accepted"])
    only = run_entry(cuda_device, c["cpu"], GHMC, c["x0"], c["v0"], 7, 3, c["eps"], L=3, noise=c["z"], u=c["u"], counts=held, mask=False)
    assert torch.equal(only["counts"], got["counts"]) and torch.equal(only["mom"], got["mom"])


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_kinetic_moments_mlp.py with real buffers: each raises its code and no buffer is touched."""
    from test_kinetic_moments_mlp import ANALYTIC, EINVAL, _abi_call

    dev, (n, dim) = cuda_device, (4, 8)
    names = ("x", "v", "recip", "mom", "v2_mom", "v_traj")
    bufs = {name: torch.full((4 * n * 132,), FILL, device=dev) for name in names}
    real = {name: bufs[name].data_ptr() for name in ("x", "v", "recip", "mom")}
    desc = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
    for kw, match in EINVAL:
        kw = {key: (bufs[key].data_ptr() if key in ("v2_mom", "v_traj") else val) for key, val in kw.items()}
        with pytest.raises(ValueError, match=match):
            _abi_call(desc, **{**real, **kw})
    with pytest.raises(ValueError, match="bad shape"):
        _abi_call(desc, n=-1, **real)
    for key in ("x", "v", "mom"):
        with pytest.raises(ValueError, match="16-byte aligned"):
            _abi_call(desc, **{**real, key: real[key] + 4})
    with pytest.raises(ValueError, match="energy descriptor is NULL"):
        _abi_call(None, **real)
    for sampler in (0, 1):
        with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
            _abi_call(ta.DoubleWellModel(device=dev).fused_spec().to_c(), sampler=sampler, **real)
        with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
            _abi_call(ta.GaussianModel(torch.zeros(dim), torch.eye(dim), device=dev).fused_spec().to_c(), sampler=sampler, **real)
        with pytest.raises(RuntimeError, match=r"code -2.*no running-moments kernel"):
            _abi_call(desc, entry=ANALYTIC, sampler=sampler, **real)
        with pytest.raises(RuntimeError, match=r"code -3.*got 64, 129"):
            _abi_call(desc, dim=129, sampler=sampler, **real)
        with pytest.raises(RuntimeError, match=r"code -3.*got 64, 0"):
            _abi_call(desc, dim=0, sampler=sampler, **real)
        wide = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
        wide.n_comp = 96
        with pytest.raises(RuntimeError, match=r"code -3.*got 96, 8"):
            _abi_call(wide, sampler=sampler, **real)
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == FILL).all()), name


# ---------------------------------------------------------------------------------
# through the samplers
# ---------------------------------------------------------------------------------
def _sampler(which, model, dev, friction=GAMMA):
    if which == "baoab":
        return ta.UnderdampedLangevin(model, step_size=STEP, friction=friction, temperature=TEMP, device=dev)
    return ta.GeneralizedHMC(model, step_size=EPS, n_leapfrog_steps=2, friction=friction, temperature=TEMP, device=dev)


@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_sample_moments_with_both_opt_ins_is_one_launch(cuda_device, which):
    dev, (n, dim, k, burn_in) = cuda_device, (300, 6, 11, 3)
    ghmc = which == "ghmc"
    cpu = sharp_net(dim, 64) if ghmc else flat_net(dim, 64)
    model = copy.deepcopy(cpu).to(dev)
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    s = _sampler(which, model, dev)
    s.fused_mlp = s.fused_mlp_moments = True
    assert s._route(x0)[0] == "fused_mlp"
    plain_entry = PLAIN_GHMC if ghmc else PLAIN_BAOAB
    g = torch.Generator(device=dev).manual_seed(5)
    before = hip_calls(ENTRY), hip_calls(plain_entry), hip_calls("ebm_kinetic_moments_f32")
    x, mom, v = s.sample_moments(x=x0, n_steps=k, burn_in=burn_in, energy=True, return_velocity=True, generator=g)
    torch.cuda.synchronize()
    assert (hip_calls(ENTRY), hip_calls(plain_entry), hip_calls("ebm_kinetic_moments_f32")) == (before[0] + 1, before[1], before[2])
    steps = (2 * k if ghmc else k) + 1
    assert _rng._get_offset(g) == 4 * steps  # as sample() advances it
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    assert x.is_cuda and v.is_cuda and x.shape == v.shape == (n, dim)
    # the states are sample()'s with fused_mlp for the same generator state, bit for bit
    g2 = torch.Generator(device=dev).manual_seed(5)
    xs, vs = s.sample(x=x0, n_steps=k, return_velocity=True, generator=g2)
    assert hip_calls(plain_entry) == before[1] + 1 and _rng._get_offset(g2) == 4 * steps
    assert torch.equal(x, xs) and torch.equal(v, vs)
    # the moments are the entry's at the generator's coordinates
    want = run_entry(dev, cpu, GHMC if ghmc else BAOAB, x0.cpu(), None, k, burn_in, EPS if ghmc else STEP, L=2,
                     seed=_rng.kernel_seed(5), offset=0)
    h = (k - burn_in) // 2
    assert mom.half_len == h and mom.n_nonfinite == 0
    assert torch.equal(mom.chain_mean.cpu(), want["mom"][[0, 2]]) and torch.equal(mom.chain_m2.cpu(), want["mom"][[1, 3]])
    assert torch.equal(mom.energy_mean.cpu(), want["e_mom"][[0, 2]]) and torch.equal(mom.energy_m2.cpu(), want["e_mom"][[1, 3]])
    assert torch.equal(x.cpu(), want["x"]) and torch.equal(v.cpu(), want["v"])
    if ghmc:
        rate = want["accepted"].float().mean(dim=1)
        assert torch.allclose(mom.acceptance_rate.cpu(), rate, rtol=1e-6, atol=0) and bool(((rate > 0) & (rate < 1)).all())
        assert mom.velocity_sq_mean is None
    else:
        assert torch.equal(mom.velocity_sq_mean.cpu(), want["v2_mom"]) and mom.acceptance_rate is None
    # a passed velocity is continued and never written
    v_keep = v.clone()
    xb, _, vb = s.sample_moments(x=x, n_steps=8, velocity=v, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(6))
    xc, vc = s.sample(x=x, n_steps=8, velocity=v, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(6))
    assert torch.equal(v, v_keep) and torch.equal(xb, xc) and torch.equal(vb, vc)


def test_generalized_hmc_at_infinite_friction(cuda_device):
    dev, (n, dim, k) = cuda_device, (200, 6, 8)
    s = _sampler("ghmc", copy.deepcopy(sharp_net(dim, 64)).to(dev), dev, friction=math.inf)
    s.fused_mlp = s.fused_mlp_moments = True
    x0 = torch.randn(n, dim, device=dev)
    before = hip_calls(ENTRY)
    x, mom, v = s.sample_moments(x=x0, n_steps=k, energy=True, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(2))
    assert hip_calls(ENTRY) == before + 1
    xs, vs = s.sample(x=x0, n_steps=k, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(2))
    assert torch.equal(x, xs) and torch.equal(v, vs)
    assert mom.n_nonfinite == 0 and torch.isfinite(mom.rhat).all() and 0.0 < float(mom.acceptance_rate.mean()) < 1.0


def test_the_counters_serve_beyond_the_mask_limit(cuda_device, monkeypatch):
    from torchebm_amd.samplers import kinetic_moments

    dev, (n, dim, k) = cuda_device, (300, 6, 8)
    s = _sampler("ghmc", copy.deepcopy(sharp_net(dim, 64)).to(dev), dev)
    s.fused_mlp = s.fused_mlp_moments = True
    x0 = torch.randn(n, dim, device=dev)
    _, by_mask = s.sample_moments(x=x0, n_steps=k, generator=torch.Generator(device=dev).manual_seed(2))
    monkeypatch.setattr(kinetic_moments, "MASK_MAX_BYTES", k * n - 1)
    before = hip_calls(ENTRY)
    _, by_count = s.sample_moments(x=x0, n_steps=k, generator=torch.Generator(device=dev).manual_seed(2))
    assert hip_calls(ENTRY) == before + 1
    assert torch.equal(by_mask.acceptance_rate, by_count.acceptance_rate) and torch.equal(by_mask.chain_mean, by_count.chain_mean)


@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_without_the_second_opt_in_or_off_its_shapes_the_entry_is_not_launched(cuda_device, which):
    dev = cuda_device
    before = hip_calls(ENTRY)
    torch.manual_seed(3)
    x0 = torch.randn(32, 6, device=dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(1)  # noqa: E731
    # fused_mlp alone: the step-by-step recurrence, as before
    s = _sampler(which, ta.MLPEnergy(6, 64, device=dev), dev)
    s.fused_mlp = True
    assert s._route(x0)[0] == "fused_mlp" and s.fused_mlp_moments is False
    x, mom = s.sample_moments(x=x0, n_steps=8, burn_in=2, generator=gen())
    assert x.shape == (32, 6) and torch.isfinite(mom.mean).all()
    # the second opt-in alone
    s = _sampler(which, ta.MLPEnergy(6, 64, device=dev), dev)
    s.fused_mlp_moments = True
    assert s._route(x0)[0] == "eager"
    s.sample_moments(x=x0, n_steps=4, generator=gen())
    # both, but a width without kernels / a scheduled step size
    s = _sampler(which, ta.MLPEnergy(6, 96, device=dev), dev)
    s.fused_mlp = s.fused_mlp_moments = True
    assert s._route(x0)[0] == "eager"
    s.sample_moments(x=x0, n_steps=4, generator=gen())
    cls = ta.UnderdampedLangevin if which == "baoab" else ta.GeneralizedHMC
    s = cls(ta.MLPEnergy(6, 64, device=dev), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10), device=dev)
    s.fused_mlp = s.fused_mlp_moments = True
    assert s._route(x0)[0] == "eager"
    s.sample_moments(x=x0, n_steps=4, generator=gen())
    # an analytic energy keeps its own one-launch route with both opt-ins set
    s = cls(ta.DoubleWellModel(device=dev), step_size=0.05, device=dev)
    s.fused_mlp = s.fused_mlp_moments = True
    analytic = hip_calls("ebm_kinetic_moments_f32")
    s.sample_moments(x=x0, n_steps=4, generator=gen())
    assert hip_calls("ebm_kinetic_moments_f32") == analytic + 1
    assert hip_calls(ENTRY) == before


# ---------------------------------------------------------------------------------
# the law
# ---------------------------------------------------------------------------------
def _per_chain(mom):
    """Per-chain contributions (float64, CPU) whose means over the chains are the pooled mean and (up to M l / (M l - 1)) the pooled
    variance of ChainMoments: their sample variances over the independent chains give the standard errors."""
    mean, m2 = mom.chain_mean.cpu().double(), mom.chain_m2.cpu().double()
    h = mom.half_len
    m_i = mean.mean(dim=0)  # [n, dim]
    grand = m_i.mean(dim=0)
    s_i = m2.sum(dim=0) / (2 * h) + ((mean - grand) ** 2).mean(dim=0)
    return m_i, s_i


@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_the_law_of_a_confining_network_is_the_eager_routes(cuda_device, which):
    """The confining 2-D network of test_ais_mlp_gpu.py, n = 4096, step 0.3 (generalized HMC: L = 2), gamma = 1, T = 1, 300
    transitions of which the first 100 are burnt, seed 0, on the one-launch route and on the CPU eager route: the pooled mean and
    variance of ChainMoments per coordinate (and BAOAB's kinetic_temperature) differ by at most 4.5 standard errors of the
    difference, the standard errors from the sample variances of the chains' own contributions."""
    from test_ais_mlp_gpu import _confining_net

    cpu = _confining_net()
    n, dim, k, burn_in = 4096, 2, 300, 100
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(0))
    stats = {}
    for dev in (cuda_device, torch.device("cpu")):
        model = copy.deepcopy(cpu).to(dev)
        if which == "baoab":
            s = ta.UnderdampedLangevin(model, step_size=0.3, friction=1.0, temperature=1.0, device=dev)
        else:
            s = ta.GeneralizedHMC(model, step_size=0.3, n_leapfrog_steps=2, friction=1.0, temperature=1.0, device=dev)
        s.fused_mlp = s.fused_mlp_moments = True
        before = hip_calls(ENTRY)
        _, mom = s.sample_moments(x=x0.to(dev), n_steps=k, burn_in=burn_in, generator=torch.Generator(device=dev).manual_seed(0))
        assert hip_calls(ENTRY) == before + (1 if dev.type == "cuda" else 0)
        assert mom.n_nonfinite == 0 and mom.half_len == 100
        m_i, s_i = _per_chain(mom)
        scale = 2 * n * 100 / (2 * n * 100 - 1.0)
        assert torch.allclose(m_i.mean(dim=0), mom.mean.cpu(), rtol=0, atol=1e-12)
        assert torch.allclose(scale * s_i.mean(dim=0), mom.var.cpu(), rtol=1e-9)
        st = {"mean": (mom.mean.cpu(), m_i.std(dim=0) / math.sqrt(n)), "var": (mom.var.cpu(), scale * s_i.std(dim=0) / math.sqrt(n))}
        if which == "baoab":
            kt_i = mom.velocity_sq_mean.cpu().double().mean(dim=0)
            assert torch.allclose(kt_i.mean(dim=0), mom.kinetic_temperature.cpu(), rtol=1e-12)
            st["kinetic_temperature"] = (mom.kinetic_temperature.cpu(), kt_i.std(dim=0) / math.sqrt(n))
        else:
            assert 0.0 < float(mom.acceptance_rate.mean()) < 1.0
        stats[dev.type] = st
    zs = {}
    for key in stats["cpu"]:
        (m1, se1), (m2, se2) = stats["cuda"][key], stats["cpu"][key]
        zs[key] = (m1 - m2) / torch.sqrt(se1**2 + se2**2)
        print(f"{which} {key}: one launch {m1.tolist()} +- {se1.tolist()}, CPU eager route {m2.tolist()} +- {se2.tolist()}, "
              f"z = {zs[key].tolist()}")
    for key, z in zs.items():
        assert bool((z.abs() <= 4.5).all()), (key, z.tolist())
