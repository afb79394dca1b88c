"""The BAOAB kernel of ``MLP3Energy`` at hidden width 64 against ``kinetic_cases.restate`` on the fp32 and fp64 networks."""

import copy
import functools
import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng

from helpers import hip_calls
from kinetic_cases import constants, restate
from test_mlp3_hmc_gpu import _Net, _spec, _within

pytestmark = pytest.mark.gpu

ENTRY = "ebm_kinetic_chain_mlp3_f32"
H, GAMMA, TEMP = 0.2, 1.5, 0.8
SHAPES = [(2, 129), (33, 37), (128, 129)]


@functools.lru_cache(maxsize=None)
def _case(dim, n, k, thin):  # (one case: computed once, shared, never modified)
    torch.manual_seed(10 + dim)
    cpu = ta.MLP3Energy(dim, 64)
    cpu.load_state_dict({name: 1.2 * t for name, t in cpu.state_dict().items()})  # every parameter x 1.2
    g = torch.Generator().manual_seed(7000 + dim + n)
    x0, v0, noise = torch.randn(n, dim, generator=g), math.sqrt(TEMP) * torch.randn(n, dim, generator=g), torch.randn(k, n, dim, generator=g)
    ref32 = restate(_Net(cpu.net), x0, v0, noise, H, GAMMA, TEMP, thin)
    ref64 = restate(_Net(copy.deepcopy(cpu.net).double()), x0, v0, noise, H, GAMMA, TEMP, thin, torch.float64)
    return dict(cpu=cpu, x0=x0, v0=v0, noise=noise, ref32=ref32, ref64=ref64)


def _run(spec, dev, x0, v0, k, thin, noise=None, traj=True, seed=0, off=0):  # -> x, v, traj: over-allocated, NaN where not written
    n, dim = x0.shape
    x, v = (torch.full((n + 3, dim), float("nan"), device=dev) for _ in range(2))
    x[:n] = x0.to(dev)
    if v0 is not None:
        v[:n] = v0.to(dev)
    tr = torch.full((n + 3, k // thin, dim), float("nan"), device=dev) if traj else None
    nz = None if noise is None else noise.to(dev)
    _lib.call(ENTRY, spec.to_c(), x.data_ptr(), v.data_ptr(), n, dim, k, H, GAMMA, TEMP, int(v0 is None), thin, _lib.ptr(tr),
              _lib.ptr(nz), seed, off, _lib.stream_handle(dev))
    return x.cpu(), v.cpu(), None if tr is None else tr.cpu()


@pytest.mark.parametrize("dim,n,k,thin", [(2, 129, 11, 3), (1, 37, 4, 2), (32, 37, 4, 2), (33, 37, 4, 2), (64, 129, 1, 1),
                                          (65, 37, 4, 2), (128, 129, 11, 3)])
def test_against_fp64_with_injected_noise(cuda_device, dim, n, k, thin):
    c = _case(dim, n, k, thin)
    got = _run(_spec(c, cuda_device)[1], cuda_device, c["x0"], c["v0"], k, thin, c["noise"])
    for name, t in zip(("x", "v", "traj"), got):  # rows past n keep the sentinel, every row below is written
        assert torch.isnan(t[n:]).all() and torch.isfinite(t[:n]).all() and t[:n].shape == c["ref64"][name].shape
        _within(t[:n], c["ref32"][name], c["ref64"][name])


@pytest.mark.parametrize("dim,n", SHAPES)
def test_fields_cuts_and_the_sampler(cuda_device, dim, n):
    dev, c = cuda_device, _case(dim, n, 4, 2)
    spec, seed, off = _spec(c, dev)[1], 0x1234567890ABCDEF, 11

    def field(step):  # the library's normal field at `step`
        out = torch.empty((n * dim + 3) // 4 * 4, device=dev)
        _lib.call("ebm_noise_fill_f32", out.data_ptr(), n * dim, _lib.NOISE_NORMAL, seed, step, _lib.stream_handle(dev))
        return out[: n * dim].view(n, dim).cpu()

    v0, noise = constants(H, GAMMA, TEMP)[3] * field(off), torch.stack([field(off + 1 + s) for s in range(4)])
    native = _run(spec, dev, c["x0"], None, 4, 2, seed=seed, off=off)
    fed = _run(spec, dev, c["x0"], v0, 4, 2, noise)
    assert all(torch.equal(a[:n], b[:n]) for a, b in zip(native, fed))
    x3, v3, none = _run(spec, dev, c["x0"], None, 3, 1, traj=False, seed=seed, off=off)  # 3 + 1 steps, no trajectory: the call of 4
    x4, v4, _ = _run(spec, dev, x3[:n], v3[:n], 1, 1, traj=False, seed=seed, off=off + 3)
    assert none is None and torch.equal(x4[:n], native[0][:n]) and torch.equal(v4[:n], native[1][:n])

    model, src = _spec(c, dev)[0], c["x0"].to(dev)  # ---- the sampler: ONE library call, this entry
    gen = lambda: torch.Generator(device=dev).manual_seed(5)  # noqa: E731

    def make(m=model, h=H, opt_in=True, **kw):
        s = ta.UnderdampedLangevin(m, step_size=h, friction=GAMMA, temperature=TEMP, device=dev, **kw)
        s.fused_mlp = opt_in
        return s

    s, g, total, c0 = make(), gen(), sum(_lib.call_counts.values()), hip_calls(ENTRY)
    x, v = s.sample(x=src, n_steps=4, return_velocity=True, generator=g)
    assert sum(_lib.call_counts.values()) == total + 1 and hip_calls(ENTRY) == c0 + 1 and _rng._get_offset(g) == 4 * 5
    assert torch.equal(src.cpu(), c["x0"]) and x.shape == v.shape == (n, dim) and torch.isfinite(x).all()
    g = gen()  # cut in two: the second call continues from the returned velocity at the Philox step the first one stopped at
    xa, va = s.sample(x=src, n_steps=3, return_velocity=True, generator=g)
    _rng._set_offset(g, 4 * 3)
    keep = (xa.clone(), va.clone())
    xb, vb = s.sample(x=xa, n_steps=1, velocity=va, return_velocity=True, generator=g)
    assert torch.equal(xb, x) and torch.equal(vb, v) and torch.equal(xa, keep[0]) and torch.equal(va, keep[1])
    traj, diag = s.sample(x=src, n_steps=4, thin=2, return_trajectory=True, return_diagnostics=True, generator=gen())
    assert traj.shape == (n, 2, dim) and torch.equal(traj[:, -1], x) and diag["mean"].shape == diag["var"].shape == (2, dim)
    assert diag["energy"].shape == (2,) and diag["kinetic_temperature"].shape == () and torch.isfinite(diag["energy"]).all()
    c0 = hip_calls(ENTRY)  # ... and what keeps its route
    assert s._route(src)[0] == "fused_mlp3"
    for other in (make(opt_in=False), make(mass=2.0), make(h=ta.core.schedules.LinearScheduler(0.3, 0.1, 10)),
                  make(_spec(c, dev, hidden=128)[0])):
        assert other._route(src)[0] == "eager" and other.sample(x=src, n_steps=2, generator=gen()).shape == (n, dim)
    s.sample_moments(x=src, n_steps=4, generator=gen())
    assert hip_calls(ENTRY) == c0


@pytest.mark.parametrize("persistent", [False, True], ids=["cd_k", "persistent"])
def test_contrastive_divergence_makes_one_launch_per_call(cuda_device, persistent):
    dev, model = cuda_device, ta.MLP3Energy(2, 64, device=cuda_device)
    sampler = ta.UnderdampedLangevin(model, step_size=0.1, device=dev)
    sampler.fused_mlp = True
    cd = ta.losses.ContrastiveDivergence(model=model, sampler=sampler, k_steps=5, persistent=persistent, buffer_size=512, init_steps=0,
                                         device=dev)
    data, g = torch.randn(256, 2, device=dev), torch.Generator(device=dev).manual_seed(7)
    for _ in range(2):
        before = hip_calls(ENTRY)
        loss, negatives = cd(data, generator=g)
        assert hip_calls(ENTRY) == before + 1 and torch.isfinite(loss) and torch.isfinite(negatives).all()
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


@pytest.mark.parametrize("n", [4, 0])
@pytest.mark.parametrize("change,code", [
    (dict(kind=4), -2), (dict(hidden=128), -3), (dict(dim=129), -3), (dict(dim=0), -3), (dict(energy=0), -1), (dict(dev0=0), -1),
    (dict(x=0), -1), (dict(v=0), -1), (dict(n=-1), -1), (dict(k=0), -1), (dict(thin=0), -1), (dict(h=0.0), -1),
    (dict(h=math.inf), -1), (dict(gamma=-1.0), -1), (dict(gamma=math.nan), -1), (dict(temp=0.0), -1), (dict(temp=math.inf), -1),
    (dict(x=4), -1), (dict(v=4), -1), (dict(traj=4), -1), (dict(noise=4), -1)])
def test_refusals_launch_nothing(cuda_device, n, change, code):  # (before any device access and before the early return, n = 0)
    a = {**dict(kind=_lib.ENERGY_MLP3, hidden=64, dim=8, n=n, k=1, thin=1, h=0.1, gamma=1.0, temp=1.0), **change}
    x, v, buf = torch.zeros(4, 129, device=cuda_device), torch.zeros(4, 129, device=cuda_device), torch.zeros(64, device=cuda_device)
    at = lambda k, base, default: ((base + a[k]) if a[k] else None) if k in a else default  # noqa: E731  (0: NULL, 4: misaligned)
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = a["kind"], a["hidden"], at("dev0", buf.data_ptr(), buf.data_ptr())
    rc = _lib.lib().ebm_kinetic_chain_mlp3_f32(
        at("energy", 0, desc), at("x", x.data_ptr(), x.data_ptr()), at("v", v.data_ptr(), v.data_ptr()), a["n"], a["dim"], a["k"],
        a["h"], a["gamma"], a["temp"], 0, a["thin"], at("traj", buf.data_ptr(), None), at("noise", buf.data_ptr(), None), 0, 0,
        _lib.stream_handle(cuda_device))
    assert rc == code and not x.any() and not v.any()
