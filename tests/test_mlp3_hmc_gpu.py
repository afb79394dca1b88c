"""The HMC transition kernel of ``MLP3Energy`` at hidden width 64 against the fp32 and fp64 networks on the CPU driven through
``oracle.hmc.hmc_chain``: one, two and four state tiles, widths off multiples of 4, a tile edge, a partial wave, two workgroups."""

import copy
import functools

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from oracle.hmc import hmc_chain

from helpers import hip_calls

pytestmark = pytest.mark.gpu

ENTRY = "ebm_hmc_chain_mlp3_f32"
EPS = 0.125  # (exact in fp32: the fp64 reference walks with the same step size)


class _Net:  # what ``hmc_chain`` asks of an energy, from autograd
    def __init__(self, net):
        self.net = net

    def energy(self, x):
        return self.net(x).squeeze(-1).detach()

    def grad(self, x):
        x = x.detach().requires_grad_(True)
        return torch.autograd.grad(self.net(x).sum(), x)[0]


@functools.lru_cache(maxsize=None)
def _case(dim, n, n_mh, thin, leap, mass=None, scale=1.0, eps=(EPS,), random_u=False):
    torch.manual_seed(dim if random_u else 100 * dim + n + n_mh)  # (one case: computed once, shared, never modified)
    cpu = ta.MLP3Energy(dim, 64)
    with torch.no_grad():
        for q in cpu.parameters():
            q.mul_(scale)
    x, p = 2.0 * torch.randn(n, dim), torch.randn(n_mh, n, dim)
    if random_u:
        u = torch.rand(n_mh, n)
    else:  # u = 1 rejects at any a <= 1, u = 0 accepts at the clamped a >= e^-50: no decision can flip
        t, c = torch.meshgrid(torch.arange(n_mh), torch.arange(n), indexing="ij")
        u = ((t + c) % 3 == 0).float()
    table = [eps[t % len(eps)] for t in range(n_mh)]
    ref32 = hmc_chain(_Net(cpu.net), x, p, u, table, leap, mass, thin, want_traj=True)
    net64 = _Net(copy.deepcopy(cpu.net).double())
    ref64 = hmc_chain(net64, x.double(), p.double(), u.double(), table, leap, mass, thin, want_traj=True, want_margins=True)
    return dict(cpu=cpu, x=x, p=p, u=u, table=table, ref32=ref32, ref64=ref64)


def _spec(case, dev, hidden=64):
    model = ta.MLP3Energy(case["cpu"].in_dim, hidden, device=dev)
    if hidden == 64:
        model.load_state_dict(case["cpu"].state_dict())
    return model, model.fused_spec()


def _hmc(spec, x, n, n_mh, leap, dev, eps=EPS, mass=None, thin=1, seed=0, off=0, **bufs):  # bufs: table, traj, mask, count, p, u
    kind, m = (_lib.MASS_NONE, 1.0) if mass is None else (_lib.MASS_SCALAR, mass)
    table, traj, mask, count, p, u = (_lib.ptr(bufs.get(k)) for k in ("table", "traj", "mask", "count", "p", "u"))
    _lib.call(ENTRY, spec.to_c(), x.data_ptr(), n, x.shape[1], n_mh, leap, eps, table, kind, m, thin, traj, mask, count, p, u, seed, off,
              _lib.stream_handle(dev))


def _within(got, want32, want64):  # test_mlp3_gpu.py's bar: the worst error against fp64 <= 4 x torch's own fp32 run's
    err_hip, err_torch = (got.cpu().double() - want64).abs().max().item(), (want32.double() - want64).abs().max().item()
    scale = want64.abs().max().item()
    print(f"err_hip={err_hip:.3e} err_torch={err_torch:.3e} scale={scale:.3e}")
    assert err_hip <= max(4.0 * err_torch, 4e-6 * scale), (err_hip, err_torch, scale)


def _run_injected(case, dev, n_mh, thin, leap, mass=None):
    n, dim = case["x"].shape
    spec, x = _spec(case, dev)[1], torch.full((n + 3, dim), 7.0, device=dev)  # over-allocated: rows >= n are not the kernel's
    x[:n] = case["x"].to(dev)
    traj = torch.full((n, n_mh // thin, dim), float("nan"), device=dev)
    mask, count = torch.full((n_mh, n), 9, dtype=torch.uint8, device=dev), torch.zeros(n_mh, dtype=torch.int32, device=dev)
    table = torch.tensor(case["table"], device=dev) if len(set(case["table"])) > 1 else None
    _hmc(spec, x, n, n_mh, leap, dev, eps=case["table"][0], table=table, mass=mass, thin=thin, traj=traj, mask=mask, count=count,
         p=case["p"].to(dev), u=case["u"].to(dev))
    return x, traj, mask.cpu().bool(), count.cpu()


@pytest.mark.parametrize("dim,n,n_mh,thin,leap,mass,eps", [
    *[(d, n, *c, None, (EPS,)) for d in (2, 33, 128) for n in (37, 129) for c in ((4, 2, 3), (1, 1, 1))],
    (33, 37, 4, 2, 3, 2.5, (EPS, 0.0625))])  # ... and one case with a scalar mass and a step-size table of two values
def test_state_against_fp64_with_fixed_decisions(cuda_device, dim, n, n_mh, thin, leap, mass, eps):
    case = _case(dim, n, n_mh, thin, leap, mass, 1.0, eps)
    x, traj, mask, count = _run_injected(case, cuda_device, n_mh, thin, leap, mass)
    want = case["u"] == 0.0
    assert torch.equal(case["ref64"]["accepted"], want) and torch.equal(case["ref32"]["accepted"], want)
    assert torch.equal(mask, want) and torch.equal(count, want.sum(dim=1).int()) and torch.equal(x[n:].cpu(), torch.full((3, dim), 7.0))
    _within(x[:n], case["ref32"]["x"], case["ref64"]["x"])
    _within(traj, case["ref32"]["trajectory"], case["ref64"]["trajectory"])


@pytest.mark.parametrize("dim", [2, 128])
def test_acceptance_probability(cuda_device, dim):
    # one transition that rejects (eps 1.5, every parameter x 2.5): where fp64's a is > 1e-3 from u, the kernel decides as fp64 does
    n, case = 129, _case(dim, 129, 1, 1, 3, None, 2.5, (1.5,), True)
    ref = case["ref64"]
    clear, accepts = ref["margins"][0] > 1e-3, int(ref["accepted"].sum())
    assert int((~clear).sum()) <= 2 and accepts >= 10 and n - accepts >= 10
    _, _, mask, count = _run_injected(case, cuda_device, 1, 1, 3)
    assert torch.equal(mask[0][clear], ref["accepted"][0][clear]) and int(count[0]) == int(mask[0].sum())


def _fields(n, dim, n_mh, seed, off, dev):  # the library's normal field at steps off + 2 t, its uniform field at off + 2 t + 1
    ps, us = [torch.empty(n, dim, device=dev) for _ in range(n_mh)], [torch.empty(n, device=dev) for _ in range(n_mh)]
    for t in range(n_mh):
        _lib.call("ebm_noise_fill_f32", ps[t].data_ptr(), n * dim, _lib.NOISE_NORMAL, seed, off + 2 * t, _lib.stream_handle(dev))
        _lib.call("ebm_noise_fill_f32", us[t].data_ptr(), n, _lib.NOISE_UNIFORM, seed, off + 2 * t + 1, _lib.stream_handle(dev))
    return torch.stack(ps), torch.stack(us)


@pytest.mark.parametrize("dim,n", [(2, 129), (33, 37), (128, 129)])
def test_random_field_and_routes(cuda_device, dim, n):
    dev, case = cuda_device, _case(dim, n, 4, 2, 3)
    (model, spec), src = _spec(case, dev), case["x"].to(dev)
    seed, off, leap = 0x1234567890ABCDEF, 11, 3
    p, u = _fields(n, dim, 4, seed, off, dev)
    outs = []
    for kw in (dict(seed=seed, off=off), dict(p=p, u=u)):
        x, mask, traj = src.clone(), torch.zeros(4, n, dtype=torch.uint8, device=dev), torch.full((n, 2, dim), float("nan"), device=dev)
        count = torch.zeros(4, dtype=torch.int32, device=dev)
        _hmc(spec, x, n, 4, leap, dev, thin=2, mask=mask, count=count, traj=traj, **kw)
        outs.append((x, mask, count, traj))
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and torch.equal(outs[0][2], outs[0][1].sum(dim=1).int())
    halves = src.clone()
    _hmc(spec, halves, n, 3, leap, dev, seed=seed, off=off)
    _hmc(spec, halves, n, 1, leap, dev, seed=seed, off=off + 6)
    assert torch.equal(halves, outs[0][0])
    # the sampler: ONE library call, this entry, also with a thinned trajectory
    sampler = ta.HamiltonianMonteCarlo(model, step_size=EPS, n_leapfrog_steps=leap, device=dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(5)  # noqa: E731
    before, c0 = sum(_lib.call_counts.values()), hip_calls(ENTRY)
    got = sampler.sample(x=src, n_steps=4, generator=gen())
    assert sum(_lib.call_counts.values()) == before + 1 and hip_calls(ENTRY) == c0 + 1
    assert torch.equal(src.cpu(), case["x"]) and got.shape == (n, dim) and torch.isfinite(got).all()
    before = sum(_lib.call_counts.values())
    traj = sampler.sample(x=src, n_steps=4, thin=2, return_trajectory=True, generator=gen())
    assert sum(_lib.call_counts.values()) == before + 1 and traj.shape == (n, 2, dim) and torch.equal(traj[:, -1], got)
    # ... and what stays on the per-transition route
    c0 = hip_calls(ENTRY)
    sampler.sample(x=src, n_steps=2, return_diagnostics=True, generator=gen())
    ta.HamiltonianMonteCarlo(model, step_size=EPS, n_leapfrog_steps=leap, mass=torch.full((dim,), 2.0, device=dev),
                             device=dev).sample(x=src, n_steps=2, generator=gen())
    ta.HamiltonianMonteCarlo(_spec(case, dev, hidden=128)[0], step_size=EPS, n_leapfrog_steps=leap, device=dev).sample(
        x=src, n_steps=2, generator=gen())
    assert hip_calls(ENTRY) == c0


@pytest.mark.parametrize("change,code", [
    (dict(kind=4), -2), (dict(hidden=128), -3), (dict(dim=129), -3), (dict(dim=0), -3), (dict(energy=0), -1), (dict(dev0=0), -1),
    (dict(x=0), -1), (dict(n=-1), -1), (dict(n_mh=-1), -1), (dict(leap=0), -1), (dict(thin=0), -1), (dict(mass_kind=2), -1),
    (dict(x=4), -1), (dict(traj=4), -1), (dict(p=4), -1)])
def test_refusals_launch_nothing(cuda_device, change, code):
    # every refusal comes before any device access (the parameters are never read) and before the early return (n_mh = 0)
    a = {**dict(kind=_lib.ENERGY_MLP3, hidden=64, dim=8, n=4, n_mh=0, leap=1, thin=1, mass_kind=_lib.MASS_NONE), **change}
    x, buf = torch.zeros(4, 129, device=cuda_device), torch.zeros(64, device=cuda_device)
    # a pointer named in `change`: 0 is NULL, 4 is misaligned; otherwise x and dev0 are valid, traj and p_noise NULL
    at = lambda k, base, default: ((base + a[k]) if a[k] else None) if k in a else default  # noqa: E731
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = a["kind"], a["hidden"], at("dev0", buf.data_ptr(), buf.data_ptr())
    rc = _lib.lib().ebm_hmc_chain_mlp3_f32(
        at("energy", 0, desc), at("x", x.data_ptr(), x.data_ptr()), a["n"], a["dim"], a["n_mh"], a["leap"], 0.1, None, a["mass_kind"], 1.0,
        a["thin"], at("traj", buf.data_ptr(), None), None, None, at("p", buf.data_ptr(), None), None, 0, 0, _lib.stream_handle(cuda_device))
    assert rc == code and not x.any()
