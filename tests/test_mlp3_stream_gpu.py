"""The streamed bf16 kernel of the three-hidden-layer MLP energy at hidden width 128 (include/ebm_hip_mlp3_stream.h) against the
float64 network: both sides of every W1 piece and state-tile boundary, a width that is no multiple of 4, the opt-in range
(dim <= 32); a partial wave and more than one workgroup; K = 7 steps, so both buffer parities and the hand-over between
evaluations run.  The yardstick is tests/test_mlp3_gpu.py's: at most 4 x the error of torch's own fp32 network."""

import copy
import functools

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib

from helpers import hip_calls

pytestmark = pytest.mark.gpu

HIDDEN = 128
DIMS = [2, 32, 33, 64, 65, 97, 128]
NS = [37, 129]
K, ETA, COEF = 7, 0.05, 1.0
EVAL, CHAIN, IMAGE = "ebm_energy_grad_mlp3_stream_f32", "ebm_langevin_chain_mlp3_stream_f32", "ebm_mlp3_image_f32"


def _grad(net, x):
    x = x.clone().requires_grad_(True)
    e = net(x).squeeze(-1)
    (g,) = torch.autograd.grad(e.sum(), x)
    return e.detach(), g


def _em(x, g, z):  # the reference's update, every operation on its own
    return (x - ETA * g) + COEF * (z * ETA**0.5)


@functools.lru_cache(maxsize=None)
def _case(dim, n):
    """CPU model, inputs, noise and the fp32 / fp64 references of one shape -- computed once, shared, never modified."""
    torch.manual_seed(1000 * HIDDEN + 10 * dim + n)
    cpu = ta.MLP3Energy(dim, HIDDEN)
    net64 = copy.deepcopy(cpu.net).double()
    x = 2.0 * torch.randn(n, dim)
    noise = torch.randn(K, n, dim)
    x32, x64 = x, x.double()
    for i in range(K):
        x32 = _em(x32, _grad(cpu.net, x32)[1], noise[i])
        x64 = _em(x64, _grad(net64, x64)[1], noise[i].double())
    return dict(cpu=cpu, x=x, noise=noise, eval32=_grad(cpu.net, x), eval64=_grad(net64, x.double()), chain32=x32, chain64=x64)


def _gpu_model(case, dev, opt_in=True):
    model = ta.MLP3Energy(case["cpu"].in_dim, HIDDEN, device=dev)
    model.load_state_dict(case["cpu"].state_dict())
    model.streamed_bf16 = opt_in  # needed at dim <= 32 only
    return model


def _spec(case, dev):
    spec = _gpu_model(case, dev).fused_spec()
    assert spec is not None and spec.kind == _lib.ENERGY_MLP3 and spec.aux is not None  # the spec carries an image
    assert spec.aux.numel() * 4 == _lib.lib().ebm_mlp3_image_bytes(HIDDEN, case["cpu"].in_dim)
    return spec


def _within(got, want32, want64, floor):
    """The kernel's worst error against fp64 is at most 4 x that of torch's own fp32 network (`floor`: where torch's is ~0)."""
    err_hip = (got.cpu().double() - want64).abs().max().item()
    err_torch = (want32.double() - want64).abs().max().item()
    scale = want64.abs().max().item()
    print(f"err_hip={err_hip:.3e} err_torch={err_torch:.3e} scale={scale:.3e}")
    assert err_hip <= max(4.0 * err_torch, floor * scale), (err_hip, err_torch, scale)


def _field(n, dim, seed, step0, dev):
    """The library's normal field of `seed` at steps step0 .. step0 + K - 1, [K, n, dim] (each plane filled 16-byte aligned)."""
    planes = [torch.empty(n, dim, device=dev) for _ in range(K)]
    for i, plane in enumerate(planes):
        _lib.call("ebm_noise_fill_f32", plane.data_ptr(), n * dim, _lib.NOISE_NORMAL, seed, step0 + i, _lib.stream_handle(dev))
    return torch.stack(planes)


def _chain(spec, src, out, n, dim, k, noise, seed, offset, dev):
    _lib.call(CHAIN, spec.to_c(), src.data_ptr(), out.data_ptr(), n, dim, k, ETA, ETA**0.5, COEF, _lib.ptr(noise), seed, offset,
              _lib.stream_handle(dev))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dim", DIMS)
def test_evaluation_against_fp64(cuda_device, dim, n):
    case = _case(dim, n)
    spec = _spec(case, cuda_device)
    x = case["x"].to(cuda_device)
    outs = {}
    for want_e, want_g in ((True, True), (True, False), (False, True)):
        e = torch.full((n,), float("nan"), device=cuda_device) if want_e else None
        g = torch.full((n, dim), float("nan"), device=cuda_device) if want_g else None
        _lib.call(EVAL, spec.to_c(), x.data_ptr(), n, dim, _lib.ptr(e), _lib.ptr(g), _lib.stream_handle(cuda_device))
        outs[want_e, want_g] = (e, g)
    e, g = outs[True, True]
    _within(e, case["eval32"][0], case["eval64"][0], 2e-6)
    _within(g, case["eval32"][1], case["eval64"][1], 2e-6)
    assert torch.equal(outs[True, False][0], e)  # the forward pass alone
    assert torch.equal(outs[False, True][1], g)  # the gradient alone


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dim", DIMS)
def test_chain_against_the_fp64_chain(cuda_device, dim, n):
    case = _case(dim, n)
    spec = _spec(case, cuda_device)
    src, noise = case["x"].to(cuda_device), case["noise"].to(cuda_device)
    out = torch.full((n + 3, dim), 7.0, device=cuda_device)  # over-allocated: rows >= n are not the kernel's
    _chain(spec, src, out, n, dim, K, noise, 0, 0, cuda_device)
    _within(out[:n], case["chain32"], case["chain64"], 4e-6)
    assert torch.equal(out[n:].cpu(), torch.full((3, dim), 7.0)) and torch.equal(src.cpu(), case["x"])
    inplace = src.clone()
    _chain(spec, inplace, inplace, n, dim, K, noise, 0, 0, cuda_device)
    assert torch.equal(inplace, out[:n])


@pytest.mark.parametrize("dim,n", [(33, 37), (128, 129), (32, 129)])
def test_noise_field_and_sampler_routes(cuda_device, dim, n):
    case = _case(dim, n)
    model = _gpu_model(case, cuda_device)
    spec, src = _spec(case, cuda_device), case["x"].to(cuda_device)
    seed, off = 0x1234567890ABCDEF, 11
    field = _field(n, dim, seed, off, cuda_device)
    native, injected, halves = (torch.empty_like(src) for _ in range(3))
    _chain(spec, src, native, n, dim, K, None, seed, off, cuda_device)
    _chain(spec, src, injected, n, dim, K, field, 0, 0, cuda_device)
    assert torch.equal(native, injected)
    _chain(spec, src, halves, n, dim, 4, None, seed, off, cuda_device)
    _chain(spec, halves, halves, n, dim, 3, None, seed, off + 4, cuda_device)
    assert torch.equal(native, halves)
    # the sampler's plain call: one image and one streamed chain launch, nothing per step; gradient(): one image, one evaluation
    names = (IMAGE, CHAIN, EVAL, "ebm_langevin_chain_mlp3_f32", "ebm_energy_grad_mlp3_f32")
    sampler = ta.LangevinDynamics(model, step_size=ETA, noise_scale=(0.5 * COEF**2) ** 0.5, device=cuda_device)
    before, c0 = sum(_lib.call_counts.values()), [hip_calls(name) for name in names]
    got = sampler.sample(x=src, n_steps=K, generator=torch.Generator(device=cuda_device).manual_seed(5))
    assert sum(_lib.call_counts.values()) == before + 2 and [hip_calls(name) - c for name, c in zip(names, c0)] == [1, 1, 0, 0, 0]
    seed5, step0 = ta._rng.reserve(torch.Generator(device=cuda_device).manual_seed(5), cuda_device, K)
    _chain(spec, src, native, n, dim, K, None, seed5, step0, cuda_device)
    assert torch.equal(got, native) and torch.equal(src.cpu(), case["x"])
    before, c0 = sum(_lib.call_counts.values()), [hip_calls(name) for name in names]
    g = model.gradient(src)
    assert sum(_lib.call_counts.values()) == before + 2 and [hip_calls(name) - c for name, c in zip(names, c0)] == [1, 0, 1, 0, 0]
    _within(g, case["eval32"][1], case["eval64"][1], 2e-6)
    if dim <= 32:  # without the opt-in this width keeps today's exact-f32 entries
        plain = _gpu_model(case, cuda_device, opt_in=False)
        assert plain.fused_spec().aux is None
        c0 = [hip_calls(name) for name in names]
        ta.LangevinDynamics(plain, step_size=ETA, device=cuda_device).sample(x=src, n_steps=K)
        plain.gradient(src)
        assert [hip_calls(name) - c for name, c in zip(names, c0)] == [0, 0, 0, 1, 1]


@pytest.mark.parametrize("hidden,dim,kind,with_aux,code", [(64, 8, 8, True, -3), (128, 129, 8, True, -3), (128, 8, 4, True, -2),
                                                          (128, 8, 8, False, -1)])
def test_refusals_launch_nothing(cuda_device, hidden, dim, kind, with_aux, code):
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp = kind, hidden
    params = torch.zeros(16, device=cuda_device)  # never read: every refusal comes before any device access
    desc.dev0 = params.data_ptr()
    desc.aux = params.data_ptr() if with_aux else None
    x = torch.zeros(4, dim, device=cuda_device)
    st = _lib.stream_handle(cuda_device)
    assert _lib.lib().ebm_energy_grad_mlp3_stream_f32(desc, x.data_ptr(), 4, dim, None, x.data_ptr(), st) == code
    assert _lib.lib().ebm_langevin_chain_mlp3_stream_f32(desc, x.data_ptr(), x.data_ptr(), 4, dim, 3, 0.1, 0.3, 1.0, None, 0, 0, st) == code
    assert torch.equal(x.cpu(), torch.zeros(4, dim))
