"""The folded DoubleWell loop (langevin_elem.h FOLD: the gradient's power-of-two factor 4h = 2^m in the drift coefficient,
taken when 4h = 2^m with m >= 0 and b^2 = 1) gives the state the same chain gives with the field of ebm_noise_fill_f32
injected (the literal kernel), bit for bit: finite values by their bits, NaN at the same places.  The start states hold
+-0, +-1 and their neighbours, subnormals, +-inf, NaN, values inside the overflow window FLT_MAX / 2^m < |u x| <= FLT_MAX
where the two forms differ (the guard redoes those lanes with the literal loop) and a log-uniform sweep whose chains fall
into that window partway through the launch.  h = 1.5 and b = 1.5 stay on the literal loop.  Launches below, across and
past step 2^32 run both Philox counter widths; 3603 elements leave the last workgroup and the last float4 group partly
filled."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from torchebm_amd.samplers.langevin import em_coefficients

pytestmark = pytest.mark.gpu

SEED = 0x0F1E_2D3C_4B5A_6978
TWO32 = 1 << 32
N, DIM = 1201, 3  # 3603 elements: 901 float4 groups, the last one holding three
F32_MAX = torch.finfo(torch.float32).max


def _start_states():
    one = torch.tensor([1.0])
    special = torch.tensor([
        0.0, -0.0, 1.0, -1.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126, -1e-40, 2.0 ** -103, -2.0 ** -102, 1e-30,
        float("inf"), float("-inf"), float("nan"), 3.4e12, 3.6e12, -5e12, 6.0e12, -6.9e12, 7.1e12, 1e13, 1e20, F32_MAX, -F32_MAX,
        4e4, -4e4, 1e4, 79.0, 1e3])
    near_one = torch.cat([torch.nextafter(one, one * 2), torch.nextafter(one, one * 0)]).reshape(-1)
    special = torch.cat([special, near_one, -near_one])
    g = torch.Generator().manual_seed(7)
    n_sweep = 1600
    mag = 10.0 ** (torch.rand(n_sweep, generator=g, dtype=torch.float64) * 16 - 3)  # |x| from 1e-3 to 1e13
    sign = torch.where(torch.rand(n_sweep, generator=g) < 0.5, -1.0, 1.0).double()
    rest = N * DIM - special.numel() - n_sweep
    x = torch.cat([special, (mag * sign).float(), torch.randn(rest, generator=g) * 1.5])
    return x.reshape(N, DIM).contiguous()


def _eta(h):
    return 0.01 if h <= 4 else 2.0 ** -10  # 8 h eta < 2: the wells are stable (otherwise every chain ends in NaN)


def _chain(spec, x, k, eta, noise, step0, device):
    a, sq, coef = em_coefficients(eta, 1.0)
    n, dim = x.shape
    _lib.call("ebm_langevin_chain_f32", spec.to_c(), x.data_ptr(), n, dim, k, a, sq, coef, None, 0, 0.0, 0.0, 1, None, None,
              noise.data_ptr() if noise is not None else None, SEED, step0, _lib.stream_handle(device))


def _emulate(x0, noise, h, b2, eta, fold):
    """the step in fp32 torch ops on the CPU, every multiply and add rounded: literal, or with 4h folded into eta."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    a, sq, coef = em_coefficients(eta, 1.0)
    four_h, eta, b2t, sqt, coeft = f(4.0 * h), f(a), f(b2), f(sq), f(coef)
    e = f(math.ldexp(float(f(a)), int(round(math.log2(4.0 * h))))) if fold else None
    x = x0.clone()
    for i in range(noise.shape[0]):
        u = x * x - b2t
        x1 = x - e * (u * x) if fold else x - eta * ((four_h * u) * x)
        x = x1 + coeft * (noise[i].view_as(x) * sqt)
    return x


def _same(a, b):
    """bit-identical finite and infinite values, NaN at the same places"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


@pytest.mark.parametrize("k", [1, 2, 7, 200])
@pytest.mark.parametrize("step0", [5, TWO32 - 3, TWO32 + 5])
@pytest.mark.parametrize("h,b,folded", [(0.25, 1.0, True), (0.5, 1.0, True), (2.0, 1.0, True), (4.0, 1.0, True),
                                        (64.0, 1.0, True), (1.5, 1.0, False), (2.0, 1.5, False)])
def test_lean_fold_matches_injected_field(cuda_device, h, b, folded, step0, k):
    spec = ta.DoubleWellModel(barrier_height=h, b=b, device=cuda_device).fused_spec()
    eta = _eta(h)
    x0 = _start_states()
    rows = torch.empty(k, N * DIM + 1, device=cuda_device)  # ebm_noise_fill_f32 writes 16-byte aligned rows
    for i in range(k):
        _lib.call("ebm_noise_fill_f32", rows[i].data_ptr(), N * DIM, _lib.NOISE_NORMAL, SEED, step0 + i, _lib.stream_handle(cuda_device))
    noise = rows[:, :N * DIM].contiguous()
    native, injected = x0.to(cuda_device), x0.to(cuda_device)
    _chain(spec, native, k, eta, None, step0, cuda_device)
    _chain(spec, injected, k, eta, noise, step0, cuda_device)
    torch.cuda.synchronize(cuda_device)
    native, injected = native.cpu(), injected.cpu()
    assert _same(native, injected)
    fin = torch.isfinite(native)
    assert fin.float().mean() > 0.4 and not fin.all() and not torch.equal(native[fin], x0[fin])

    # the inputs do reach the overflow window, where the folded arithmetic alone ends differently from the literal one in a
    # short launch (a few steps later both chains are NaN: the window absorbs)
    literal = _emulate(x0, noise.cpu(), h, b * b, eta, fold=False)
    assert _same(literal, injected)
    if folded and h > 0.25 and k <= 2:
        assert not _same(_emulate(x0, noise.cpu(), h, b * b, eta, fold=True), literal)
