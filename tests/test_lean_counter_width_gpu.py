"""The lean Langevin kernels draw at 32-bit Philox counter words when the launch allows it (langevin_elem.h lean_counters32:
ceil(n_elem / 4) <= 2^32 and step0 + k <= 2^32) and at the full 64-bit counter otherwise.  Launches around step 2^32 -- one
that crosses it (64-bit fallback), one that ends exactly on it and one far below (32-bit path), one past it -- must give
the state the same chain gives with the field of ebm_noise_fill_f32 injected, bit for bit."""

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from torchebm_amd.samplers.langevin import em_coefficients

pytestmark = pytest.mark.gpu

SEED = 0x0123_4567_89AB_CDEF
TWO32 = 1 << 32


def _chain(fn, spec, x, k, noise, step0, clamp, device):
    a, sq, coef = em_coefficients(0.01, 1.0)
    n, dim = x.shape
    _lib.call(fn, spec.to_c(), x.data_ptr(), n, dim, k, a, sq, coef, None, 1 if clamp else 0, -1.5, 1.5, 1, None, None,
              noise.data_ptr() if noise is not None else None, SEED, step0, _lib.stream_handle(device))


@pytest.mark.parametrize("step0,k", [(TWO32 - 3, 8), (TWO32 - 8, 8), (5, 8), (TWO32 + 7, 4)])
@pytest.mark.parametrize("model,fn,clamp", [("double_well", "ebm_langevin_chain_f32", False),
                                            ("double_well", "ebm_langevin_chain_f32", True),
                                            ("harmonic", "ebm_langevin_chain_f32", False),
                                            ("double_well", "ebm_langevin_heun_chain_f32", False)])
def test_lean_chain_across_step_2_32_matches_injected_field(cuda_device, step0, k, model, fn, clamp):
    n, dim = 300, 12  # 3600 elements: 900 float4 groups, the last workgroup partly filled
    m = ta.DoubleWellModel(device=cuda_device) if model == "double_well" else ta.HarmonicModel(device=cuda_device)
    spec = m.fused_spec()
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(11)).clamp_(-2.5, 2.5).to(cuda_device)
    noise = torch.empty(k, n * dim, device=cuda_device)
    for i in range(k):
        _lib.call("ebm_noise_fill_f32", noise[i].data_ptr(), n * dim, _lib.NOISE_NORMAL, SEED, step0 + i, _lib.stream_handle(cuda_device))
    native, injected = x0.clone(), x0.clone()
    _chain(fn, spec, native, k, None, step0, clamp, cuda_device)
    _chain(fn, spec, injected, k, noise, step0, clamp, cuda_device)
    torch.cuda.synchronize(cuda_device)
    assert torch.isfinite(native).all()
    assert torch.equal(native, injected)
    assert not torch.equal(native, x0)
