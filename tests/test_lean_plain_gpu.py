"""The plain-f32 folded DoubleWell loop (langevin_elem.h PLAIN, kind 17, langevin_fold.hip: what the plain DoubleWell call
launches) against k launches of the per-step kernel fed with torch-autograd gradients: the same generator state, so the same
Philox field, and the states agree bit for bit (compared as int32, so the signs of zeros and the inf / NaN patterns count too).
Shapes: one partial float4 group (5 x 3), one workgroup plus one lane (257 x 4), several workgroups (300 x 64); k = 1, 2, 7
walks the two-step unroll and its tail; a generator offset past 2^32 runs the 64-bit-counter instantiation.  One lane starts
at 6.0 in one coordinate: it diverges (-inf after 5 steps, NaN after 6), fails the folded loop's guard and is redone by the
literal loop."""

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from torchebm_amd.samplers.langevin import em_coefficients

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0F_7A11_CAFE
TWO32 = 1 << 32
ETA, SIGMA = 0.01, 1.0


def _fused(spec, x0, k, step0, device):
    a, sq, coef = em_coefficients(ETA, SIGMA)
    x = x0.clone()
    n, dim = x.shape
    _lib.call("ebm_langevin_chain_f32", spec.to_c(), x.data_ptr(), n, dim, k, a, sq, coef, None, 0, 0.0, 0.0, 1, None, None,
              None, SEED, step0, _lib.stream_handle(device))
    return x


def _per_step(model, x0, k, step0, device):
    a, sq, coef = em_coefficients(ETA, SIGMA)
    x = x0.clone()
    for i in range(k):
        g = model.gradient(x)
        out = torch.empty_like(x)
        _lib.call("ebm_langevin_step_f32", x.data_ptr(), g.data_ptr(), out.data_ptr(), None, x.numel(), a, sq, coef, 0, 0.0, 0.0,
                  SEED, step0 + i, _lib.stream_handle(device))
        x = out
    return x


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("k", [1, 2, 7])
@pytest.mark.parametrize("step0", [1000, TWO32 + 5], ids=["c32", "c64"])
@pytest.mark.parametrize("n,dim", [(5, 3), (257, 4), (300, 64)])
def test_plain_fold_equals_per_step_kernel(cuda_device, n, dim, step0, k):
    model = ta.DoubleWellModel(device=cuda_device)  # h = 2, b = 1: 4h = 2^3, the folded route
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(3)).clamp_(-2.5, 2.5).to(cuda_device)
    got = _fused(model.fused_spec(), x0, k, step0, cuda_device)
    want = _per_step(model, x0, k, step0, cuda_device)
    torch.cuda.synchronize(cuda_device)
    assert torch.isfinite(want).all() and not torch.equal(want, x0)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("k,ends", [(5, "inf"), (7, "nan")])
@pytest.mark.parametrize("step0", [1000, TWO32 + 5], ids=["c32", "c64"])
def test_lane_that_leaves_the_guard_is_redone_literally(cuda_device, step0, k, ends):
    n, dim = 257, 4
    model = ta.DoubleWellModel(device=cuda_device)
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(4)).clamp_(-2.5, 2.5)
    x0[100, 2] = 6.0  # 6 -> -10.8 -> 89 -> -5.7e4 -> 1.4e13 -> -inf -> NaN: 8 h eta |x|^2 > 2 never comes back
    x0 = x0.to(cuda_device)
    got = _fused(model.fused_spec(), x0, k, step0, cuda_device)
    want = _per_step(model, x0, k, step0, cuda_device)
    torch.cuda.synchronize(cuda_device)
    bad = want[100, 2]
    assert bool(torch.isinf(bad)) if ends == "inf" else bool(torch.isnan(bad))
    assert int((~torch.isfinite(want)).sum()) == 1  # the lane's other three coordinates stay finite, and are redone with it
    assert torch.equal(_bits(got), _bits(want))
