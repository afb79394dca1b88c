"""ebm_langevin_chain_from_f32 (include/ebm_hip.h): the fused Langevin chain started from a read-only source state and
stored to a second tensor.  The yardstick is the in-place entry ebm_langevin_chain_f32 run on a clone of the source with the
same seed and offset -- the entry the bit-exact, oracle and fp64 tests hold to the reference.  Every comparison is
torch.equal, and every case checks that the source still holds what it held before the call.

The element-wise kernels read the source themselves (langevin_elem.h: the prologue load); the shapes are those at which the
flat kernel takes another path: 3 x 5 (one partial float4 group: scalar loads and stores), 256 x 4 (exactly one workgroup),
257 x 4 (one workgroup and one group more), 41 x 12, k = 3 and 4 (the two-step unroll with and without its odd tail).
DoubleWell(h = 2, b = 1) takes the folded loop, DoubleWell(h = 1.5) the literal one.  Every other kernel family gets the
source copied into the output by the entry and runs in place: one small case each."""

import pytest
import torch

import torchebm_amd as ta
from helpers import hip_calls
from torchebm_amd import _lib, _rng
from torchebm_amd.samplers.langevin import em_coefficients

pytestmark = pytest.mark.gpu

SEED = 0x1357_9BDF_0246_8ACE
TWO32 = 1 << 32
SHAPES = [(3, 5), (256, 4), (257, 4), (41, 12)]
ENERGIES = ["fold", "literal", "harmonic"]


def _model(name, device):
    if name == "fold":
        return ta.DoubleWellModel(barrier_height=2.0, b=1.0, device=device)
    if name == "literal":
        return ta.DoubleWellModel(barrier_height=1.5, b=1.0, device=device)
    return ta.HarmonicModel(k=1.3, device=device)


def _start(n, dim, device, seed=3):
    return torch.randn(n, dim, generator=torch.Generator().manual_seed(seed)).clamp_(-2.5, 2.5).to(device)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _in_place(spec, x, k, device, *, flags=0, noise=None, step0=5, eta=0.01):
    a, sq, coef = em_coefficients(eta, 1.0)
    n, dim = x.shape
    _lib.call("ebm_langevin_chain_f32", spec.to_c(), x.data_ptr(), n, dim, k, a, sq, coef, None, flags, -1.5, 1.5, 1, None, None,
              _lib.ptr(noise), SEED, step0, _lib.stream_handle(device))


def _from(spec, src, out, k, device, *, flags=0, noise=None, step0=5, eta=0.01):
    a, sq, coef = em_coefficients(eta, 1.0)
    n, dim = out.shape
    _lib.call("ebm_langevin_chain_from_f32", spec.to_c(), _lib.ptr(src), out.data_ptr(), n, dim, k, a, sq, coef, None, flags,
              -1.5, 1.5, 1, None, None, _lib.ptr(noise), SEED, step0, _lib.stream_handle(device))


def _check_entry(spec, x0, k, device, **kw):
    """the out-of-place entry against the in-place one on a clone; the output starts as NaN, so an element the launch
    does not write fails the comparison"""
    want, src, keep = x0.clone(), x0.clone(), x0.clone()
    out = torch.full_like(x0, float("nan"))
    before = hip_calls("ebm_langevin_chain_f32")
    _in_place(spec, want, k, device, **kw)
    _from(spec, src, out, k, device, **kw)
    torch.cuda.synchronize(device)
    assert hip_calls("ebm_langevin_chain_f32") == before + 2  # the out-of-place entry is booked under the same name
    assert torch.equal(_bits(src), _bits(keep))
    assert torch.equal(_bits(out), _bits(want))
    assert not torch.equal(want, keep)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the C entry, element-wise kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("n,dim", SHAPES)
@pytest.mark.parametrize("energy", ENERGIES)
def test_entry_matches_in_place_entry(cuda_device, energy, n, dim, k):
    spec = _model(energy, cuda_device).fused_spec()
    out = _check_entry(spec, _start(n, dim, cuda_device), k, cuda_device)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("energy", ENERGIES)
def test_entry_with_clamp(cuda_device, energy):
    spec = _model(energy, cuda_device).fused_spec()
    out = _check_entry(spec, _start(41, 12, cuda_device), 3, cuda_device, flags=_lib.CHAIN_CLAMP)
    assert out.abs().max().item() <= 1.5


@pytest.mark.parametrize("energy", ENERGIES)
def test_entry_with_contracted_arithmetic(cuda_device, energy):
    spec = _model(energy, cuda_device).fused_spec()
    _check_entry(spec, _start(257, 4, cuda_device), 4, cuda_device, flags=_lib.CHAIN_CONTRACTED)


@pytest.mark.parametrize("step0", [TWO32 - 2, TWO32 + 7])  # a launch that crosses 2^32 and one past it: 64-bit counters
@pytest.mark.parametrize("energy", ENERGIES)
def test_entry_with_wide_counters(cuda_device, energy, step0):
    spec = _model(energy, cuda_device).fused_spec()
    _check_entry(spec, _start(41, 12, cuda_device), 4, cuda_device, step0=step0)


@pytest.mark.parametrize("n,dim", [(3, 5), (257, 4)])
@pytest.mark.parametrize("energy", ENERGIES)
def test_entry_with_injected_noise(cuda_device, energy, n, dim):
    """the general kernel (langevin_chain_elem_kernel), which an injected field selects"""
    k = 3
    spec = _model(energy, cuda_device).fused_spec()
    noise = torch.randn(k, n, dim, generator=torch.Generator().manual_seed(9)).to(cuda_device)
    _check_entry(spec, _start(n, dim, cuda_device), k, cuda_device, noise=noise)


def test_fold_redo_lane_starts_from_the_source(cuda_device):
    """One coordinate starts at 1e13: its lane fails the folded loop's guard and is run again by the literal loop -- from the
    start values, which are the SOURCE's.  That lane ends non-finite in both runs; bit patterns are compared."""
    spec = _model("fold", cuda_device).fused_spec()
    x0 = _start(257, 4, cuda_device)
    x0[100, 2] = 1e13
    out = _check_entry(spec, x0, 4, cuda_device)
    assert not torch.isfinite(out[100, 2]).item()
    fin = torch.isfinite(out)
    assert (~fin).sum().item() <= 4 and not fin[100].all()  # the lane's own float4 group at the most


def test_null_and_same_source_are_the_in_place_call(cuda_device):
    spec = _model("fold", cuda_device).fused_spec()
    x0 = _start(41, 12, cuda_device)
    want, a, b = x0.clone(), x0.clone(), x0.clone()
    _in_place(spec, want, 3, cuda_device)
    _from(spec, None, a, 3, cuda_device)
    _from(spec, b, b, 3, cuda_device)
    torch.cuda.synchronize(cuda_device)
    assert torch.equal(a, want) and torch.equal(b, want)


def test_no_step_copies_the_source(cuda_device):
    spec = _model("fold", cuda_device).fused_spec()
    src = _start(41, 12, cuda_device)
    out = torch.full_like(src, float("nan"))
    _from(spec, src, out, 0, cuda_device)
    torch.cuda.synchronize(cuda_device)
    assert torch.equal(out, src)


# ---------------------------------------------------------------------------------------------------------------
# the sampler: sample() reads the caller's tensor and writes a fresh one; donate_input = True is the in-place entry
# ---------------------------------------------------------------------------------------------------------------
def _sampler(energy, device, **kw):
    return ta.LangevinDynamics(_model(energy, device), step_size=kw.pop("step_size", 0.01), device=device, **kw)


def _gen(device, offset=0):
    g = torch.Generator(device=device).manual_seed(77)
    if offset:
        _rng._set_offset(g, offset)
    return g


def _check_sampler(make, x0, k, device, *, offset=0, **call):
    """sample(x) against the same sampler with donate_input = True (ebm_langevin_chain_f32 in place) on a clone"""
    keep, donated = x0.clone(), x0.clone()
    ref = make()
    ref.donate_input = True
    want = ref.sample(x=donated, n_steps=k, generator=_gen(device, offset), **call)
    s = make()
    before = hip_calls("ebm_langevin_chain_f32")
    got = s.sample(x=x0, n_steps=k, generator=_gen(device, offset), **call)
    torch.cuda.synchronize(device)
    assert hip_calls("ebm_langevin_chain_f32") > before
    assert torch.equal(_bits(x0), _bits(keep))
    want_t, got_t = (want[0], got[0]) if isinstance(want, tuple) else (want, got)
    assert got_t.data_ptr() != x0.data_ptr()
    assert torch.equal(_bits(got_t), _bits(want_t))
    if isinstance(want, tuple):
        for name in want[1]:
            assert torch.equal(_bits(got[1][name]), _bits(want[1][name])), name
    return got


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("n,dim", SHAPES)
@pytest.mark.parametrize("energy", ENERGIES)
def test_sample_matches_donated_call(cuda_device, energy, n, dim, k):
    x0 = _start(n, dim, cuda_device)
    before = hip_calls("ebm_langevin_chain_f32")
    got = _check_sampler(lambda: _sampler(energy, cuda_device), x0, k, cuda_device)
    assert hip_calls("ebm_langevin_chain_f32") == before + 2  # one launch per call, no other one
    assert torch.isfinite(got).all() and not torch.equal(got, x0)


def test_sample_with_scheduler(cuda_device):
    make = lambda: ta.LangevinDynamics(_model("fold", cuda_device), step_size=ta.core.LinearScheduler(0.01, 0.002, 4),  # noqa: E731
                                       noise_scale=ta.core.CosineScheduler(1.0, 0.2, 5), device=cuda_device)
    _check_sampler(make, _start(41, 12, cuda_device), 5, cuda_device)


def test_sample_with_clamp(cuda_device):
    got = _check_sampler(lambda: _sampler("literal", cuda_device, clamp=(-1.0, 1.0)), _start(257, 4, cuda_device), 3, cuda_device)
    assert got.abs().max().item() <= 1.0


def test_sample_with_thinned_trajectory(cuda_device):
    got = _check_sampler(lambda: _sampler("harmonic", cuda_device), _start(41, 12, cuda_device), 5, cuda_device, thin=2,
                         return_trajectory=True)
    assert got.shape == (41, 2, 12)


def test_sample_with_diagnostics(cuda_device):
    got, diag = _check_sampler(lambda: _sampler("fold", cuda_device), _start(256, 8, cuda_device), 4, cuda_device, thin=2,
                               return_diagnostics=True)
    assert diag["mean"].shape == (2, 8) and torch.isfinite(diag["energy"]).all()


def test_sample_with_fused_arithmetic(cuda_device):
    def make():
        s = _sampler("fold", cuda_device)
        s.fused_arithmetic = True
        return s

    _check_sampler(make, _start(257, 4, cuda_device), 4, cuda_device)


def test_sample_with_generator_offset_past_2_32(cuda_device):
    _check_sampler(lambda: _sampler("fold", cuda_device), _start(41, 12, cuda_device), 4, cuda_device, offset=4 * (TWO32 + 3))


def test_chunked_records_read_the_source_once(cuda_device):
    """DIAG_RECORD_BYTES lowered on the instance cuts the call into several launches: only the first may read the caller's
    tensor, every later one continues in place on the output.  The cut call equals the uncut one."""
    x0 = _start(256, 8, cuda_device)
    keep = x0.clone()
    whole = _sampler("fold", cuda_device)
    want, want_d = whole.sample(x=x0, n_steps=5, return_diagnostics=True, generator=_gen(cuda_device))
    cut = _sampler("fold", cuda_device)
    layout = _lib.diag_layout(cut.model.fused_spec().to_c(), _lib.DIAG_LANGEVIN, 256, 8)
    cut.DIAG_RECORD_BYTES = 2 * 4 * layout[0] * (2 * layout[1] + 8)  # the records of two kept steps: launches of 2, 2 and 1 steps
    before = hip_calls("ebm_langevin_chain_f32")
    got, got_d = cut.sample(x=x0, n_steps=5, return_diagnostics=True, generator=_gen(cuda_device))
    torch.cuda.synchronize(cuda_device)
    assert hip_calls("ebm_langevin_chain_f32") == before + 3
    assert torch.equal(_bits(x0), _bits(keep))
    assert torch.equal(_bits(got), _bits(want))
    for name in want_d:
        assert torch.equal(_bits(got_d[name]), _bits(want_d[name])), name
    # ... and the uncut call is the donated (in-place) one
    _check_sampler(lambda: _sampler("fold", cuda_device), x0, 5, cuda_device, return_diagnostics=True)


def test_diagnostics_off_the_flat_kernel(cuda_device):
    """rows of 12 neither divide nor are divided by the flat kernel's 1024-element blocks: an element-wise energy whose
    diagnostics call is served by another kernel family, which gets the source copied into the output by the entry"""
    _check_sampler(lambda: _sampler("literal", cuda_device), _start(41, 12, cuda_device), 5, cuda_device, thin=2,
                   return_diagnostics=True)


# ---------------------------------------------------------------------------------------------------------------
# kernel families that update in place: the entry copies the source into the output first
# ---------------------------------------------------------------------------------------------------------------
def _gaussian(dim, device):
    g = torch.Generator().manual_seed(dim)
    a = torch.randn(dim, dim, generator=g)
    return ta.GaussianModel(torch.zeros(dim), a @ a.t() / dim + 0.5 * torch.eye(dim), device=device)


def _mlp(device):
    torch.manual_seed(0)
    return ta.MLPEnergy(2, device=device)


FALLBACK = {
    "gaussian_dim8": (lambda d: _gaussian(8, d), 64, 8),          # the lane-group / packed route
    "gaussian_dim64": (lambda d: _gaussian(64, d), 64, 64),       # the matrix route
    "ring_mixture": (lambda d: ta.core.ring_mixture(8, 32, device=d), 64, 32),
    "mlp": (_mlp, 128, 2),
}


@pytest.mark.parametrize("family", sorted(FALLBACK))
def test_fallback_families_match_in_place_entry(cuda_device, family):
    make, n, dim = FALLBACK[family]
    model = make(cuda_device)
    spec = model.fused_spec()
    _check_entry(spec, _start(n, dim, cuda_device), 3, cuda_device)
    # and through the sampler
    _check_sampler(lambda: ta.LangevinDynamics(model, step_size=0.01, device=cuda_device), _start(n, dim, cuda_device, seed=4), 3,
                   cuda_device)
