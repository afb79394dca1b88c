"""ebm_chain_stats_f32 -- the mean / var diagnostics of every sampler configuration without in-kernel records -- against
float64, both kernels (csrc/misc.hip chain_stats_kernel, chain_stats_wide_kernel).  Shapes, data and the derived bars:
tests/chain_stats_cases.py; tests/test_chain_stats_bars.py checks the bars on the CPU.  The bars are derived from the kernels'
arithmetic, not measured: a result outside them is a bug in the kernel or in the derivation."""

import pytest
import torch

import chain_stats_cases as sc
from chain_cases import family_of
from helpers import launched_kernels
from torchebm_amd import _lib

pytestmark = pytest.mark.gpu

VAR_FLOOR = torch.tensor(1e-10, dtype=torch.float32)


def _work(dim, dev):
    return torch.zeros(2 * dim + 1, dtype=torch.float64, device=dev)


def _stats(x, work):
    """(mean, var) of a device [n, dim] fp32 tensor; outputs pre-filled with a sentinel, one element of slack behind each"""
    n, dim = x.shape
    mean = torch.full((dim + 1,), 7.0, device=x.device)
    var = torch.full((dim + 1,), 7.0, device=x.device)
    _lib.call("ebm_chain_stats_f32", x.data_ptr(), n, dim, mean.data_ptr(), var.data_ptr(), work.data_ptr(), _lib.stream_handle(x.device))
    torch.cuda.synchronize()
    assert mean[dim].item() == 7.0 and var[dim].item() == 7.0, "wrote past the outputs"
    return mean[:dim].cpu(), var[:dim].cpu()


def _work_is_zero(work):
    """all 2 dim + 1 doubles, the ticket (an integer in the last one) included, bit for bit"""
    return not bool(work.view(torch.int64).any())


def _run_shapes(shapes, kind, wide, dev):
    worst = (0.0, 0.0, 0.0)
    for n, dim in shapes:
        assert sc.is_wide(n, dim) == wide
        x = sc.data(kind, n, dim)
        work = _work(dim, dev)
        mean, var = _stats(x.to(dev), work)
        r = sc.check(mean, var, x, wide=wide, what=(kind, n, dim))
        worst = tuple(max(a, b) for a, b in zip(worst, r))
        assert _work_is_zero(work), (kind, n, dim)
        if kind == "constant" or n == 1:
            assert bool((var == VAR_FLOOR).all()), (kind, n, dim)
    print("wide" if wide else "generic", kind, "worst error / bar: mean %.3f var %.3f; worst |dvar| / var %.3e" % worst)


@pytest.mark.parametrize("kind", sc.DATA)
def test_generic_kernel_meets_the_bars(cuda_device, kind):
    _run_shapes(sc.GENERIC_SHAPES, kind, False, cuda_device)


@pytest.mark.parametrize("kind", sc.DATA)
def test_wide_kernel_meets_the_bars(cuda_device, kind):
    _run_shapes(sc.WIDE_SHAPES, kind, True, cuda_device)


@pytest.mark.parametrize("shape,wide", [(sc.GENERIC_LARGE, False), (sc.WIDE_LARGE, True)], ids=["generic-rows-capped", "wide-blocks-capped"])
def test_past_the_block_caps(cuda_device, shape, wide):
    """more rows than the capped grid covers in one sweep: every block loops.  The float64 reference is taken on the device."""
    n, dim = shape
    assert sc.is_wide(n, dim) == wide
    work = _work(dim, cuda_device)
    for kind in ("normal", "mean1e4"):
        x = sc.data(kind, n, dim, device=cuda_device)
        mean, var = _stats(x, work)
        print(shape, kind, "error / bar: mean %.3f var %.3f; |dvar| / var %.3e" % sc.check(mean, var, x, wide=wide, what=(kind, n, dim)))
        assert _work_is_zero(work)


def test_dispatch(cuda_device):
    """which kernel a shape runs: the power-of-two path from n dim = 1024, dims 4 .. 1024; everything else the generic one"""
    for n, dim in ((255, 4), (256, 4), (15, 64), (16, 64), (1, 512), (1, 1024), (sc.N, 2), (sc.N, 96), (sc.N, 1024), (sc.N, 2048)):
        x = sc.data("normal", n, dim).to(cuda_device)
        work = _work(dim, cuda_device)
        with launched_kernels() as k:
            _stats(x, work)
        want = "chain_stats_wide_kernel" if sc.is_wide(n, dim) else "chain_stats_kernel"
        ours = [family_of(name) for name in k.names if "chain_stats" in name]  # (the rest: torch's fills of the outputs)
        assert ours == [want], (n, dim, k.names)


@pytest.mark.parametrize("dim", [100, 64])
def test_work_is_shared_across_calls(cuda_device, dim):
    """three calls with different inputs and row counts on ONE work buffer, zeroed once: each is right and leaves all
    2 dim + 1 doubles zero"""
    work = _work(dim, cuda_device)
    rows = {100: (1000, 257, 33), 64: (1000, 15, 4096)}[dim]  # (width 64: the wide kernel, the generic one below 1024 elements, the wide one)
    for kind, n in zip(("normal", "mean1e4", "outlier"), rows):
        x = sc.data(kind, n, dim, salt=1)
        mean, var = _stats(x.to(cuda_device), work)
        sc.check(mean, var, x, wide=sc.is_wide(n, dim), what=(kind, n, dim))
        assert _work_is_zero(work), (kind, n, dim)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("n,dim", [(sc.N, 100), (sc.N, 64), (4352, 4)])
def test_a_non_finite_column_stays_in_its_column(cuda_device, n, dim, bad):
    wide = sc.is_wide(n, dim)
    col = dim // 3
    x = sc.data("normal", n, dim, salt=2)
    x[n // 2, col] = bad
    work = _work(dim, cuda_device)
    mean, var = _stats(x.to(cuda_device), work)
    assert not torch.isfinite(mean[col]) and not torch.isfinite(var[col]), (mean[col], var[col])
    keep = torch.arange(dim) != col
    m64, v64, mean_bar, var_bar = sc.bars(x[:, keep], wide)
    assert bool(((mean[keep].double() - m64).abs() <= mean_bar).all()) and bool(((var[keep].double() - v64).abs() <= var_bar).all())
    assert _work_is_zero(work), "a non-finite sum was left in the work buffer"
    y = sc.data("mean1e4", n, dim, salt=3)
    mean, var = _stats(y.to(cuda_device), work)
    sc.check(mean, var, y, wide=wide, what=("after non-finite", n, dim))
    assert _work_is_zero(work)


def test_outlier_first_row_costs_the_wide_kernel_accuracy(cuda_device):
    """The same bars hold; what they allow differs: the generic kernel's var stays at fp32 rounding, the wide kernel's error is
    relative to the spread about row 0 (m2 ~ 1e6 here, var ~ 1).  Printed for both (include/ebm_hip.h says so)."""
    for n, dim in ((sc.N, 100), (sc.N, 64), (4352, 4), (17, 1024)):
        x = sc.data("outlier", n, dim, salt=4)
        mean, var = _stats(x.to(cuda_device), _work(dim, cuda_device))
        wide = sc.is_wide(n, dim)
        _, _, rel = sc.check(mean, var, x, wide=wide, what=("outlier", n, dim))
        print("wide" if wide else "generic", (n, dim), "outlier row 0: |dvar| / var = %.3e" % rel)
