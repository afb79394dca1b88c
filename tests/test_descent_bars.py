"""The bars of tests/test_descent_fp64_gpu.py, on the CPU (tests/descent_cases.py): for every energy kind, width and both
update rules the inputs are a fair yardstick -- the fp32 oracle's own chain is off the float64 one in the median chain --
and a deliberately degraded evaluation fails the bar the GPU test asserts: the Gaussian / mixture contraction on
two-term bf16 operands (tests/test_fp64_bars.py), the landscapes' gradient of inputs rounded to 16 significant bits
(landscape_cases.degraded_grad).  The two element-wise energies are held to bit-equality with the fp32 oracle instead, which
needs no bar.  No constant here is tuned against a GPU."""

import pytest
import torch

import descent_cases as dc
import landscape_cases as lc
import oracle
from helpers import yardstick
from test_fp64_bars import grad_split2

torch.set_num_threads(1)


class Degraded:
    """an energy whose gradient is the degraded evaluation (fp32 states in, fp32 gradient out)"""

    def __init__(self, s):
        self.s = s
        self.m = lc.model(s.kind) if s.kind in lc.ENERGIES else None

    def grad(self, x):
        if self.m is not None:
            return lc.degraded_grad(self.s.kind, self.m, x).float()
        return grad_split2(self.s.case, x, self.s.fp).float()


def _fails(got, r32, r64, **factors):
    try:
        yardstick(got, r32, r64, **factors)
    except AssertionError:
        return True
    return False


def _check_case(kind, dim, K, nesterov):
    s = dc.setup(kind, dim, K)
    assert len(set(s.etas)) == dc.K_STEPS and all(e == float(torch.tensor(e, dtype=torch.float32)) for e in s.etas)
    r32, r64 = dc.refs(kind, dim, K, nesterov)
    assert torch.isfinite(r64).all() and r32.dtype == torch.float32 and r64.dtype == torch.float64
    err = (r32.double() - r64).abs().amax(dim=1)
    assert err.median().item() > 0.0, (kind, dim, K, "the fp32 reference lands on float64: no yardstick")
    assert (r64 - s.x0.double()).abs().amax(dim=1).median().item() > 0.0  # the chain moves
    if kind in dc.EXACT:
        return None
    factors = dc.yardstick_factors(kind, K)
    yardstick(r32, r32, r64, **factors)
    deg, _, _ = oracle.descent_chain(Degraded(s), s.x0, s.etas, dc.MU if nesterov else None)
    # The bar is the conjunction the GPU test asserts.  (Which factor catches the degraded evaluation depends on the case: the
    # iteration contracts, so at a few dims the rounding of the state itself outweighs the gradient's error in the worst chain and
    # only the median tells; the ratios are returned for the report.)
    assert _fails(deg, r32, r64, **factors), (kind, dim, K, nesterov, "passes on degraded operands")
    st = yardstick(deg, r32, r64, k_med=1e30)
    return {"med": st["hip_med"] / st["ref_med"], "q90": st["hip_q90"] / st["ref_q90"], "max": st["hip_max"] / st["ref_max"]}


CASES = [(k, K, d) for k, K in dc.ENERGIES for d in dc.widths(k)]


@pytest.mark.parametrize("nesterov", [False, True], ids=["gd", "nesterov"])
@pytest.mark.parametrize("kind,K,dim", CASES, ids=[f"{k}{K or ''}-d{d}" for k, K, d in CASES])
def test_fp32_oracle_is_a_yardstick_and_degraded_operands_fail(kind, K, dim, nesterov):
    ratios = _check_case(kind, dim, K, nesterov)
    if ratios is not None:
        print(kind, K, dim, "nesterov" if nesterov else "gd", "degraded error / fp32 reference error:", ratios)


@pytest.mark.parametrize("nesterov", [False, True], ids=["gd", "nesterov"])
def test_padded_mixture(nesterov):
    kind, K, dim = dc.GMM_PADDED
    print(_check_case(kind, dim, K, nesterov))


def test_every_geometry_and_both_parameter_placements_are_covered():
    """rows.h pick_geometry: G = 1 .. 64 with one vector per lane up to 256 dims, then (64, 2) and (64, 4); plan_params: 56 KiB of
    LDS for the parameters"""
    def geometry(dim):
        nvec = (dim + 3) // 4
        if nvec <= 64:
            g = 1
            while g < nvec:
                g <<= 1
            return g, 1
        return (64, 2) if nvec <= 128 else (64, 4)

    masked = {geometry(d) for d in dc.WIDTHS if d != 4 * geometry(d)[0] * geometry(d)[1]}
    full = {geometry(d) for d in dc.WIDTHS if d == 4 * geometry(d)[0] * geometry(d)[1]}
    every = {(1 << p, 1) for p in range(7)} | {(64, 2), (64, 4)}
    assert masked == every and full == every
    assert set(dc.STRUCT_WIDTHS) <= set(dc.WIDTHS)

    def gauss_floats(dim):
        return dim * ((dim + 3) & ~3)

    def gmm_floats(dim, K):
        kp = 8 if K < 8 else (K + 7) & ~7
        return kp * ((dim + 3) & ~3) + ((kp + 3) & ~3)

    budget = 56 * 1024 // 4  # floats (rows.h kParamLdsBudget)
    assert 119 in dc.WIDTHS and 120 in dc.WIDTHS and gauss_floats(119) <= budget < gauss_floats(120)
    assert 892 in dc.WIDTHS and 893 in dc.WIDTHS and gmm_floats(892, 16) <= budget < gmm_floats(893, 16)
    assert ("gmm", 16) in dc.ENERGIES and gmm_floats(1024, 8) <= budget  # eight components stay in LDS at every width
