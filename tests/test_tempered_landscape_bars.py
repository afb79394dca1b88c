"""The cases of tests/test_tempered_landscapes_gpu.py hold what they claim, on the CPU: every case's fp32 and float64
restatements take the same decisions with no borderline call, reject and accept enough to exercise both outcomes, and three
deliberately wrong fp32 evaluations -- run through the restatements as if they were the kernel -- fail the GPU test's own checks
(check_langevin / check_hmc / check_ais there: a changed decision or the float64 yardstick) in at least one case of every family
they apply to.  Also the inputs of the GPU file's identity and safe-mode tests: both accept outcomes occur, no swap decision of a
wild ladder is borderline, and the tame rows' fp32 and float64 runs agree far inside the bars the GPU test asks of the kernel."""

import math

import pytest
import torch

import ais_cases
import tempering_cases
import tempering_hmc_cases
import test_tempered_landscapes_gpu as gpu
from tempering_cases import MARGIN_BAR, Landscape, model_of, oracle_of
from test_tempering_gpu import want_counts
from test_tempering_hmc_gpu import want_swap_counts


# ---------------------------------------------------------------------------------
# the conditions every case meets on the restatement alone
# ---------------------------------------------------------------------------------
def _swap_conditions(ref32, ref64, n, R, events):
    assert torch.equal(ref32["mask"], ref64["mask"])
    want = want_counts(ref32["mask"], n, R)
    tried, took = int(want[: R - 1].sum()), int(want[R - 1 :].sum())
    if events >= 2 and n >= 37:
        assert 0 < took < tried, (took, tried)
    return took, tried


def _reject_conditions(accepted):
    rejected, total = int((~accepted).sum()), accepted.numel()
    assert 0.02 * total <= rejected <= 0.5 * total, (rejected, total)
    return rejected, total


@pytest.mark.parametrize("kind,dim,R,n,swap_every,k", tempering_cases.LANDSCAPE_CASES)
def test_langevin_ladder_case(kind, dim, R, n, swap_every, k):
    c = tempering_cases.case(kind, dim, R, n, swap_every, k)
    assert c["ref64"]["margin"].min().item() > MARGIN_BAR, c["seed"]
    assert torch.isfinite(c["ref32"]["x"]).all() and torch.isfinite(c["ref64"]["x"]).all()
    print(kind, dim, "seed", c["seed"], "swaps %d of %d" % _swap_conditions(c["ref32"], c["ref64"], n, R, k // swap_every))
    # the kernel's own place in the GPU test: the fp32 restatement passes the checks it is held to
    gpu.check_langevin(c, c["ref32"]["x"], want_counts(c["ref32"]["mask"], n, R))


@pytest.mark.parametrize("kind,dim,R,n,swap_every,n_mh", tempering_hmc_cases.LANDSCAPE_CASES)
def test_hmc_ladder_case(kind, dim, R, n, swap_every, n_mh):
    c = tempering_hmc_cases.case(kind, dim, R, n, swap_every, n_mh)
    ref32, ref64 = c["ref32"], c["ref64"]
    assert tempering_hmc_cases.closest_call(ref64) > MARGIN_BAR, c["seed"]
    assert torch.equal(ref32["accepted"], ref64["accepted"])
    print(kind, dim, "seed", c["seed"], "rejects %d of %d" % _reject_conditions(ref32["accepted"]),
          "swaps %d of %d" % _swap_conditions(ref32, ref64, n, R, n_mh // swap_every))
    gpu.check_hmc(c, _as_hmc_run(ref32, n, R))


@pytest.mark.parametrize("kind,dim,n,T", ais_cases.LANDSCAPE_CASES)
def test_ais_case(kind, dim, n, T):
    c = ais_cases.case(kind, dim, n, T)
    ref32, ref64 = c["ref32"], c["ref64"]
    assert ref64["margin"].min().item() > MARGIN_BAR, c["seed"]
    assert torch.equal(ref32["accepted"], ref64["accepted"])
    assert torch.isfinite(ref32["logw"]).all() and torch.isfinite(ref64["logw"]).all()
    print(kind, dim, "seed", c["seed"], "rejects %d of %d" % _reject_conditions(ref32["accepted"]))
    gpu.check_ais(c, _as_ais_run(ref32))


def test_the_cases_cover_what_they_name():
    for cases, dims in ((tempering_cases.LANDSCAPE_CASES, gpu.DIMS + (260,)), (tempering_hmc_cases.LANDSCAPE_CASES, gpu.DIMS),
                        (ais_cases.LANDSCAPE_CASES, gpu.DIMS)):
        for kind in gpu.KINDS:
            assert {c[1] for c in cases if c[0] == kind} == set(dims)
        assert any(c[0] == "ackley_c3" for c in cases)
        assert any(c[-3 if len(c) == 6 else -2] == 1 for c in cases), "no single ladder / chain"
    for cases in (tempering_cases.LANDSCAPE_CASES, tempering_hmc_cases.LANDSCAPE_CASES):
        assert 2 * sum(c[4] == 1 for c in cases) >= len(cases), "swap_every = 1 in at least half of the cases"


# ---------------------------------------------------------------------------------
# three wrong evaluations, as if they were the kernel
# ---------------------------------------------------------------------------------
class RosenbrockWithoutVectorBoundary(Landscape):
    """The coupling term of x_{4 j + 3} with x_{4 j + 4} left out: a lane that takes 0 for the first element of the vector that
    follows its own (a neighbour exchange that does not arrive)."""

    def energy(self, x):
        m = self.model
        head, tail = x[:, :-1], x[:, 1:]
        inside = (torch.arange(x.shape[-1] - 1) % 4 != 3).to(x.dtype)
        return ((m.a - head).pow(2) + m.b * inside * (tail - head.pow(2)).pow(2)).sum(dim=-1)


def padded_width(dim):
    """4 G NV of the lane geometry (rows.h pick_geometry): G the smallest power of two with 4 G >= dim, up to 64 lanes."""
    g = 1
    while 4 * g < dim and g < 64:
        g *= 2
    return 4 * g * -(-dim // (4 * g))


class AckleyOverThePaddedWidth(Landscape):
    """Both means taken over the padded width 4 G instead of dim."""

    def energy(self, x):
        m = self.model
        n = padded_width(x.shape[-1])
        radial = -m.a * torch.exp(-m.b * torch.sqrt(torch.sum(x**2, dim=-1) / n))
        ripple = -torch.exp(torch.sum(torch.cos(m.c * x), dim=-1) / n)
        return radial + ripple + m.a + math.e


def wrong_energy(spec):
    model = model_of(spec)
    return RosenbrockWithoutVectorBoundary(model) if spec["kind"] == "rosenbrock" else AckleyOverThePaddedWidth(model)


def _as_hmc_run(r, n, R):
    return {"x": r["x"], "traj": r["traj"], "accepted": r["accepted"], "accepts": r["accepted"].sum(dim=(0, 1)).long(),
            "swaps": want_swap_counts(r["mask"], n, R)}


def _as_ais_run(r):
    return {"x": r["x"], "logw": r["logw"], "accepted": r["accepted"], "counts": r["accepted"].sum(dim=1).long()}


def _caught(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _langevin_caught(c, energy):
    (n, R, _), se = c["shape"], c["swap_every"]
    r = tempering_cases.restate(energy, c["x0"], c["noise"], c["u"], tempering_cases.ETA, tempering_cases.SIGMA, c["temps"], se)
    return _caught(gpu.check_langevin, c, r["x"], want_counts(r["mask"], n, R))


def _hmc_caught(c, energy):
    (n, R, _), se = c["shape"], c["swap_every"]
    r = tempering_hmc_cases.restate(energy, c["x0"], c["z"], c["u_accept"], c["u_swap"], c["eps"], c["L"], c["temps"], se, thin=2)
    return _caught(gpu.check_hmc, c, _as_hmc_run(r, n, R))


def _ais_caught(c, energy, force_betas=None):
    r = ais_cases.restate(energy, c["x0"], c["z"], c["u"], c["betas"], c["eps"], c["L"], c["base_std"], force_betas=force_betas)
    return _caught(gpu.check_ais, c, _as_ais_run(r))


FAMILIES = {
    "langevin": (tempering_cases, _langevin_caught),
    "hmc": (tempering_hmc_cases, _hmc_caught),
    "ais": (ais_cases, _ais_caught),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("kind", gpu.KINDS)
def test_a_wrong_energy_fails_the_gpu_checks(kind, family):
    """Rosenbrock without the coupling across a float4 boundary, Ackley with its means over the padded width.  (Rosenbrock at dim
    2 and Ackley on the full rows 32, 64 and 256 cannot tell: there the wrong evaluation is the right one.)"""
    module, caught = FAMILIES[family]
    hits = []
    for shape in module.LANDSCAPE_CASES:
        if not shape[0].startswith(kind):
            continue
        c = module.case(*shape)
        hits.append((shape, caught(c, wrong_energy(c["spec"]))))
    print(hits)
    same = [s for s, _ in hits if (s[1] == 2 if kind == "rosenbrock" else padded_width(s[1]) == s[1])]
    assert not any(hit for s, hit in hits if s in same), "a case in which the wrong evaluation is the right one failed"
    missed = [s for s, hit in hits if not hit and s not in same]
    assert not missed, missed  # (more than the one case per family that is asked: every case that can tell does)


@pytest.mark.parametrize("kind", gpu.KINDS)
def test_a_force_at_the_previous_beta_fails_the_ais_checks(kind):
    """AIS with the trajectory's force mixed at beta_{t-1}: a carried force that was not rebuilt when beta moved."""
    hits = []
    for shape in ais_cases.LANDSCAPE_CASES:
        if not shape[0].startswith(kind):
            continue
        c = ais_cases.case(*shape)
        lagged = torch.cat([c["betas"][:1], c["betas"][:-1]])
        hits.append((shape, _ais_caught(c, oracle_of(c["spec"]), force_betas=lagged)))
    print(hits)
    assert all(hit for _, hit in hits), hits


# ---------------------------------------------------------------------------------
# the inputs of the identity, native-draw and safe-mode tests
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", gpu.KINDS)
def test_identity_inputs_take_both_accept_outcomes(kind):
    for dim in gpu.DIMS:
        energy = oracle_of(tempering_cases.energy_spec(kind, dim))
        i = gpu.identity_inputs(kind, dim, "hmc")
        n, R, _ = i["x0"].shape
        r = tempering_hmc_cases.restate(energy, i["x0"], i["z"], i["ua"], torch.zeros(0, n, R), (i["eps"],) * R, i["L"], None, i["n_mh"] + 1,
                                        sqrt_temp=torch.ones(R), beta=torch.ones(R))
        rejected, total = int((~r["accepted"]).sum()), r["accepted"].numel()
        a = gpu.identity_inputs(kind, dim, "ais")
        ra = ais_cases.restate(energy, a["x0"], a["z"], a["u"], torch.tensor([0.0, 1.0]), (a["eps"],), a["L"], a["base_std"])
        rejected_a, total_a = int((~ra["accepted"]).sum()), ra["accepted"].numel()
        print(kind, dim, "hmc rejects %d of %d" % (rejected, total), "ais rejects %d of %d" % (rejected_a, total_a))
        # (at least 3 either way: a kernel decision that differs from torch's in one chain still leaves both outcomes)
        assert 3 <= rejected <= total - 3 and 3 <= rejected_a <= total_a - 3
        assert torch.isfinite(r["x"]).all() and torch.isfinite(ra["x"]).all() and torch.isfinite(ra["logw"]).all()


@pytest.mark.parametrize("kind,dim,R,n", [("rosenbrock", 12, 4, 37), ("ackley", 100, 3, 37)])
def test_frozen_ladders_accept_and_reject_swaps(kind, dim, R, n):
    c = tempering_hmc_cases.frozen_case(kind, dim, R, n)
    lan, hmc = tempering_hmc_cases.frozen_masks(c)
    assert torch.equal(lan["mask"], hmc["mask"]) and hmc["accepted"].all()
    print(kind, dim, "seed", c["seed"], "swaps", int(lan["mask"].sum()), "of", c["attempts"])
    assert 0 < int(lan["mask"].sum()) < c["attempts"]


def _rel(a, b):
    return ((a.double() - b).abs() / b.abs().clamp(min=1.0)).max().item()


@pytest.mark.parametrize("dim", [5, 100])
@pytest.mark.parametrize("kind", gpu.KINDS)
def test_safe_mode_inputs(kind, dim):
    """The wild starts are what they are meant to be, every swap decision of the runs with them is clear of its threshold, their
    NaN / inf patterns are not empty where the test compares them, and on the clean inputs fp32 and float64 agree five times
    inside the 5e-4 the GPU test asks of the tame rows: that number measures the kernel and not the dynamics."""
    energy = oracle_of(tempering_cases.energy_spec(kind, dim))
    pick = lambda cases, i: next(s for s in cases if s[:2] == (kind, dim) and s[i] >= 37)  # noqa: E731
    lan, hmc, ais = (tempering_cases.case(*pick(tempering_cases.LANDSCAPE_CASES, 3)), tempering_hmc_cases.case(*pick(tempering_hmc_cases.LANDSCAPE_CASES, 3)),
                     ais_cases.case(*pick(ais_cases.LANDSCAPE_CASES, 2)))
    x0 = gpu.wild_ladders(kind, hmc["x0"])
    if kind == "ackley":
        assert torch.isfinite(energy.energy(x0[3, 1:2])).all() and torch.isnan(energy.grad(x0[3, 1:2])).all()
    else:
        assert not torch.isfinite(energy.grad(x0[3, 1:2])).all()
        assert torch.isinf(energy.energy(x0[7, 0:1])).all() and torch.isfinite(energy.grad(x0[7, 0:1])).all()
    # Langevin
    r = tempering_cases.restate(energy, gpu.wild_ladders(kind, lan["x0"]), lan["noise"], lan["u"], tempering_cases.ETA, tempering_cases.SIGMA,
                                lan["temps"], lan["swap_every"])
    assert (r["margin"] > MARGIN_BAR).all() and torch.isnan(r["x"]).any()
    others = [i for i in range(37) if i not in gpu.WILD]
    assert torch.equal(r["x"][others], lan["ref32"]["x"][others])
    # HMC
    r = tempering_hmc_cases.restate(energy, x0, hmc["z"], hmc["u_accept"], hmc["u_swap"], hmc["eps"], hmc["L"], hmc["temps"], hmc["swap_every"])
    assert (r["margin"] > MARGIN_BAR).all()
    sure = r["mh_margin"][:, list(gpu.WILD)] > MARGIN_BAR
    print(kind, dim, "hmc: sure decisions of the wild ladders", int(sure.sum()), "of", sure.numel(), "accepted there",
          int(r["accepted"][:, list(gpu.WILD)].sum()))
    assert torch.equal(r["x"][others], hmc["ref32"]["x"][others]) and sure.float().mean() > 0.9
    tame = [_rel(hmc["ref32"]["x"], hmc["ref64"]["x"])]
    # AIS
    r = ais_cases.restate(energy, gpu.wild_chains(kind, ais["x0"]), ais["z"], ais["u"], ais["betas"], ais["eps"], ais["L"], ais["base_std"])
    print(kind, dim, "ais: logw of the wild chains", r["logw"][list(gpu.WILD)].tolist())
    assert torch.equal(r["x"][others], ais["ref32"]["x"][others]) and torch.equal(r["logw"][others], ais["ref32"]["logw"][others])
    if kind == "rosenbrock":
        assert not torch.isfinite(r["logw"][list(gpu.WILD)]).any()
    tame += [_rel(ais["ref32"]["x"], ais["ref64"]["x"]), _rel(ais["ref32"]["logw"], ais["ref64"]["logw"])]
    print(kind, dim, "fp32 against float64 on the clean inputs: hmc states, ais states, ais logw", tame)
    assert max(tame) < 1e-4
