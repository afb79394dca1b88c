"""CPU tier of the step-route kernel tests: the restatements of step_cases.py tell a plausible wrong kernel from a right one on
the very inputs test_step_kernels_gpu.py runs, and the conditions that make `torch.equal` the right assertion there hold for
the reference alone -- no FMA input near an fp32 rounding midpoint, no accept decision within 1024 ulp of its uniform."""

import math

import pytest
import torch

import oracle
from oracle.hmc import leapfrog
import step_cases as sc

def _differs(right, wrong, what):
    share = sc.share_differing(right, wrong)
    print(f"{what}: {round(share * right.numel())} of {right.numel()} elements differ ({100.0 * share:.4f} %)")
    assert share > 0.0, what
    return share


# ---------------------------------------------------------------------------------
# every wrong variant shows on the cases' own inputs
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, sc.BIG_GROUPS[1]])
def test_a_contracted_drift_shows(n):
    c = sc.elem_case(n)
    args = (c["x"], c["grad"], c["noise"], sc.ETA, sc.SQRT_ETA, sc.NOISE_COEF)
    _differs(sc.langevin_step(*args), sc.langevin_step(*args, fused_drift=True), "langevin step, x - eta g as an FMA")
    _differs(sc.langevin_step(*args, clamp=sc.CLAMP), sc.langevin_step(*args, clamp=sc.CLAMP, fused_drift=True), "... clamped")


@pytest.mark.parametrize("dim", [1, 3, 5, 64])
def test_a_split_square_root_shows(dim):
    """Over the periods of a row width (1, dim, n_elem): a field of one or three values may hide it, the set does not."""
    n = 7 * dim
    c = sc.elem_case(n)
    right, wrong = [], []
    for period in sorted({1, dim, n}):
        args = (c["x"], c["grad"], c["noise"], sc.diffusion_field(period), period, sc.ETA, sc.SQRT_ETA)
        right.append(sc.diffusion_step(*args))
        wrong.append(sc.diffusion_step(*args, split_sqrt=True))
        print(f"period {period}: {100.0 * sc.share_differing(right[-1], wrong[-1]):.3f} % differ")
    _differs(torch.cat(right), torch.cat(wrong), f"diffusion, sqrt(2) sqrt(D), dim {dim}")


@pytest.mark.parametrize("n_chains,dim", [(205, 5)] + list(sc.BIG_KICK_DRIFT))
def test_the_wrong_kicks_show(n_chains, dim):
    c = sc.kick_case(n_chains, dim, True)
    x, p, f = c["x"], c["p"], c["force"]
    # 0.5 (eps f) is (0.5 eps) f up to a power of two, so it can only differ where eps f leaves the range: the 3e38 force
    right = sc.kick_drift(x, p, f, sc.EPS)
    wrong = sc.kick_drift(x, p, f, sc.EPS, variant="half_last")
    _differs(right[1], wrong[1], "kick-drift p_half, 0.5 (eps f)")
    _differs(right[0], wrong[0], "kick-drift x_new, 0.5 (eps f)")
    mass = sc.diag_mass(dim)
    for name, kind, scalar in sc.MASS_FORMS[1:]:
        if name == "tiny":
            continue  # (eps / 1e-10 and (eps p) / 1e-10 differ too; one scalar form is enough)
        right = sc.kick_drift(x, p, f, sc.EPS, kind, scalar, mass)
        wrong = sc.kick_drift(x, p, f, sc.EPS, kind, scalar, mass, variant="hoisted")
        _differs(right[0], wrong[0], f"kick-drift x_new, eps / m hoisted, {name} mass")
    # safe mode: a clamp that swallows the NaN force
    right = sc.kick_drift(x, p, f, sc.EPS, safe=True)
    wrong = sc.kick_drift(x, p, f, sc.EPS, safe=True, variant="drop_nan")
    _differs(right[1], wrong[1], "kick-drift p_half, clamp drops NaN")
    right = sc.kick(x, p, f, sc.EPS, safe=True)
    wrong = sc.kick(x, p, f, sc.EPS, safe=True, variant="drop_nan")
    _differs(right[1], wrong[1], "kick p_new, clamp drops NaN")


@pytest.mark.parametrize("n", [1025, sc.BIG_ELEM])
def test_an_unfused_descent_shows(n):
    c = sc.elem_case(n)
    _differs(sc.descent_step(c["x"], c["grad"], None, sc.DESCENT_ETA, 0.0)[0],
             sc.descent_step(c["x"], c["grad"], None, sc.DESCENT_ETA, 0.0, unfused=True)[0], "plain descent, multiply then add")
    right = sc.descent_step(c["x"], c["grad"], c["v"], sc.DESCENT_ETA, sc.MOMENTUM)
    wrong = sc.descent_step(c["x"], c["grad"], c["v"], sc.DESCENT_ETA, sc.MOMENTUM, unfused=True)
    _differs(right[1], wrong[1], "momentum descent v, multiply then add")
    _differs(right[0], wrong[0], "momentum descent x, multiply then add")
    _differs(sc.lookahead(c["x"], c["v"], sc.MOMENTUM), sc.lookahead(c["x"], c["v"], sc.MOMENTUM, unfused=True), "lookahead")


def test_the_wrong_accept_rules_show():
    for n, dim in ((63, 1), (1000, 3), sc.ACCEPT_BIG[0]):
        c = sc.accept_case(n, dim)
        wide = sc.accept_ref(c["h0"], c["h1"], c["u"], clamp_at=88.0)[0]
        loose = sc.accept_ref(c["h0"], c["h1"], c["u"], strict=False)[0]
        print(f"accept n {n}: clamp at 88 flips {(wide != c['acc']).sum().item()}, u <= a flips {(loose != c['acc']).sum().item()}")
        assert (wide != c["acc"]).any(), "the clamp at 88 decides like the clamp at 50"
        assert (loose != c["acc"]).any(), "u <= a decides like u < a"


# ---------------------------------------------------------------------------------
# the conditions behind torch.equal
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.SMALL + (sc.BIG_ELEM,))
def test_no_fma_input_sits_on_a_midpoint(n):
    c = sc.elem_case(n)
    neg_eta, mu = -sc.s32(sc.DESCENT_ETA), sc.s32(sc.MOMENTUM)
    for what, (a, b, cc) in {"plain": (neg_eta, c["grad"], c["x"]), "momentum": (neg_eta, c["grad"], c["v"] * mu),
                             "lookahead": (mu, c["v"], c["x"])}.items():
        risk = sc.fma_midpoint_risk(a, b, cc)
        assert not risk.any(), f"{what}: {int(risk.sum())} elements within one float64 ulp of an fp32 midpoint"


def test_the_midpoint_check_sees_a_midpoint():
    one, ulp = torch.ones(1), torch.tensor([2.0**-24])
    assert sc.fma_midpoint_risk(one, one, ulp).all()  # 1 + half an ulp32: a tie
    assert sc.fma_midpoint_risk(-one, one, -ulp).all()
    assert not sc.fma_midpoint_risk(one + 2.0**-23, one - 2.0**-24, 0.0 * one).any()  # 2^-47 below the tie: 32 float64 ulps
    assert not sc.fma_midpoint_risk(one, one, ulp * 1.5).any()
    assert not sc.fma_midpoint_risk(one, one, ulp * 0.5).any()


@pytest.mark.parametrize("n,dim", sc.accept_shapes())
def test_no_accept_decision_is_close(n, dim):
    c = sc.accept_case(n, dim)
    nan_rows = torch.isnan(c["a64"])
    edges = sc.edge_positions(n)
    want_nan = torch.zeros(n, dtype=torch.bool)
    for pos, j in edges.items():
        want_nan[pos] = math.isnan(sc.EDGE_ROWS[j][0] - sc.EDGE_ROWS[j][1])  # a NaN Hamiltonian, or inf - inf
    assert torch.equal(nan_rows, want_nan), "a NaN acceptance outside the NaN edge rows"
    ok = sc.accept_margin_ok(c["u"], c["a64"]) | nan_rows  # (a NaN acceptance rejects whatever expf returns)
    assert ok.all(), f"{int((~ok).sum())} chains within {sc.ACCEPT_ULPS} ulp of their uniform"
    for pos, j in edges.items():
        assert bool(c["acc"][pos]) == sc.EDGE_ROWS[j][3], (pos, sc.EDGE_ROWS[j])
    # both outcomes occur wherever there is room for them
    if n >= 63:
        assert c["acc"].any() and (~c["acc"]).any()
        assert set(edges.values()) == set(range(len(sc.EDGE_ROWS)))
    assert torch.isnan(c["x"]).sum() == (0 if c["acc"].all() else 1)


# ---------------------------------------------------------------------------------
# the restatement is not only this file's reading of the header
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("safe", [False, True])
@pytest.mark.parametrize("name,kind,scalar", sc.MASS_FORMS)
def test_the_two_sub_steps_are_the_oracle_leapfrog(name, kind, scalar, safe):
    n, dim = 37, 5
    g = torch.Generator().manual_seed(11)
    x, p = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g)
    x[3, 1] = 300.0  # a force past the safe-mode clamp
    energy, mass = oracle.DoubleWell(2.0, 1.0), sc.diag_mass(dim)
    want_x, want_p = leapfrog(energy, x, p, 0.05, 1, sc.oracle_mass(kind, scalar, mass), safe=safe)
    got_x, got_p = sc.leapfrog_once(energy, x, p, 0.05, kind, scalar, mass, safe)
    assert sc.same_bits(got_x, want_x) and sc.same_bits(got_p, want_p)
    assert torch.isfinite(want_p[:, 4]).all() and not sc.same_bits(want_x, x)
