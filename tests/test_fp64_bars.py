"""The bars of tests/test_fp64_one_step_gpu.py, on the CPU: the fp32 oracle's own evaluation (oracle.Gaussian /
oracle.GaussianMixture in fp32) meets each of them, and the same evaluation with a contraction whose operands are rounded
to a TWO-term bf16 split (hi = bf16(a), lo = bf16(a - hi), the third piece dropped) fails each of them.  These set the
constants of tests/chain_cases.py (k_step, K_GMM, GMM_FORCE_TARGET, C_H, C_EXP; for the diagnostics records K_REC_GAUSS,
K_REC_GMM and the derived sums_bar / m2_bar) -- none is tuned against a GPU."""

import pytest
import torch

import chain_cases as cc
from helpers import yardstick


def split2(a):
    """a as the sum of its two leading bf16 pieces, in float64 (products of such pieces are exact there)."""
    a = a.float()
    hi = a.bfloat16().float()
    lo = (a - hi).bfloat16().float()
    return hi.double() + lo.double()


def gauss_grad_split2(x, fp):
    mean, ps = fp
    return split2(x - mean) @ split2(ps).t()


def gmm_grad_split2(x, fp):
    """the kernels' form: |x|^2 - 2 x.mu + |mu|^2 with x.mu on split operands, then the weighted means the same way."""
    means, sigma, logw = fp
    x = x.float()
    sq = (x.double().square().sum(1, keepdim=True) - 2 * (split2(x) @ split2(means).t()) +
          means.double().square().sum(1)[None]).float().double()
    w = torch.softmax(logw.double()[None] - sq / (2 * sigma ** 2), dim=1)
    return (x.double() - split2(w) @ split2(means)) / sigma ** 2


def grad_split2(case, x, fp):
    return gauss_grad_split2(x, fp) if case.energy == "gauss" else gmm_grad_split2(x, fp)


def _case(sampler, energy, dim, K=0, mass="none", n=300):
    return cc.Case(sampler, energy, dim, K=K, mass=mass, n=n)


def langevin_bar_holds(case, x0, fp, got):
    eta = 0.25 if case.energy == "gauss" else 0.5
    want, natural = cc.langevin_ref(case, x0, fp, eta)
    err = (got.double() - want).abs()
    if case.energy == "gauss":
        return (err / natural).max().item() < cc.k_step(case.dim) * cc.U
    try:
        yardstick(got, cc.langevin_ref32(case, x0, fp, eta), want, k_med=2.0, k_max=16.0)
    except AssertionError:
        return False
    return (err.amax(dim=1) / natural).max().item() < cc.K_GMM * cc.U


LANGEVIN_SAMPLE = [_case("langevin", "gauss", d, n=n) for d, n in ((10, 320), (20, 300), (64, 300), (157, 300), (254, 300), (512, 200))] + \
                  [_case("langevin", "gmm", d, K) for d, K in ((20, 8), (64, 16), (128, 32), (200, 12), (255, 16))]


@pytest.mark.parametrize("case", LANGEVIN_SAMPLE, ids=lambda c: c.id)
def test_langevin_bars(case):
    fp = cc.cpu_params(case)
    x0 = cc.langevin_x0(case, fp)
    eta = 0.25 if case.energy == "gauss" else 0.5
    assert langevin_bar_holds(case, x0, fp, cc.langevin_ref32(case, x0, fp, eta)), "the fp32 oracle misses the bar"
    two = (x0.double() - eta * grad_split2(case, x0, fp)).float()
    assert not langevin_bar_holds(case, x0, fp, two), "a two-term bf16 contraction passes the bar"


def test_heun_bar_is_met_by_the_oracle():
    case = _case("heun", "gauss", 64)
    fp = cc.cpu_params(case)
    x0 = cc.langevin_x0(case, fp)
    assert langevin_bar_holds(case, x0, fp, cc.langevin_ref32(case, x0, fp, 0.25))


# (a thousand Gaussian chains: above 200 dims two-term energies misdecide only two to eight of the ~570 kept ones)
HMC_SAMPLE = [_case("hmc", "gauss", d, mass=m, n=1000) for d, m in ((20, "none"), (64, "diag"), (160, "scalar"), (200, "none"), (255, "none"))] + \
             [_case("hmc", "gmm", d, K, mass=m) for d, K, m in ((20, 8, "none"), (96, 16, "diag"), (228, 16, "none"))]


def hmc_bar_holds(case, x0, p, mass, fp, eps, got):
    want, natural, _ = cc.hmc_ref(case, x0, p, mass, fp, eps)
    err = (got.double() - want).abs()
    if case.energy == "gauss":
        return (err / natural).max().item() < cc.k_step(case.dim) * cc.U
    try:
        yardstick(got, cc.hmc_ref32(case, x0, p, mass, fp, eps), want, k_med=2.0, k_max=16.0)
    except AssertionError:
        return False
    return (err.amax(dim=1) / natural).max().item() < cc.K_GMM * cc.U


@pytest.mark.parametrize("case", HMC_SAMPLE, ids=lambda c: c.id)
def test_hmc_position_bars(case):
    fp = cc.cpu_params(case)
    x0, p, mass = cc.hmc_inputs(case, fp)
    eps = cc.hmc_eps(case, x0, p, mass, fp, target=1.0 if case.energy == "gauss" else cc.GMM_FORCE_TARGET)
    assert hmc_bar_holds(case, x0, p, mass, fp, eps, cc.hmc_ref32(case, x0, p, mass, fp, eps)), "the fp32 oracle misses the bar"
    m = torch.ones(case.dim, dtype=torch.float64) if mass is None else (
        torch.full((case.dim,), mass, dtype=torch.float64) if isinstance(mass, float) else mass.double())
    ps = p.double() * m.sqrt()
    two = (x0.double() + eps * (ps - 0.5 * eps * grad_split2(case, x0, fp)) / m).float()
    assert not hmc_bar_holds(case, x0, p, mass, fp, eps, two), "a two-term bf16 force passes the bar"


def energy_split2(case, x, fp):
    if case.energy == "gauss":
        mean, ps = fp
        d = (x - mean).double()
        return 0.5 * (split2(d.float()) * (split2(d.float()) @ split2(ps).t())).sum(dim=1)
    means, sigma, logw = fp
    x = x.float()
    sq = (x.double().square().sum(1, keepdim=True) - 2 * (split2(x) @ split2(means).t()) + means.double().square().sum(1)[None])
    return -torch.logsumexp(logw.double()[None] - sq.float().double() / (2 * sigma ** 2), dim=1)


@pytest.mark.parametrize("case", HMC_SAMPLE, ids=lambda c: c.id)
def test_hmc_accept_bars(case):
    """the margin delta: the fp32 oracle's H0, H1 decide every kept chain as float64 does; H from two-term bf16 contractions
    (on the same fp32 leapfrog state) decide some of them wrongly."""
    fp = cc.cpu_params(case)
    x0, p, mass = cc.hmc_inputs(case, fp)
    x0 = cc.hmc_accept_x0(case, x0, fp)
    eps = cc.hmc_accept_eps(case, x0, p, mass, fp)
    h0, h1, n0, n1 = cc.hmc_hamiltonians64(case, x0, p, mass, fp, eps)
    keep, u, below = cc.accept_draws(h0, h1, n0, n1)
    assert keep.sum().item() >= case.n // 4

    def decisions(e0, e1):
        a = torch.exp((e0 - e1).clamp(-50, 50)).clamp(max=1.0)
        return u.double() < a

    H0, H1 = cc.hmc_hamiltonians32(case, x0, p, mass, fp, eps)
    assert not (keep & (decisions(H0.double(), H1.double()) != below)).any(), "the fp32 oracle decides a kept chain wrongly"
    en = cc._oracle32(case, fp)
    pm = p.clone() if mass is None else p * (mass ** 0.5 if isinstance(mass, float) else mass.sqrt())
    x1, p1 = cc.oracle.hmc.leapfrog(en, x0, pm, eps, 1, mass, safe=True)
    k0, k1 = cc.oracle.hmc.kinetic(pm, mass).double(), cc.oracle.hmc.kinetic(p1, mass).double()
    b0, b1 = energy_split2(case, x0, fp) + k0, energy_split2(case, x1, fp) + k1
    assert (keep & (decisions(b0, b1) != below)).any(), "two-term bf16 energies decide every kept chain as float64 does"


# ----------------------------------------------------------------------------------------------------------------
# Diagnostics records (tests/test_records_fp64_gpu.py): the record-to-chain map, then the bars of a record's energy share,
# column sums and M2
# ----------------------------------------------------------------------------------------------------------------
RECORD_DIMS = sorted({c.dim for c in cc.ROUTES if c.records})
RAGGED_N = (1, 31, 33, 129, 300)


def record_geometries(n, dim):
    """every documented form at this width: a wave's 32 rows (classes / packed rows where the width asks for them), the
    lane-group blocks of 1 .. 64 chains, a chain spread over 2 .. 4 blocks, the flat kernel's 1024 elements"""
    out = []
    for nn in (n, n + (-n) % 16):  # (packed rows need a chain count the packing divides)
        try:
            out.append((nn, cc.wave_layout(nn, dim)))
        except AssertionError:
            pass
    out += [(n, cc.rows_layout(n, dim, c)) for c in (1, 2, 5, 16, 64)]
    out += [(n, (cc.record_count(dim // f, dim // f, n, dim), dim // f, dim // f)) for f in (2, 3, 4) if dim % f == 0]
    if 1024 % dim == 0 or dim % 1024 == 0:
        out.append((n, (cc.record_count(min(dim, 1024), 1024, n, dim), min(dim, 1024), 1024)))
    return out


@pytest.mark.parametrize("dim", RECORD_DIMS + [2, 1024, 2048])
def test_record_chains_puts_every_chain_in_exactly_one_record(dim):
    forms = set()
    for n0 in RAGGED_N:
        for n, layout in record_geometries(n0, dim):
            nb, S, E = layout
            forms.add("classes" if E < 0 else "packed" if S > dim else "rows" if E % dim == 0 else "slices")
            # the record count of diag::plan / plan_classes (csrc/diag.h)
            want = -(-n // (32 * cc.diag_classes(dim))) * cc.diag_classes(dim) if E < 0 else -(-(n * dim) // E)
            assert nb == want and nb == cc.record_count(S, E, n, dim), (n, layout)
            idx = cc.record_chains(layout, n, dim)
            assert len(idx) == nb and all(i.shape[1] == S for i in idx), (n, layout)
            flat = torch.cat([i.flatten() for i in idx])
            assert torch.equal(flat.sort().values, torch.arange(n * dim)), (n, layout)  # every element once
            W = max(S, dim)
            for b, i in enumerate(idx):  # slot s holds one column of the rows of width W, and a record whole rows or one slice
                assert i.shape[0] <= max(1, abs(E) // W), (n, layout, b)
                assert (i % W == i[:1] % W).all() and (E % W != 0 or (i[:, 0] % W == 0).all()), (n, layout, b)
            groups = cc.record_groups(layout, n, dim)
            chains = torch.cat([c for _, c in groups])
            assert torch.equal(chains.sort().values, torch.arange(n)), (n, layout)  # every chain in one group
            assert [r for rs, _ in groups for r in rs] == list(range(nb)), (n, layout)
            if E < 0:  # the interleaving, spelt out
                K = cc.diag_classes(dim)
                for b, (_, c) in enumerate(groups):
                    assert all(int(v) % K == b % K and int(v) // (32 * K) == b // K for v in c), (n, layout, b)
    assert "rows" in forms and (dim % 4 == 0 or dim < 20 or "classes" in forms) and (dim >= 20 or dim < 3 or "packed" in forms), forms


def gmm_energy_expansion32(x, fp):
    """the mixture energy as the matrix-layout kernels form it -- |x|^2 - 2 x.mu + |mu|^2 -- with every operation in fp32"""
    means, sigma, logw = fp
    sq = x.square().sum(1, keepdim=True) - 2 * (x @ means.t()) + means.square().sum(1)[None]
    return -torch.logsumexp(logw.float()[None] - sq / (2 * sigma ** 2), dim=1)


def kept_state32(case, fp):
    """the fp32 oracle's state after one step of the one-step tests' inputs: what a record of that step describes"""
    if case.sampler == "hmc":
        x0, p, mass = cc.hmc_inputs(case, fp)
        eps = cc.hmc_eps(case, x0, p, mass, fp, target=1.0 if case.energy == "gauss" else cc.GMM_FORCE_TARGET)
        return cc.hmc_ref32(case, x0, p, mass, fp, eps)
    x0 = cc.langevin_x0(case, fp)
    return cc.langevin_ref32(case, x0, fp, 0.25 if case.energy == "gauss" else 0.5)


def record_energy_ratios(case, layout, fp, x, energies, fp32_sum):
    """worst record's |energy share - float64| / (U sum N(E)) of per-chain energies summed over each record's chains"""
    e64, nat = cc.energy64(case, x, fp)
    groups = cc.record_groups(layout, case.n, case.dim)
    want = torch.stack([e64[c].sum() for _, c in groups])
    scale = torch.stack([nat[c].sum() for _, c in groups])
    got = torch.stack([(energies[c].float().sum().double() if fp32_sum else energies[c].double().sum()) for _, c in groups])
    return ((got - want).abs() / scale / cc.U)


# (n raised where the two-term worst record of 300 chains came close: 19 U at dim 254, 25 U at dim 512, 2.7 U at 132 dims)
RECORD_ENERGY_SAMPLE = \
    [_case("langevin", "gauss", d, n=n) for d, n in ((10, 320), (21, 300), (64, 300), (200, 300), (254, 1000), (512, 1000))] + \
    [_case("langevin", "gmm", d, K, n=n) for d, K, n in ((21, 8, 300), (64, 16, 300), (132, 12, 1000), (200, 12, 1000))] + \
    [_case("hmc", "gauss", d, mass=m) for d, m in ((21, "none"), (64, "scalar"), (200, "none"), (256, "diag"))] + \
    [_case("hmc", "gmm", d, K, mass=m) for d, K, m in ((64, 16, "none"), (94, 8, "none"))]


@pytest.mark.parametrize("case", RECORD_ENERGY_SAMPLE, ids=lambda c: c.id)
def test_record_energy_bars(case):
    """K_REC_GAUSS / K_REC_GMM: fp32 energies (the oracle's; for mixtures also the kernels' expansion in fp32) summed in fp32
    over a record's chains meet the bar in EVERY record; energies from two-term bf16 operands miss it in some record."""
    fp = cc.cpu_params(case)
    x = kept_state32(case, fp)
    layout = cc.wave_layout(case.n, case.dim)
    k = cc.K_REC_GAUSS if case.energy == "gauss" else cc.K_REC_GMM
    r32 = record_energy_ratios(case, layout, fp, x, cc._oracle32(case, fp).energy(x), True)
    r2 = record_energy_ratios(case, layout, fp, x, energy_split2(case, x, fp), False)
    print(f"{case.id}: fp32 worst record {r32.max().item():.2f} U, two-term worst record {r2.max().item():.1f} U", end="")
    assert r32.max().item() < k, "the fp32 oracle misses the bar in some record"
    if case.energy != "gauss":
        rx = record_energy_ratios(case, layout, fp, x, gmm_energy_expansion32(x, fp), True)
        print(f", fp32 expansion {rx.max().item():.2f} U", end="")
        assert rx.max().item() < k, "the expansion in fp32 misses the bar in some record"
    print()
    assert r2.max().item() > k, "two-term bf16 energies pass the bar in every record"


@pytest.mark.parametrize("case,chains", [(cc.Case("langevin", "gauss", 516, n=200, family="langevin_chain_rows_kernel"), 1),
                                         (cc.Case("heun", "gauss", 64, family="langevin_heun_rows_kernel"), 16),
                                         (cc.Case("hmc", "gauss", 260, family="hmc_chain_kernel"), 1),
                                         (cc.Case("hmc", "gmm", 95, K=8, family="hmc_chain_kernel"), 2)], ids=lambda c: getattr(c, "id", c))
def test_lane_group_record_energy_bar(case, chains):
    """records of a few chains (the lane-group kernels): the chain's own bar, k_record_energy -- met by the fp32 oracle; two-term
    operands would miss it for the Gaussians (those kernels have no split contraction to lose a term of)."""
    fp = cc.cpu_params(case)
    x = kept_state32(case, fp) if case.sampler != "heun" else cc.langevin_ref32(case, cc.langevin_x0(case, fp), fp, 0.25)
    layout = cc.rows_layout(case.n, case.dim, chains)
    k = cc.k_record_energy(case, layout)
    r32 = record_energy_ratios(case, layout, fp, x, cc._oracle32(case, fp).energy(x), True)
    r2 = record_energy_ratios(case, layout, fp, x, energy_split2(case, x, fp), False)
    print(f"{case.id}: bar {k} U, fp32 worst record {r32.max().item():.2f} U, two-term worst record {r2.max().item():.1f} U")
    assert r32.max().item() < k
    assert case.energy != "gauss" or r2.max().item() > k


def tree_sum32(v):
    """fp32 sum over dim 0 as a wave adds its 32 lanes: five levels of pairs"""
    v = torch.cat([v, v.new_zeros(32 - v.shape[0], v.shape[1])])
    while v.shape[0] > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def seq_sum32(v):
    """... as diag::emit adds a slot's rows: one after the other"""
    acc = v.new_zeros(v.shape[1])
    for row in v:
        acc = acc + row
    return acc


def far_population():
    """tests/test_diag_gpu.py test_population_far_from_the_origin: mean ~ 1000, std ~ 0.05"""
    return 1000.0 + 0.05 * torch.randn(2000, 16, generator=torch.Generator().manual_seed(0))


@pytest.mark.parametrize("what", ["wave", "emit"])
@pytest.mark.parametrize("population", ["wide", "far"])
def test_record_sum_and_m2_bars(population, what):
    """sums_bar / m2_bar are derived from the addition depth (chain_cases.py), not measured: an fp32 two-pass emulation in the
    kernels' order meets them in every slot of every record; the one-pass sum x^2 - (sum x)^2 / m misses the M2 bar on the
    far-from-origin population."""
    if population == "wide":
        case = _case("langevin", "gauss", 64, n=300)
        x = cc.langevin_x0(case, cc.cpu_params(case))
    else:
        x = far_population()
    n, dim = x.shape
    layout, depth, add = (cc.wave_layout(n, dim), 5, tree_sum32) if what == "wave" else (cc.rows_layout(n, dim, 16), 16, seq_sum32)
    if what == "wave" and dim == 16:
        layout, depth = (cc.record_count(dim, 32 * dim, n, dim), dim, 32 * dim), 5
    refs = cc.record_refs(layout, n, dim, x, torch.zeros(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64))
    worst_sum = worst_m2 = worst_one = 0.0
    for b, idx in enumerate(cc.record_chains(layout, n, dim)):
        v = x.flatten()[idx]
        m = v.shape[0]
        s = add(v)
        mean = s * (torch.tensor(1.0) / m)
        dv = v - mean
        m2 = add(dv * dv)
        one = add(v * v) - s * s / m
        sb = cc.sums_bar(depth, refs.abs_sums[b])
        mb = cc.m2_bar(depth, refs.cnt[b], refs.abs_sums[b], refs.m2[b])
        worst_sum = max(worst_sum, ((s.double() - refs.sums[b]).abs() / sb).max().item())
        worst_m2 = max(worst_m2, ((m2.double() - refs.m2[b]).abs() / mb).max().item())
        worst_one = max(worst_one, ((one.double() - refs.m2[b]).abs() / mb).max().item())
    print(f"{population} {what}: sums at {worst_sum:.3f} of the bar, two-pass M2 at {worst_m2:.3f}, one-pass M2 at {worst_one:.3g}")
    assert worst_sum < 1.0 and worst_m2 < 1.0
    if population == "far":
        assert worst_one > 1.0, "a one-pass M2 passes the bar far from the origin"


@pytest.mark.parametrize("dim,n", [(21, 300), (64, 129), (10, 320), (254, 33), (516, 31), (64, 1)])
def test_merge_of_exact_records_is_the_population_statistic(dim, n):
    """cc.merge_records64 (the reference ebm_diag_finish_f32 is held to) on records filled from cc.record_refs gives the
    population's mean, biased variance and mean energy, whichever geometry cut the population into records"""
    g = torch.Generator().manual_seed(dim + n)
    x = (3.0 + torch.randn(n, dim, generator=g, dtype=torch.float64)).float()
    e = torch.randn(n, generator=g, dtype=torch.float64)
    mask = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
    for nn, layout in record_geometries(n, dim):
        if nn != n:
            continue
        nb, S, E = layout
        refs = cc.record_refs(layout, n, dim, x, e, e.abs(), mask)
        rec = torch.zeros(1, nb, 2 * S + 8, dtype=torch.float64)
        rec[0, :, :S], rec[0, :, S:2 * S] = refs.sums, refs.m2
        for (rs, _), en, acc in zip(refs.groups, refs.energy, refs.accepts):
            rec[0, rs[0], 2 * S + 1], rec[0, rs[-1], 2 * S + 6] = en, acc
        mean, var, energy, accept = cc.merge_records64(rec, layout, n, dim)
        W = max(S, dim)
        rows = x.double().view(-1, W)
        torch.testing.assert_close(mean[0], rows.mean(dim=0), rtol=1e-12, atol=0)
        want_var = rows.var(dim=0, unbiased=False).clamp(1e-10, 1e10) if rows.shape[0] > 1 else torch.zeros(W, dtype=torch.float64)
        torch.testing.assert_close(var[0], want_var, rtol=1e-9, atol=0)
        torch.testing.assert_close(energy[0], e.sum() / rows.shape[0], rtol=1e-12, atol=1e-15)
        assert accept[0].item() == pytest.approx(mask.sum().item() / rows.shape[0], rel=1e-12)
