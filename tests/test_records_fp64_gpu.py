"""The diagnostics records of every fused chain route against float64, record by record (tests/chain_cases.py ROUTES, the
records=True cases).

return_diagnostics=True is served by records the chain kernels write themselves: per kept step and workgroup -- per wave of
32 chains in the matrix-layout kernels -- the column sums, the centred second moments, four shares of the energy sum and four
of the accept count; ebm_diag_finish_f32 merges them.  The merged statistics cannot tell which record a chain was counted in,
and an energy from a two-term bf16 contraction can sit closer to float64 in the mean than fp32 does.  Here every record is read:
  * which chains it holds is cc.record_chains, written from the documented geometry (include/ebm_hip.h, ebm_diag_layout);
  * its sums, M2 and energy share are compared with float64 of the state the kernel itself returned (so the state's own
    error, which tests/test_fp64_one_step_gpu.py bars, stays out), at bars set on the CPU (tests/test_fp64_bars.py): the sums
    and M2 from the addition depth, the energy share between what fp32 and what two-term bf16 operands reach per record;
  * its accept shares equal the accept mask's count over its chains;
  * ebm_diag_finish_f32 on the same buffer equals an exact float64 merge of the raw records to the fp32 rounding of the result.
One kept step with the one-step tests' inputs, the accept-decision setup (records describe the state AFTER the accept), then
several kept steps against the trajectory: a kept middle step, a kept last step, and a last step that is not kept.

Measured on an MI355X (worst record of every case a family runs here; the energy share in U of sum N(E) against its bar,
sums and M2 as fractions of their bars):
  matrix_langevin_diag_kernel 5.8 of 16 (sums 0.50, M2 0.57)     gauss_shift_langevin_diag_kernel 3.6 of 16 (0.43, 0.58)
  gauss_res_langevin_kernel<true,..> 2.3 .. 2.8 of 16 (0.60, 0.63)   gauss_big_langevin_kernel<1|2,true,..> 2.1 .. 5.0 of 16 (0.55, 0.62)
  gmm_shift_ / gmm_wide_langevin_diag_kernel 0.10 of 2 (0.38, 0.43)
  gauss_hmc_mfma_kernel DIAG=true: GaussE 1.9 / 2.4 (shifted) of 16, GaussStreamE 2.5 / 3.6 (shifted) of 16, GmmE 0.34 / 0.22 of 2
  lane-group: langevin_chain_rows_kernel 17 of 47 (516 dims), hmc_chain_kernel 10 of 45, langevin_heun_rows_kernel 3.4 of 39
Mutation checks (neither committed): with the contraction of the records' energy in matrix_langevin_diag_kernel cut to two
pieces per operand, that family's Gaussian cases fail the energy share at 22 .. 29 U; with record_chains putting class s + 1
where s belongs, every interleaved-class case fails the sums."""

import dataclasses

import pytest
import torch

import chain_cases as cc

pytestmark = pytest.mark.gpu

RECORDS = [c for c in cc.ROUTES if c.records]
LANGEVIN = [c for c in RECORDS if c.sampler != "hmc"]
HMC = [c for c in RECORDS if c.sampler == "hmc"]
HMC_CLAMP = 1e10  # the HMC records' energy clamp (include/ebm_hip.h: "mean clamped energy")


def check_records(case, layout, rec, x, fp, mask, what):
    """every record of one kept step (rec [n_blocks, 2 S + 8]) against the float64 references of the state x (which it
    returns); prints the worst ratios to the bars (sums, M2: of the bar; energy: in U of its natural scale)."""
    n, dim = case.n, case.dim
    nb, S, E = layout
    assert nb == cc.record_count(S, E, n, dim) and tuple(rec.shape) == (nb, 2 * S + 8), (case.id, layout, rec.shape)
    assert torch.isfinite(rec).all(), (case.id, what)
    e64, nat = cc.energy64(case, x, fp)
    refs = cc.record_refs(layout, n, dim, x, e64, nat, mask, HMC_CLAMP if case.sampler == "hmc" else None)
    depth = cc.record_depth(case, layout)
    r = rec.double()
    tiny = torch.finfo(torch.float64).tiny  # (a slot without elements: reference 0, bar 0, the record must hold 0)
    sum_ratio = (r[:, :S] - refs.sums).abs() / (cc.sums_bar(depth, refs.abs_sums) + tiny)
    m2_ratio = (r[:, S:2 * S] - refs.m2).abs() / (cc.m2_bar(depth, refs.cnt, refs.abs_sums, refs.m2) + tiny)
    b, s = divmod(int(sum_ratio.argmax()), S)
    assert sum_ratio.max().item() <= 1.0, (case.id, what, "sum of record", b, "slot", s, sum_ratio.max().item(), "of the bar")
    b, s = divmod(int(m2_ratio.argmax()), S)
    assert m2_ratio.max().item() <= 1.0, (case.id, what, "M2 of record", b, "slot", s, m2_ratio.max().item(), "of the bar")
    shares = torch.stack([r[rs, 2 * S:2 * S + 4].sum() for rs, _ in refs.groups])
    accepts = torch.stack([r[rs, 2 * S + 4:2 * S + 8].sum() for rs, _ in refs.groups])
    e_ratio = (shares - refs.energy).abs() / (cc.U * refs.energy_scale + tiny)
    k = cc.k_record_energy(case, layout)
    print(f"RECORDS {case.id} [{case.family}] {what}: layout {layout}, sums {sum_ratio.max().item():.3f} and M2 "
          f"{m2_ratio.max().item():.3f} of the bar, energy share {e_ratio.max().item():.2f} U (bar {k:g} U)")
    g = int(e_ratio.argmax())
    assert e_ratio.max().item() <= k, (case.id, what, "energy share of records", refs.groups[g][0], e_ratio.max().item(), "U, bar", k)
    assert torch.equal(accepts, refs.accepts.double()), (case.id, what, "accept shares", (accepts - refs.accepts).abs().max().item())
    return refs


def check_finish(case, run, dev, accept):
    """ebm_diag_finish_f32 against the exact float64 merge of the same raw records: the kernel merges in fp64, so only the
    fp32 rounding of each result (and the documented clamp of the variance, which the reference applies too) separates them"""
    mean, var, energy, acc = cc.diag_finish(run, case.n, case.dim, dev, accept)
    want = cc.merge_records64(run.rec, run.layout, case.n, case.dim)
    for name, got, ref in zip(("mean", "var", "energy", "acceptance"), (mean, var, energy, acc), want):
        if got is None:
            continue
        err = (got.double() - ref).abs()
        bar = cc.U * ref.abs() * (1 + 1e-6)
        assert (err <= bar).all(), (case.id, "ebm_diag_finish_f32", name, (err / ref.abs().clamp(min=1e-300)).max().item() / cc.U, "U")


def langevin_eta(case):
    return 0.25 if case.energy == "gauss" else 0.5


@pytest.mark.parametrize("noise_field", [False, True], ids=["fast", "noise"])
@pytest.mark.parametrize("case", LANGEVIN, ids=lambda c: c.id)
def test_langevin_records_of_one_kept_step(cuda_device, case, noise_field):
    _, spec, fp = cc.device_model(case, cuda_device)
    x0 = cc.langevin_x0(case, fp)
    run = cc.run_langevin(case, spec, x0, langevin_eta(case), noise_field, cuda_device)
    check_records(case, run.layout, run.rec[0], run.x, fp, None, "noise field" if noise_field else "noise-free")
    check_finish(case, run, cuda_device, accept=False)


def hmc_setup(case, dev):
    _, spec, fp = cc.device_model(case, dev)
    x0, p, mass = cc.hmc_inputs(case, fp)
    return spec, fp, x0, p, mass


@pytest.mark.parametrize("case", HMC, ids=lambda c: c.id)
def test_hmc_records_of_one_kept_transition(cuda_device, case):
    spec, fp, x0, p, mass = hmc_setup(case, cuda_device)
    eps = cc.hmc_eps(case, x0, p, mass, fp, target=1.0 if case.energy == "gauss" else cc.GMM_FORCE_TARGET)
    run = cc.run_hmc(case, spec, x0, p, torch.zeros(case.n), mass, eps, cuda_device)
    assert bool((run.mask[0] == 1).all()), "u = 0 accepts every proposal"
    check_records(case, run.layout, run.rec[0], run.x, fp, run.mask[0], "u = 0")
    check_finish(case, run, cuda_device, accept=True)


@pytest.mark.parametrize("case", HMC, ids=lambda c: c.id)
def test_hmc_records_describe_the_state_after_the_accept(cuda_device, case):
    """the accept-decision setup of tests/test_fp64_one_step_gpu.py: a near even mix of accepted and rejected chains.  A
    record holds x0 and E(x0) for a rejected chain, the proposal and its energy for an accepted one."""
    spec, fp, x0, p, mass = hmc_setup(case, cuda_device)
    x0 = cc.hmc_accept_x0(case, x0, fp)
    eps = cc.hmc_accept_eps(case, x0, p, mass, fp)
    h0, h1, n0, n1 = cc.hmc_hamiltonians64(case, x0, p, mass, fp, eps)
    keep, u, below = cc.accept_draws(h0, h1, n0, n1)
    x1 = cc.run_hmc(case, spec, x0, p, torch.zeros(case.n), mass, eps, cuda_device).x  # the kernel's own proposals
    run = cc.run_hmc(case, spec, x0, p, u, mass, eps, cuda_device)
    mask = run.mask[0]
    assert bool(((mask == 0) | (mask == 1)).all())
    state = torch.where(mask.bool()[:, None], x1, x0)
    assert torch.equal(run.x, state), (case.id, "the returned state is not where(mask, x1, x0)")
    # energies of the two outcomes differ by far more than the bar, so a record of the proposal's energy would show
    refs = check_records(case, run.layout, run.rec[0], state, fp, mask, "accept decisions")
    both = [int(a) for (_, c), a in zip(refs.groups, refs.accepts) if 0 < int(a) < len(c)]
    assert both, (case.id, "no record holds both an accepted and a rejected chain")
    e1, nat1 = cc.energy64(case, x1, fp)
    e0, _ = cc.energy64(case, x0, fp)
    rejected = ~mask.bool()
    k = cc.k_record_energy(case, run.layout)
    moved = torch.stack([((e1 - e0) * rejected)[c].sum().abs() / (cc.U * nat1[c].sum()) for _, c in refs.groups])
    assert (moved > 4 * k).any(), (case.id, "the rejected proposals' energies are within the bar of the kept states'", moved.max().item())
    check_finish(case, run, cuda_device, accept=True)


RAGGED = [c for c in RECORDS if (c.sampler, c.energy, c.dim) in {("langevin", "gauss", 21), ("langevin", "gauss", 64), ("langevin", "gauss", 254),
                                                               ("langevin", "gmm", 127), ("langevin", "gmm", 132), ("hmc", "gauss", 21),
                                                               ("hmc", "gauss", 200), ("hmc", "gmm", 94), ("hmc", "gmm", 95)} and c.image]


@pytest.mark.parametrize("n", [1, 33, 129])
@pytest.mark.parametrize("case", RAGGED, ids=lambda c: c.id)
def test_ragged_and_empty_records(cuda_device, case, n):
    """a ragged last record counts only its valid chains; a record past the last chain (an alignment class without chains, at
    n = 1 three of the four) holds nothing.  Whatever family these chain counts route to, its layout is the one asked for."""
    case = dataclasses.replace(case, n=n)
    if case.sampler == "hmc":
        spec, fp, x0, p, mass = hmc_setup(case, cuda_device)
        eps = cc.hmc_eps(case, x0, p, mass, fp, target=1.0 if case.energy == "gauss" else cc.GMM_FORCE_TARGET)
        run = cc.run_hmc(case, spec, x0, p, torch.full((n,), 0.5), mass, eps, cuda_device)
        mask = run.mask[0]
    else:
        _, spec, fp = cc.device_model(case, cuda_device)
        x0 = cc.langevin_x0(case, fp)
        run, mask = cc.run_langevin(case, spec, x0, langevin_eta(case), False, cuda_device), None
    refs = check_records(case, run.layout, run.rec[0], run.x, fp, mask, f"n = {n}")
    if run.layout[2] < 0 and n == 1:
        assert sum(len(c) == 0 for _, c in refs.groups) == cc.diag_classes(case.dim) - 1
    check_finish(case, run, cuda_device, accept=case.sampler == "hmc")


# ----------------------------------------------------------------------------------------------------------------
# several kept steps
# ----------------------------------------------------------------------------------------------------------------
def same_family_without_records(case):
    """whether ROUTES sends the same call without a record buffer to the same kernel family"""
    for c in cc.ROUTES:
        if not c.records and dataclasses.replace(c, records=True, launcher=case.launcher, family=case.family, family_noise=case.family_noise) == case:
            return c.family == case.family
    return False


def stable_eta(case, fp):
    """a step the chain is stable at for several steps (the one-step eta of the Gaussians, 0.25, is far past the stiffest
    direction's limit): 1 / max_i sum_j |P_ij| >= 1 / lambda_max, so the stiff directions still move by O(1) of themselves per
    step and consecutive states have energies far apart on the bar's scale (asserted below)."""
    if case.energy != "gauss":
        return 0.5
    return float((1.0 / fp[1].double().abs().sum(dim=1).max()).float())


def check_kept_steps(case, run, fp, masks, what):
    """record j against trajectory slice j; the slices' energies are far enough apart for a share that landed in the wrong
    step's record, or described a state one step off, to show"""
    kept = run.traj.shape[1]
    assert run.rec.shape[0] == kept
    k = cc.k_record_energy(case, run.layout)
    for j in range(kept):
        xj = run.traj[:, j].contiguous()
        refs = check_records(case, run.layout, run.rec[j], xj, fp, None if masks is None else masks[j], f"{what}, kept step {j}")
        other = run.traj[:, j + 1].contiguous() if j + 1 < kept else (run.traj[:, j - 1].contiguous() if torch.equal(run.x, xj) else run.x)
        eo, _ = cc.energy64(case, other, fp)
        if case.sampler == "hmc":
            eo = eo.clamp(-HMC_CLAMP, HMC_CLAMP)
        apart = torch.stack([(eo[c].sum() - e).abs() / (cc.U * s) for (_, c), e, s in zip(refs.groups, refs.energy, refs.energy_scale) if len(c)])
        assert (apart > 4 * k).float().mean().item() > 0.5, (case.id, what, j, "neighbouring states' record energies are not apart", apart.median().item())


@pytest.mark.parametrize("k,thin", [(4, 2), (3, 2)], ids=["k4-thin2", "k3-thin2"])
@pytest.mark.parametrize("case", LANGEVIN, ids=lambda c: c.id)
def test_langevin_records_of_several_kept_steps(cuda_device, case, k, thin):
    """k = 4, thin = 2: a kept step in the middle and a kept last step; k = 3, thin = 2: a kept middle step and a last step that
    is not kept -- where a kernel writes a record's energy share one evaluation late (the streamed-Ps kernels), the share of
    the kept step must still land."""
    _, spec, fp = cc.device_model(case, cuda_device)
    x0 = cc.langevin_x0(case, fp)
    eta = stable_eta(case, fp)
    run = cc.run_langevin(case, spec, x0, eta, False, cuda_device, k=k, thin=thin, traj=True)
    assert torch.isfinite(run.traj).all() and torch.isfinite(run.x).all()
    if k % thin == 0:
        assert torch.equal(run.traj[:, -1], run.x)
    check_kept_steps(case, run, fp, None, f"k = {k}, thin = {thin}")
    check_finish(case, run, cuda_device, accept=False)
    if same_family_without_records(case):
        plain = cc.run_langevin(case, spec, x0, eta, False, cuda_device, k=k, thin=thin, traj=True, records=False)
        assert torch.equal(plain.traj, run.traj) and torch.equal(plain.x, run.x), (case.id, "records change the chain")


def eps_with_rejections(case, x0, p, mass, fp):
    """the accept-decision step size, doubled (the mixtures' is so small that every proposal is accepted) until a tenth of
    the chains lose at least half their acceptance probability over one leapfrog step in float64"""
    eps = cc.hmc_accept_eps(case, x0, p, mass, fp)
    for _ in range(12):
        h0, h1, _, _ = cc.hmc_hamiltonians64(case, x0, p, mass, fp, eps)
        if ((h1 - h0) > 0.7).float().mean().item() >= 0.1:
            break
        eps = float(torch.tensor(eps * 2.0, dtype=torch.float32).item())
    return eps


@pytest.mark.parametrize("case", HMC, ids=lambda c: c.id)
def test_hmc_records_of_several_kept_transitions(cuda_device, case):
    """T = 2 transitions of L = 2 leapfrog steps, every one kept, with injected momenta and uniforms (accepts and rejects)"""
    spec, fp, x0, p, mass = hmc_setup(case, cuda_device)
    x0 = cc.hmc_accept_x0(case, x0, fp)
    g = cc._gen(case, 31)
    T, L = 2, 2
    ps = torch.randn(T, case.n, case.dim, generator=g)
    eps = eps_with_rejections(case, x0, ps[0], mass, fp)
    u = torch.rand(T, case.n, generator=g)
    run = cc.run_hmc(case, spec, x0, ps, u, mass, eps, cuda_device, T=T, L=L, thin=1, traj=True)
    assert torch.isfinite(run.traj).all() and torch.equal(run.traj[:, -1], run.x)
    assert bool(((run.mask == 0) | (run.mask == 1)).all()) and 0 < int(run.mask.sum()) < T * case.n
    for j in range(T):  # a rejected chain keeps its state
        prev = x0 if j == 0 else run.traj[:, j - 1]
        assert torch.equal(run.traj[:, j][run.mask[j] == 0], prev[run.mask[j] == 0])
    check_kept_steps(case, run, fp, run.mask, f"T = {T}, L = {L}")
    check_finish(case, run, cuda_device, accept=True)
    if same_family_without_records(case):
        plain = cc.run_hmc(case, spec, x0, ps, u, mass, eps, cuda_device, T=T, L=L, thin=1, traj=True, records=False)
        assert torch.equal(plain.traj, run.traj) and torch.equal(plain.x, run.x) and torch.equal(plain.mask, run.mask), (case.id, "records change the chain")
