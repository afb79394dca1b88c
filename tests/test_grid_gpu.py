"""The HIP kernels against the reference's recorded runs on the SURVEY.md section 8c grid (tests/golden/grid): every
energy x {Langevin k = 16, HMC L = 5 / 20} x dim in {2, 32, 64, 100} at n = 1000, scheduled step sizes, scalar and
diagonal masses.  Through the C ABI with the draws the reference consumed (replayed from the seeds); the diagnostics
come from the in-kernel records.  Bars: element-wise Langevin bit-exact (sha256 of the whole state), coupled energies
3e-5, HMC accept masks bit-identical and states 5e-4 (per chain: >= 99 % of them, 5e-3 all) with an fp64 referee beside it on the quartic well, diagnostics 1e-4 (they are fp64 merges against fp32 torch sums)."""

import os

import pytest
import torch

import torchebm_amd as ta
from helpers import grid_inputs, grid_names, load_grid, mass_to, package_model, sha16
from torchebm_amd import _lib
from torchebm_amd.integrators.symplectic import _mass_args
from torchebm_amd.samplers.langevin import em_coefficients

pytestmark = pytest.mark.gpu


def _records(desc, sampler, n, dim, n_kept, dev, injected=True):
    layout = _lib.diag_layout(desc, sampler, n, dim, injected, False)
    assert layout is not None
    nb, S, E = layout
    rec = torch.empty(n_kept * nb * (2 * S + 8), device=dev)
    work = torch.zeros(n_kept * (3 * max(S, dim) + 3), dtype=torch.float64, device=dev)
    return layout, rec, work


def _finish(layout, rec, work, n, dim, n_kept, dev, with_accept):
    nb, S, E = layout
    # S > dim: PACKED rows (include/ebm_hip.h, ebm_diag_layout): the records are those of n / pack rows of width pack * dim,
    # merged as such; the `pack` columns of every coordinate are pooled afterwards (within + between-group variance)
    pack = S // dim if S > dim else 1
    m_n, m_dim = n // pack, dim * pack
    out = {"mean": torch.empty(n_kept, m_dim, device=dev), "var": torch.empty(n_kept, m_dim, device=dev),
           "energy": torch.empty(n_kept, device=dev)}
    if with_accept:
        out["acceptance_rate"] = torch.empty(n_kept, device=dev)
    _lib.call("ebm_diag_finish_f32", rec.data_ptr(), n_kept, nb, S, E, m_n, m_dim, out["mean"].data_ptr(), out["var"].data_ptr(),
              out["energy"].data_ptr(), _lib.ptr(out.get("acceptance_rate")), work.data_ptr(), _lib.stream_handle(dev))
    if pack > 1:
        gm = out["mean"].view(n_kept, pack, dim).double()
        mean = gm.mean(dim=1)
        var = out["var"].view(n_kept, pack, dim).double().mean(dim=1) + (gm - mean.unsqueeze(1)).square().mean(dim=1)
        out["mean"], out["var"], out["energy"] = mean.float(), var.float().clamp(1e-10, 1e10), out["energy"] / pack
    return {k: v.cpu() for k, v in out.items()}


def _state_pass_diagnostics(desc, x, nz, table, rows, n, dim, k, thin, dev):
    n_kept = k // thin
    out = {"mean": torch.empty(n_kept, dim, device=dev), "var": torch.empty(n_kept, dim, device=dev), "energy": torch.empty(n_kept, device=dev)}
    work = torch.zeros(2 * dim + 1, dtype=torch.float64, device=dev)
    energy = torch.empty(n, device=dev)
    st = _lib.stream_handle(dev)
    for keep in range(n_kept):
        s0 = keep * thin
        _lib.call("ebm_langevin_chain_f32", desc, x.data_ptr(), n, dim, thin, rows[s0][0], rows[s0][1], rows[s0][2], table[s0:].data_ptr(),
                  0, 0.0, 0.0, thin, None, None, nz[s0:].data_ptr(), 0, 0, st)
        _lib.call("ebm_chain_stats_f32", x.data_ptr(), n, dim, out["mean"][keep].data_ptr(), out["var"][keep].data_ptr(), work.data_ptr(), st)
        _lib.call("ebm_energy_grad_f32", desc, x.data_ptr(), n, dim, energy.data_ptr(), None, st)
        out["energy"][keep] = energy.mean()
    if n_kept * thin < k:
        s0 = n_kept * thin
        _lib.call("ebm_langevin_chain_f32", desc, x.data_ptr(), n, dim, k - s0, rows[s0][0], rows[s0][1], rows[s0][2], table[s0:].data_ptr(),
                  0, 0.0, 0.0, thin, None, None, nz[s0:].data_ptr(), 0, 0, st)
    return {key: v.cpu() for key, v in out.items()}


def _check_diag(got, want, keys):
    for key in keys:
        torch.testing.assert_close(got[key], want[key], rtol=1e-4, atol=1e-5, msg=lambda m, key=key: f"{key}: {m}")


@pytest.mark.parametrize("name", grid_names("ld_"))
def test_langevin_grid(cuda_device, name):
    fx = load_grid(name)
    x0, noise = grid_inputs(fx)
    n, dim, k, thin = fx["n"], fx["dim"], fx["k"], fx["thin"]
    model = package_model(fx["energy"], cuda_device)
    desc = model.fused_spec().to_c()
    rows = [em_coefficients(e, s) for e, s in zip(fx["etas"], fx["sigmas"])]
    table = torch.tensor([(r[0], r[1], r[2], 0.0) for r in rows], dtype=torch.float32, device=cuda_device)
    x, nz = x0.to(cuda_device), noise.to(cuda_device)
    if _lib.diag_layout(desc, _lib.DIAG_LANGEVIN, n, dim, True, False) is None:
        # no in-kernel records (dense Gaussians above 128 dims, csrc/gauss_big.hip): `thin` steps per launch and the
        # statistics from the state, as the sampler does (samplers/_chain_host.py, run_with_state_passes)
        diag = _state_pass_diagnostics(desc, x, nz, table, rows, n, dim, k, thin, cuda_device)
    else:
        layout, rec, work = _records(desc, _lib.DIAG_LANGEVIN, n, dim, k // thin, cuda_device)
        _lib.call("ebm_langevin_chain_f32", desc, x.data_ptr(), n, dim, k, rows[0][0], rows[0][1], rows[0][2], table.data_ptr(),
                  0, 0.0, 0.0, thin, None, rec.data_ptr(), nz.data_ptr(), 0, 0, _lib.stream_handle(cuda_device))
        diag = _finish(layout, rec, work, n, dim, k // thin, cuda_device, False)
    got = x.cpu()
    if fx["energy"]["kind"] in ("double_well", "harmonic"):
        assert sha16(got) == fx["ref"]["sha_x"]  # all 1000 x dim values bit-identical to the reference
    else:
        torch.testing.assert_close(got[:256], fx["ref"]["x_rows"], rtol=3e-5, atol=3e-5)
    _check_diag(diag, fx["ref"]["diagnostics"], ("mean", "var", "energy"))
    # the same run without records (for the Gaussian: the matrix-core kernel where it applies)
    x2 = x0.to(cuda_device)
    _lib.call("ebm_langevin_chain_f32", desc, x2.data_ptr(), n, dim, k, rows[0][0], rows[0][1], rows[0][2], table.data_ptr(),
              0, 0.0, 0.0, thin, None, None, nz.data_ptr(), 0, 0, _lib.stream_handle(cuda_device))
    torch.testing.assert_close(x2.cpu()[:256], fx["ref"]["x_rows"], rtol=3e-5, atol=3e-5)


def _referee(name, got_rows, ref_rows, n_leapfrog, coupled):
    """Beside the flat tolerance, an fp64 yardstick for EVERY HMC fixture (tests/golden/make_referee.py: the same transitions in
    float64 on the same draws and accept decisions; round 4 had it for the quartic well only).  The kernel must be as close to
    the fp64 chain as the reference's own fp32 arithmetic is:
      * element-wise energies (quartic well, harmonic): population median error <= the reference's, 99th percentile <= 2 x,
        maximum <= 4 x (measured on MI355X: medians 0.5 - 0.8 x -- fused multiply-adds round once where the eager ops round
        twice); per chain err_hip <= 4 x the chain's yardstick at L = 5, 16 x at L = 20 (160 steps in the well amplify ONE
        differing rounding by up to 1e4, and which chain draws it is independent between two fp32 runs), the yardstick being
        the reference's error on that chain with the population's median reference error as its floor;
      * row-coupled energies (dense Gaussian, mixtures): the row contraction sums in another order than torch's bmm / logsumexp
        (split-bf16 products accumulated in fp32 on the matrix pipe, lane-group reductions), so neither fp32 run is the other's
        rounding: median <= 1.5 x the reference's, 99th percentile <= 2 x, maximum <= 4.5 x; per chain 6 x / 32 x.  Measured over
        the 20 coupled fixtures: medians 0.3 - 1.45 x, 99th percentiles 0.25 - 1.6 x, maxima 0.4 - 4.2 x, per chain up to 5.1 (L = 5)
        and 22.8 (L = 20: mixture chains near a tie between two components -- in a fixture whose population figures are all
        BELOW the reference's)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_referee", name + ".pt")
    assert os.path.exists(path), f"no fp64 referee for {name}: run tests/golden/make_referee.py"
    f64 = torch.load(path, weights_only=False)["x_rows_f64"]
    err_ref = (ref_rows.double() - f64).abs().amax(dim=1)
    err_hip = (got_rows.double() - f64).abs().amax(dim=1)
    ratio = err_hip / torch.maximum(err_ref, err_ref.median())
    q = lambda t, f: float(t.double().quantile(f))  # noqa: E731
    stats = {"name": name, "hip": [q(err_hip, 0.5), q(err_hip, 0.99), float(err_hip.max())],
             "ref": [q(err_ref, 0.5), q(err_ref, 0.99), float(err_ref.max())], "ratio_max": float(ratio.max())}
    k_med, k_p99, k_max = (1.5, 2.0, 4.5) if coupled else (1.0, 2.0, 4.0)
    assert stats["hip"][0] <= k_med * stats["ref"][0] and stats["hip"][1] <= k_p99 * stats["ref"][1] and stats["hip"][2] <= k_max * stats["ref"][2], stats
    per_chain = (6.0 if n_leapfrog <= 5 else 32.0) if coupled else (4.0 if n_leapfrog <= 5 else 16.0)
    assert stats["ratio_max"] <= per_chain, stats


@pytest.mark.parametrize("name", grid_names("hmc"))
def test_hmc_grid(cuda_device, name):
    fx = load_grid(name)
    x0, p, u = grid_inputs(fx)
    n, dim, T, L, thin = fx["n"], fx["dim"], fx["T"], fx["L"], fx["thin"]
    model = package_model(fx["energy"], cuda_device)
    desc = model.fused_spec().to_c()
    eps = fx["eps"]
    table = torch.tensor(eps, dtype=torch.float32, device=cuda_device) if len(set(eps)) > 1 else None
    p_d, u_d = p.to(cuda_device), u.to(cuda_device)
    mass = mass_to(fx["mass"], cuda_device)

    def run(records):
        x = x0.to(cuda_device)
        mask = torch.empty(T, n, dtype=torch.uint8, device=cuda_device)
        kind, ms, md = _mass_args(mass, x)
        _lib.call("ebm_hmc_chain_f32", desc, x.data_ptr(), n, dim, T, L, eps[0], _lib.ptr(table), kind, ms, _lib.ptr(md), thin, None,
                  _lib.ptr(records), mask.data_ptr(), None, p_d.data_ptr(), u_d.data_ptr(), 0, 0, _lib.stream_handle(cuda_device))
        return x.cpu(), mask.cpu().bool()

    layout, rec, work = _records(desc, _lib.DIAG_HMC, n, dim, T // thin, cuda_device)
    got, mask = run(rec)
    diag = _finish(layout, rec, work, n, dim, T // thin, cuda_device, True)
    assert torch.equal(mask, fx["accepted"])  # all 8 x 1000 accept / reject decisions identical to the reference's
    scale = fx["ref"]["x_rows"].abs().clamp(min=1.0)

    def check_states(x):
        # per chain; 160 leapfrog steps in the quartic well amplify a last-bit difference of one chain in a few
        # hundred by 1e4, so the bar is 5e-4 for >= 99 % of the chains and 5e-3 for every one
        err = ((x[:256] - fx["ref"]["x_rows"]).abs() / scale).amax(dim=1)
        assert (err <= 5e-4).float().mean().item() >= 0.99 and err.max().item() <= 5e-3, (err.max().item(), (err > 5e-4).sum().item())

    check_states(got)
    coupled = fx["energy"]["kind"] in ("gaussian", "gmm")
    _referee(name, got[:256], fx["ref"]["x_rows"], L, coupled)
    assert torch.equal(diag["acceptance_rate"], fx["ref"]["diagnostics"]["acceptance_rate"])
    _check_diag(diag, fx["ref"]["diagnostics"], ("mean", "energy"))
    torch.testing.assert_close(diag["var"], fx["ref"]["diagnostics"]["var"], rtol=2e-3, atol=1e-5)
    # without records (Gaussian: the matrix-core kernel where it applies)
    got2, mask2 = run(None)
    assert torch.equal(mask2, fx["accepted"])
    check_states(got2)
    _referee(name, got2[:256], fx["ref"]["x_rows"], L, coupled)
