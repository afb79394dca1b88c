"""The bars of tests/energy_grad_cases.py hold what they claim, on the CPU: the fp32 oracle meets them on the tests' own seeded
inputs at every width and scale, and every mutant (16-bit inputs, uniform weights, padding components with log-weight 0, a
dropped column of the precision matrix) misses them in every case it applies to.  Also the placement edges of rows.h
plan_params the widths are chosen for, and the refusals of ebm_energy_grad_f32 that need no launch.  No constant here is tuned
against a GPU."""

import ctypes

import pytest
import torch

import descent_cases as dc
import energy_grad_cases as eg
from torchebm_amd import _lib

torch.set_num_threads(1)

EBM_EINVAL, EBM_EDIM = -1, -3
KIND_IDS = [eg.kind_id(*k) for k in eg.KINDS]


def measure(kind, K, uniform):
    """({quantity: worst fp32-oracle error}, {mutant: {quantity: lowest error over the cases it applies to}}) in units of U * N"""
    worst = {"energy": 0.0, "grad": 0.0}
    lowest = {}
    for dim, scale in eg.all_cases(kind, K, uniform):
        s = eg.setup(kind, dim, K, uniform, scale)
        assert s.x.dtype == torch.float32 and s.x.shape == (eg.N, dim) and s.route == eg.route(kind, dim)
        ref = eg.reference(s)
        assert all(torch.isfinite(t).all() for t in ref if t is not None), s.id
        e32, g32 = eg.cpu32(s)
        ee, egr = eg.errors(ref, e32, g32)
        worst["energy"] = max(worst["energy"], ee)
        if egr is not None:
            worst["grad"] = max(worst["grad"], egr)
        for name, (mutant, _) in eg.MUTANTS.items():
            out = mutant(s)
            if out is None:
                continue
            me, mg = eg.errors(ref, *out)
            low = lowest.setdefault(name, {"energy": float("inf"), "grad": float("inf"), "cases": 0})
            low["cases"] += 1
            low["energy"] = min(low["energy"], me)
            if mg is not None:
                low["grad"] = min(low["grad"], mg)
    if kind in eg.ELEMENTWISE:
        worst.pop("grad")
    return worst, lowest


@pytest.mark.parametrize("kind,K,uniform", eg.KINDS, ids=KIND_IDS)
def test_fp32_oracle_meets_the_bars_and_every_mutant_misses_them(kind, K, uniform):
    worst, lowest = measure(kind, K, uniform)
    name = eg.kind_id(kind, K, uniform)
    bar, recorded = eg.BAR[name], eg.CPU_WORST[name]
    print(name, "cpu fp32 worst:", {q: round(v, 3) for q, v in worst.items()}, "bars:", bar)
    assert set(worst) == set(bar)
    for q, v in worst.items():
        assert v > 0.0, (name, q, "the fp32 oracle lands on float64: no yardstick")
        assert v <= bar[q], (name, q, v)
        # the constants in the cases module are what this loop measures (another host's torch may add a row in another order)
        assert v <= 1.5 * recorded[q], (name, q, v)
    assert ("inputs16" in lowest) == (kind not in eg.ELEMENTWISE)
    for mutant, low in lowest.items():
        ratios = {q: low[q] / bar[q] for q in eg.MUTANTS[mutant][1]}
        print(name, "mutant", mutant, "cases", low["cases"], "lowest error / bar:", {q: round(r, 1) for q, r in ratios.items()})
        for q, r in ratios.items():
            assert r > 1.0, (name, mutant, q, "passes the bar in some case")


def test_every_mutant_applies_somewhere():
    seen = set()
    for kind, K, uniform in eg.KINDS:
        s = eg.setup(kind, 5, K, uniform)
        seen |= {m for m, (f, _) in eg.MUTANTS.items() if f(s) is not None}
    assert seen == set(eg.MUTANTS)
    assert {K for K in eg.GMM_KS if eg.padded_components(K) != K} == {1, 3, 9, 10, 11}


def test_natural_scales_bound_the_quantities():
    for kind, K, uniform in eg.KINDS:
        s = eg.setup(kind, 33, K, uniform, 5.0)
        e64, g64, ne, ng = eg.reference(s)
        if kind != "gmm":  # (a mixture's scales are those of the expansion |x|^2 - 2 x.mu + |mu|^2, no bound of the result)
            assert (e64.abs() <= ne * (1 + 1e-12)).all(), kind
        if kind == "gauss":
            assert (g64.abs() <= ng * (1 + 1e-12)).all()


def test_widths_cover_every_geometry_route_and_parameter_placement():
    """rows.h pick_geometry and plan_params restated (energy_grad_cases.geometry, plan_floats): 56 KiB of LDS for the shared
    parameters, dim rounded up to 4, components to whole blocks of eight, the log-weights behind the means"""
    every = {(1 << p, 1) for p in range(7)} | {(64, 2), (64, 4)}
    for kind, K, uniform in eg.KINDS:
        ws = eg.widths(kind, K)
        assert set(eg.struct_widths(kind, K)) <= set(ws), (kind, K)
        if K not in (9, 10, 11, 40):
            lane = [d for d in ws if d <= 1024]
            assert {eg.geometry(d) for d in lane if d != 4 * eg.geometry(d)[0] * eg.geometry(d)[1]} == every, (kind, K)
            assert {eg.geometry(d) for d in lane if d == 4 * eg.geometry(d)[0] * eg.geometry(d)[1]} == every, (kind, K)
    budget = eg.LDS_BUDGET_FLOATS
    assert budget == 14336
    g = eg.widths("gauss")
    assert 119 in g and 120 in g and eg.plan_floats("gauss", 119) == 119 * 120 <= budget < 120 * 120 == eg.plan_floats("gauss", 120)
    w16 = eg.widths("gmm", 16)
    assert 892 in w16 and 893 in w16 and eg.plan_floats("gmm", 892, 16) == 16 * 892 + 16 <= budget < 16 * 896 + 16 == eg.plan_floats("gmm", 893, 16)
    # forty components: 40 (dim rounded up to 4) + 40 <= 14336 up to a padded width of 357.4, i.e. 356; 357 rounds up to 360
    assert eg.K40_WIDTHS[-2:] == (356, 357) and eg.widths("gmm", 40) == eg.K40_WIDTHS
    assert eg.plan_floats("gmm", 356, 40) == 40 * 356 + 40 == 14280 <= budget < 40 * 360 + 40 == 14440 == eg.plan_floats("gmm", 357, 40)
    assert (budget - 40) // 40 == 357 and (357 & ~3) == 356
    for K in (1, 3, 8, 9, 10, 11):  # up to sixteen staged components stay in LDS at every structure width but the last
        assert all(eg.plan_floats("gmm", d, K) <= budget for d in eg.widths("gmm", K) if d <= 892), K
    assert eg.plan_floats("gmm", 1024, 8) <= budget < eg.plan_floats("gmm", 1024, 9)
    # routes: the wide-row kernel from 1025 dims (element-wise kinds only), the tiled Gaussian kernel at 132 .. 512 in steps of 4
    assert [eg.route("double_well", d) for d in (1024, 1025, 5000)] == ["rows", "wide", "wide"]
    assert {d for d in g if eg.route("gauss", d) == "tiled"} == {132, 200, 256, 260, 512}
    assert [eg.route("gauss", d) for d in (128, 129, 257, 1000, 1024)] == ["rows"] * 5
    assert eg.N == dc.N == 301 and max(max(eg.widths(k, K)) for k, K, _ in eg.KINDS) == 5000
    # the row counts of the structure tests straddle a block: 256 / G chains, four for the wide-row kernel
    assert eg.n_edges("harmonic", 1025) == (1, 3, 4, 5) and eg.n_edges("gauss", 256) == (1, 3, 4, 5)
    assert eg.n_edges("gmm", 5) == (1, 127, 128, 129) and eg.n_edges("gmm", 100) == (1, 7, 8, 9)


# ----------------------------------------------------------------------------------------------------------------
# refusals of the C entry that launch nothing
# ----------------------------------------------------------------------------------------------------------------
def _desc(kind, n_comp=0, dev0=None, dev1=None):
    d = _lib.EnergyDesc()
    d.kind, d.n_comp = kind, n_comp
    d.s[0], d.s[1] = 1.0, 1.0
    d.dev0, d.dev1 = dev0, dev1
    return d


def _host(floats):
    """(the buffer, a 16-byte aligned address inside it)"""
    buf = (ctypes.c_float * (floats + 8))()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_entry_refuses_before_any_launch():
    """host memory stands in for the device pointers: every call here returns before anything could read them"""
    lib = _lib.lib()
    keep, x = _host(4096)
    keep_g, g = _host(4096)
    keep_p, p = _host(64)
    call = lib.ebm_energy_grad_f32
    for desc in (_desc(_lib.ENERGY_GAUSSIAN, dev0=p, dev1=p), _desc(_lib.ENERGY_GMM, n_comp=8, dev0=p, dev1=p)):
        for dim in (1025, 1028, 5000):
            rc = call(ctypes.byref(desc), x, 2, dim, None, g, None)
            assert rc == EBM_EDIM, (desc.kind, dim, rc, lib.ebm_last_error_string())
    for desc in (_desc(_lib.ENERGY_DOUBLE_WELL), _desc(_lib.ENERGY_HARMONIC), _desc(_lib.ENERGY_GAUSSIAN, dev0=p, dev1=p),
                 _desc(_lib.ENERGY_GMM, n_comp=8, dev0=p, dev1=p)):
        for off in (4, 8, 12):
            rc = call(ctypes.byref(desc), x, 2, 8, None, ctypes.c_void_p(g.value + off), None)
            assert rc == EBM_EINVAL and b"16-byte aligned" in lib.ebm_last_error_string(), (desc.kind, off, rc)
        assert call(ctypes.byref(desc), x, 0, 8, None, g, None) == 0
        assert call(ctypes.byref(desc), x, 0, 8, None, ctypes.c_void_p(g.value + 4), None) == 0  # no chains: nothing is looked at
    del keep, keep_g, keep_p
