"""The fused chain calls' kernel routes and the float64 one-step references that check every route.

ROUTES pins, for each case, the kernel family the host predicates (csrc/api.hip ``langevin_chain_impl``, csrc/hmc.hip
``launch_hmc_chain``) send it to: the first and last width of every predicate and the first width past each edge.  The
inputs, the float64 references and the bars below need no GPU: tests/test_fp64_bars.py checks on the CPU that an fp32
evaluation meets every bar and that a contraction on two-term bf16 splits fails it; tests/test_fp64_one_step_gpu.py holds
the kernels to the same bars, tests/test_route_map_gpu.py checks the routes.

The records=True cases run with a diagnostics record buffer attached (that is what selects the records kernels): record_chains
says which chains the documented geometry puts into which record, record_refs gives every record's float64 references, and
tests/test_records_fp64_gpu.py reads the records the kernels wrote against them (bars: sums_bar, m2_bar, k_record_energy)."""

import math
import re
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

import oracle

U = 2.0 ** -24  # fp32 unit roundoff
K_GMM = 4.0     # the mixture's bar on its expansion scale (tests/test_edge_cases_gpu.py, the mixture matrix-path test)
GMM_FORCE_TARGET = 30.0  # HMC mixtures: the force term's share of the position's natural scale (hmc_eps)


def k_step(dim: int) -> float:
    """per-element bar of one Gaussian step, in units of U times the step's natural scale: 16 up to 128 dims (the bound of
    tests/test_edge_cases_gpu.py); above, an fp32 accumulation of the row itself -- torch's, the lane-group kernel's --
    reaches 17 - 21 on a few hundred chains (tests/test_fp64_bars.py), so 32.  Two-term bf16 operands land at 120 - 200."""
    return 16.0 if dim <= 128 else 32.0
# accept-decision margin: delta = C_H * U * (N(H0) + N(H1)) + C_EXP * 2^-23.  tests/test_fp64_bars.py at 8, 4, 3 and 2: the fp32
# oracle decides every kept chain as float64 does at each of them; two-term bf16 energies decide some chain wrongly in every
# sampled case only from 2 down (at 8 three of the seven cases, at 4 the 160 / 255-dim Gaussians, at 3 the 255-dim one escape;
# at 2 the 200 / 255-dim Gaussians are caught by 2 - 8 of ~570 kept chains, the thinnest margin of the bar tests)
C_H = 2.0
C_EXP = 8.0


@dataclass(frozen=True)
class Case:
    sampler: str   # "langevin" | "heun" | "hmc"
    energy: str    # "gauss" | "gmm" | "ring" (a mixture whose means differ in columns 0..3 only)
    dim: int
    K: int = 0     # mixture components
    mass: str = "none"  # "none" | "scalar" | "diag" (HMC)
    records: bool = False
    image: bool = True  # the Gaussian's pre-split precision image (FusedSpec.aux) handed over
    n: int = 300
    launcher: str = ""  # the chain launcher the route enters (chain_launch.h)
    family: str = ""    # the kernel families launched (family_of), in launch order, space-separated
    family_noise: str = ""  # ... when a noise field is injected, where that differs (Langevin: the non-_fast forms)

    @property
    def id(self):
        s = f"{self.sampler}-{self.energy}-d{self.dim}"
        if self.K:
            s += f"-K{self.K}"
        if self.mass != "none":
            s += f"-{self.mass}"
        if self.records:
            s += "-rec"
        if not self.image:
            s += "-noimg"
        return s + f"-n{self.n}"


def _template_args(s: str):
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += (ch == "<") - (ch == ">")
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()]


def family_of(name: str) -> str:
    """A demangled kernel name cut to what tells the families apart: the base name; for the matrix-core HMC kernels (one
    template, mfma_hmc_body.h) also the energy body, the records flag DIAG and the shift flag SH; for the streamed-Ps Langevin
    kernels (gauss_big_body.h) every flag but the tile count."""
    n = re.sub(r"^void\s+", "", name.strip())
    for ns in ("ebm::", "(anonymous namespace)::", "hmc::", "gbig::"):
        n = n.replace(ns, "")
    head = n[: n.index("(")] if "(" in n else n
    if "<" not in head:
        return head
    base, args = head[: head.index("<")], _template_args(head[head.index("<") + 1: head.rindex(">")])
    if base.startswith("gauss_hmc_mfma_kernel"):
        return f"{base}<{args[2].split('<')[0]},DIAG={args[3]},SH={args[4]}>"
    if base in ("gauss_res_langevin_kernel", "gauss_big_langevin_kernel"):
        return f"{base}<{','.join(args[1:])}>"
    return base


def _R(sampler, energy, dim, **kw):
    return Case(sampler, energy, dim, **kw)


# ----------------------------------------------------------------------------------------------------------------
# The route map: (case, the launcher the route enters, the kernel families it launches).  Families are the gfx950 kernels'
# demangled names cut by family_of.  Element-wise and MLP energies are routed by kind alone (ROUTE_EXEMPT).
# ----------------------------------------------------------------------------------------------------------------
ROUTE_EXEMPT = {
    # launchers whose energies have no width edges to pin (kind alone routes them), each with the tests that cover them
    "launch_langevin_chain_elem": "tests/test_langevin_gpu.py",
    "launch_langevin_chain_elem_diag": "tests/test_diag_gpu.py",
    "launch_langevin_chain_mlp": "tests/test_mlp_gpu.py",
    "launch_mlp_wide": "tests/test_mlp_wide_gpu.py",
    "launch_hmc_chain_audit": "tests/test_hmc_audit_gpu.py",
    "launch_hmc_chain_mlp": "tests/test_mlp_gpu.py",
    "launch_hmc_chain_mlp_wide": "tests/test_mlp_wide_gpu.py",
}

# Kernel families in the built library that no chain route reaches, by family_of name (tests/test_route_map.py lists the
# library's kernels and requires every other one to be pinned by a ROUTES case).
KERNELS_OFF_ROUTE = {
    # not chain kernels: one-step / helper launches of other entry points
    **dict.fromkeys(["cd_loss_kernel", "cd_loss_seed_kernel", "chain_stats_kernel", "chain_stats_wide_kernel", "descent_chain_rows_kernel",
                     "descent_step_kernel", "diag_finish_kernel", "energy_grad_kernel", "energy_grad_wide_row_kernel",
                     "gauss_prec_image_kernel", "gauss_prec_image_res_kernel", "gmm_active_columns_kernel", "hmc_accept_kernel",
                     "kick_drift_kernel", "kick_kernel", "lookahead_kernel", "noise_fill_kernel", "pcd_gather_kernel",
                     "pcd_scatter_kernel", "pcd_start_points_kernel", "probe_issue_kernel", "probe_mix_kernel", "probe_valu_kernel",
                     "langevin_step_diffusion_kernel", "langevin_step_kernel", "langevin_step_wide_kernel",
                     "mlpgrads::mlp_param_grads_kernel", "mlpgrads::mlp_param_grads_reduce_kernel", "widemlp::mlp_w1_image_kernel"],
                    "not a chain kernel"),
    # chain kernels of the launchers in ROUTE_EXEMPT
    **dict.fromkeys(["langevin_chain_elem_kernel", "langevin_chain_lean_kernel", "langevin_chain_lean_contracted_kernel",
                     "langevin_chain_lean_diag_kernel"], "element-wise energies (launch_langevin_chain_elem / _elem_diag)"),
    "hmc_chain_kernel_literal": "launch_hmc_chain_audit",
    "widemlp::mlp_wide_chain_kernel": "launch_mlp_wide", "widemlp::mlp_wide_hmc_kernel": "launch_hmc_chain_mlp_wide",
    # reached only through an A/B switch or a compile-time option, never by a default call
    "gauss_langevin_mfma_kernel": "EBM_GAUSS_F32MFMA=1 (gauss_mfma.hip launch_nt)",
    **dict.fromkeys(["gauss_big_langevin_kernel<1,false,true>", "gauss_big_langevin_kernel<1,true,true>"],
                    "eight tiles on the image: the resident kernel runs them (gauss_big.hip dispatch_big) unless EBM_BIG_TILED_ONLY"),
}

# Predicate edges: (a case at a family's last width or form, the nearest case past it: the next width, or the same width
# without the image / with another mass or records), both in ROUTES; tests/test_route_map.py checks that the two route to
# different families and that every pinned family sits on one side of some edge.
def _key(sampler, energy, dim, **kw):
    return Case(sampler, energy, dim, **kw).id


EDGES = [
    # Gaussian Langevin
    (_key("langevin", "gauss", 3, n=320), _key("langevin", "gauss", 3, n=321)),
    (_key("langevin", "gauss", 16, n=320), _key("langevin", "gauss", 17)),
    (_key("langevin", "gauss", 20), _key("langevin", "gauss", 19, n=320)),
    (_key("langevin", "gauss", 64), _key("langevin", "gauss", 68)),
    (_key("langevin", "gauss", 96), _key("langevin", "gauss", 100)),
    (_key("langevin", "gauss", 62), _key("langevin", "gauss", 63)),
    (_key("langevin", "gauss", 94), _key("langevin", "gauss", 95)),
    (_key("langevin", "gauss", 158), _key("langevin", "gauss", 159)),
    (_key("langevin", "gauss", 160), _key("langevin", "gauss", 164)),
    (_key("langevin", "gauss", 224, image=False), _key("langevin", "gauss", 228, image=False)),
    (_key("langevin", "gauss", 256), _key("langevin", "gauss", 260)),
    (_key("langevin", "gauss", 320), _key("langevin", "gauss", 324)),
    (_key("langevin", "gauss", 256, image=False), _key("langevin", "gauss", 260, image=False)),
    (_key("langevin", "gauss", 260, image=False), _key("langevin", "gauss", 384, image=False, n=200)),
    (_key("langevin", "gauss", 512, n=200), _key("langevin", "gauss", 516, n=200)),
    (_key("langevin", "gauss", 254), _key("langevin", "gauss", 255)),
    (_key("langevin", "gauss", 164), _key("langevin", "gauss", 164, image=False)),
    (_key("langevin", "gauss", 200, records=True, image=False), _key("langevin", "gauss", 256, records=True, image=False)),
    (_key("langevin", "gauss", 201, records=True), _key("langevin", "gauss", 200, records=True)),
    (_key("langevin", "gauss", 64, records=True), _key("langevin", "gauss", 21, records=True)),
    (_key("langevin", "gauss", 200, records=True), _key("langevin", "gauss", 516, records=True, n=200)),
    (_key("langevin", "gauss", 512, records=True, n=200), _key("langevin", "gauss", 516, records=True, n=200)),
    (_key("langevin", "gauss", 260, records=True), _key("langevin", "gauss", 260)),
    (_key("langevin", "gauss", 260, records=True, image=False), _key("langevin", "gauss", 260, image=False)),
    (_key("langevin", "gauss", 256, records=True, image=False), _key("langevin", "gauss", 260, records=True, image=False)),
    (_key("heun", "gauss", 64), _key("langevin", "gauss", 64)),
    # mixture Langevin
    (_key("langevin", "gmm", 20, K=8), _key("langevin", "gmm", 16, K=8)),
    (_key("langevin", "gmm", 12, K=9), _key("langevin", "gmm", 8, K=9)),
    (_key("langevin", "gmm", 32, K=9), _key("langevin", "gmm", 32, K=8)),
    (_key("langevin", "gmm", 17, K=8), _key("langevin", "gmm", 13, K=8)),
    (_key("langevin", "gmm", 126, K=8), _key("langevin", "gmm", 127, K=8)),
    (_key("langevin", "gmm", 256, K=8), _key("langevin", "gmm", 260, K=8)),
    (_key("langevin", "gmm", 128, K=32), _key("langevin", "gmm", 132, K=16)),
    (_key("langevin", "gmm", 64, K=16, records=True), _key("langevin", "gmm", 64, K=33, records=True)),
    (_key("langevin", "gmm", 21, K=8, records=True), _key("langevin", "gmm", 127, K=8, records=True)),
    (_key("langevin", "gmm", 127, K=8, records=True), _key("langevin", "gmm", 255, K=8, records=True)),
    (_key("langevin", "gmm", 2, K=4), _key("langevin", "gmm", 7, K=9)),
    (_key("heun", "gmm", 20, K=8), _key("langevin", "gmm", 20, K=8)),
    # Gaussian HMC
    (_key("hmc", "gauss", 20), _key("hmc", "gauss", 16)),
    (_key("hmc", "gauss", 17), _key("hmc", "gauss", 16)),
    (_key("hmc", "gauss", 158, mass="diag"), _key("hmc", "gauss", 159)),
    (_key("hmc", "gauss", 160), _key("hmc", "gauss", 164)),
    (_key("hmc", "gauss", 256, mass="scalar"), _key("hmc", "gauss", 260)),
    (_key("hmc", "gauss", 254, mass="diag"), _key("hmc", "gauss", 255)),
    (_key("hmc", "gauss", 164), _key("hmc", "gauss", 164, image=False)),
    (_key("hmc", "gauss", 100, records=True), _key("hmc", "gauss", 200, records=True)),
    (_key("hmc", "gauss", 21, records=True), _key("hmc", "gauss", 64, records=True)),
    (_key("hmc", "gauss", 201, mass="scalar", records=True), _key("hmc", "gauss", 200, records=True)),
    (_key("hmc", "gauss", 256, mass="diag", records=True), _key("hmc", "gauss", 260, records=True)),
    # mixture HMC
    (_key("hmc", "gmm", 20, K=8), _key("hmc", "gmm", 16, K=8)),
    (_key("hmc", "gmm", 12, K=9), _key("hmc", "gmm", 8, K=9)),
    (_key("hmc", "gmm", 96, K=16, mass="diag"), _key("hmc", "gmm", 100, K=16, mass="diag")),
    (_key("hmc", "gmm", 128, K=32, mass="scalar"), _key("hmc", "gmm", 132, K=8)),
    (_key("hmc", "gmm", 32, K=9), _key("hmc", "gmm", 32, K=8)),
    (_key("hmc", "gmm", 32, K=8), _key("hmc", "gmm", 32, K=8, mass="scalar")),
    (_key("hmc", "gmm", 17, K=8), _key("hmc", "gmm", 13, K=8)),
    (_key("hmc", "gmm", 126, K=8), _key("hmc", "gmm", 127, K=8)),
    (_key("hmc", "gmm", 94, K=8, mass="diag"), _key("hmc", "gmm", 95, K=8, mass="diag")),
    (_key("hmc", "gmm", 94, K=8, records=True), _key("hmc", "gmm", 95, K=8, records=True)),
    (_key("hmc", "gmm", 64, K=16, records=True), _key("hmc", "gmm", 94, K=8, records=True)),
    (_key("hmc", "gmm", 252, K=32), _key("hmc", "gmm", 256, K=16)),
    (_key("hmc", "gmm", 254, K=32), _key("hmc", "gmm", 255, K=16)),
    (_key("hmc", "gmm", 132, K=8), _key("hmc", "gmm", 132, K=8, mass="diag")),
    (_key("hmc", "gmm", 132, K=8), _key("hmc", "gmm", 132, K=8, records=True)),
    (_key("hmc", "gmm", 129, K=16), _key("hmc", "gmm", 132, K=8)),
    (_key("hmc", "gmm", 64, K=33), _key("hmc", "gmm", 32, K=9)),
]

ROUTES = [
    _R('langevin', 'gauss', 2, launcher="launch_langevin_chain_rows", family="langevin_chain_pair_kernel"),
    _R('langevin', 'gauss', 3, n=320, launcher="launch_langevin_chain_gauss_mfma", family="gauss_langevin_bf16x3_fast_kernel", family_noise="gauss_langevin_bf16x3_kernel"),
    _R('langevin', 'gauss', 3, n=321, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gauss', 5, n=320, launcher="launch_langevin_chain_gauss_mfma", family="gauss_langevin_bf16x3_fast_kernel", family_noise="gauss_langevin_bf16x3_kernel"),
    _R('langevin', 'gauss', 5, n=322, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gauss', 10, n=320, launcher="launch_langevin_chain_gauss_mfma", family="gauss_langevin_bf16x3_fast_kernel", family_noise="gauss_langevin_bf16x3_kernel"),
    _R('langevin', 'gauss', 10, n=321, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gauss', 14, n=320, launcher="launch_langevin_chain_gauss_mfma", family="gauss_langevin_bf16x3_fast_kernel", family_noise="gauss_langevin_bf16x3_kernel"),
    _R('langevin', 'gauss', 14, n=321, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gauss', 16, n=320, launcher="launch_langevin_chain_gauss_mfma", family="gauss_langevin_bf16x3_fast_kernel", family_noise="gauss_langevin_bf16x3_kernel"),
    _R('langevin', 'gauss', 16, n=321, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gauss', 19, n=320, launcher="launch_langevin_chain_gauss_shift", family="gauss_shift_langevin_fast_kernel", family_noise="gauss_shift_langevin_kernel"),
    _R('langevin', 'gauss', 19, n=321, launcher="launch_langevin_chain_gauss_shift", family="gauss_shift_langevin_fast_kernel", family_noise="gauss_shift_langevin_kernel"),
    _R('langevin', 'gauss', 17, launcher="launch_langevin_chain_gauss_shift", family="gauss_shift_langevin_fast_kernel", family_noise="gauss_shift_langevin_kernel"),
    _R('langevin', 'gauss', 18, launcher="launch_langevin_chain_gauss_shift", family="gauss_shift_langevin_fast_kernel", family_noise="gauss_shift_langevin_kernel"),
    _R('langevin', 'gauss', 20, launcher="launch_langevin_chain_gauss_mfma", family="gauss_langevin_bf16x3_fast_kernel", family_noise="gauss_langevin_bf16x3_kernel"),
    _R('langevin', 'gauss', 128, launcher="launch_langevin_chain_gauss_mfma", family="gauss_langevin_bf16x3_fast_kernel", family_noise="gauss_langevin_bf16x3_kernel"),
    _R('langevin', 'gauss', 157, launcher="launch_langevin_chain_gauss_shift", family="gauss_shift_langevin_fast_kernel", family_noise="gauss_shift_langevin_kernel"),
    _R('langevin', 'gauss', 158, launcher="launch_langevin_chain_gauss_shift", family="gauss_shift_langevin_fast_kernel", family_noise="gauss_shift_langevin_kernel"),
    _R('langevin', 'gauss', 132, launcher="launch_langevin_chain_gauss_mfma", family="gauss_langevin_bf16x3_fast_kernel", family_noise="gauss_langevin_bf16x3_kernel"),
    _R('langevin', 'gauss', 160, launcher="launch_langevin_chain_gauss_mfma", family="gauss_langevin_bf16x3_fast_kernel", family_noise="gauss_langevin_bf16x3_kernel"),
    _R('langevin', 'gauss', 164, launcher="launch_langevin_chain_gauss_big", family="gauss_res_langevin_kernel<false,true,true,false>", family_noise="gauss_res_langevin_kernel<false,true,false,false>"),
    _R('langevin', 'gauss', 512, n=200, launcher="launch_langevin_chain_gauss_big", family="gauss_big_langevin_kernel<2,true,true>"),
    _R('langevin', 'gauss', 516, n=200, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gauss', 164, image=False, launcher="launch_langevin_chain_gauss_big", family="gauss_res_langevin_kernel<false,false,false,false>"),
    _R('langevin', 'gauss', 159, launcher="launch_langevin_chain_gauss_res_shift", family="gauss_res_langevin_kernel<false,true,true,true>", family_noise="gauss_res_langevin_kernel<false,true,false,true>"),
    _R('langevin', 'gauss', 254, launcher="launch_langevin_chain_gauss_res_shift", family="gauss_res_langevin_kernel<false,true,true,true>", family_noise="gauss_res_langevin_kernel<false,true,false,true>"),
    _R('langevin', 'gauss', 255, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gauss', 201, image=False, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gmm', 2, K=4, launcher="launch_langevin_chain_rows", family="langevin_chain_pair_kernel"),
    _R('langevin', 'gmm', 20, K=8, launcher="launch_langevin_chain_gmm_mfma", family="gmm_langevin_bf16x3_fast_kernel", family_noise="gmm_langevin_bf16x3_kernel"),
    _R('langevin', 'gmm', 16, K=8, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gmm', 12, K=9, launcher="launch_langevin_chain_gmm_mfma", family="gmm_langevin_bf16x3_fast_kernel", family_noise="gmm_langevin_bf16x3_kernel"),
    _R('langevin', 'gmm', 8, K=9, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gmm', 128, K=32, launcher="launch_langevin_chain_gmm_mfma", family="gmm_langevin_bf16x3_fast_kernel", family_noise="gmm_langevin_bf16x3_kernel"),
    _R('langevin', 'gmm', 32, K=8, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gmm', 32, K=9, launcher="launch_langevin_chain_gmm_mfma", family="gmm_langevin_bf16x3_fast_kernel", family_noise="gmm_langevin_bf16x3_kernel"),
    _R('langevin', 'gmm', 17, K=8, launcher="launch_langevin_chain_gmm_shift", family="gmm_shift_langevin_fast_kernel", family_noise="gmm_shift_langevin_kernel"),
    _R('langevin', 'gmm', 13, K=8, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gmm', 9, K=9, launcher="launch_langevin_chain_gmm_shift", family="gmm_shift_langevin_fast_kernel", family_noise="gmm_shift_langevin_kernel"),
    _R('langevin', 'gmm', 7, K=9, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gmm', 126, K=8, launcher="launch_langevin_chain_gmm_shift", family="gmm_shift_langevin_fast_kernel", family_noise="gmm_shift_langevin_kernel"),
    _R('langevin', 'gmm', 127, K=8, launcher="launch_langevin_chain_gmm_wide_shift", family="gmm_wide_langevin_kernel"),
    _R('langevin', 'gmm', 132, K=16, launcher="launch_langevin_chain_gmm_wide", family="gmm_wide_langevin_kernel"),
    _R('langevin', 'gmm', 256, K=8, launcher="launch_langevin_chain_gmm_wide", family="gmm_wide_langevin_kernel"),
    _R('langevin', 'gmm', 260, K=8, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gmm', 254, K=8, launcher="launch_langevin_chain_gmm_wide_shift", family="gmm_wide_langevin_kernel"),
    _R('langevin', 'gmm', 255, K=8, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gmm', 64, K=33, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gauss', 64, records=True, launcher="launch_langevin_chain_matrix_diag", family="matrix_langevin_diag_kernel"),
    _R('langevin', 'gauss', 10, records=True, n=320, launcher="launch_langevin_chain_matrix_diag", family="matrix_langevin_diag_kernel"),
    _R('langevin', 'gauss', 21, records=True, launcher="launch_langevin_chain_matrix_diag", family="gauss_shift_langevin_diag_kernel"),
    _R('langevin', 'gauss', 200, records=True, launcher="launch_langevin_chain_gauss_big", family="gauss_res_langevin_kernel<true,true,false,false>"),
    _R('langevin', 'gauss', 516, records=True, n=200, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    _R('langevin', 'gmm', 64, K=16, records=True, launcher="launch_langevin_chain_matrix_diag", family="matrix_langevin_diag_kernel"),
    _R('langevin', 'gmm', 21, K=8, records=True, launcher="launch_langevin_chain_matrix_diag", family="gmm_shift_langevin_diag_kernel"),
    _R('langevin', 'gmm', 64, K=33, records=True, launcher="launch_langevin_chain_rows", family="langevin_chain_rows_kernel"),
    # ---- Gaussian Langevin: the 512-thread forms at three tiles (dims 68 .. 96, shifted extents 65 .. 96), the streamed-Ps
    #      dispatch (gauss_big.hip dispatch_big: resident up to seven tiles, eight with the image; NS = 1 at eight tiles without
    #      it; NS = 2 above 256, the records instantiation for the plain call from six out tiles)
    _R('langevin', 'gauss', 64, launcher='launch_langevin_chain_gauss_mfma', family='gauss_langevin_bf16x3_fast_kernel', family_noise='gauss_langevin_bf16x3_kernel'),
    _R('langevin', 'gauss', 68, launcher='launch_langevin_chain_gauss_mfma', family='gauss_langevin_bf16x3_fast_wide_kernel', family_noise='gauss_langevin_bf16x3_kernel'),
    _R('langevin', 'gauss', 96, launcher='launch_langevin_chain_gauss_mfma', family='gauss_langevin_bf16x3_fast_wide_kernel', family_noise='gauss_langevin_bf16x3_kernel'),
    _R('langevin', 'gauss', 100, launcher='launch_langevin_chain_gauss_mfma', family='gauss_langevin_bf16x3_fast_kernel', family_noise='gauss_langevin_bf16x3_kernel'),
    _R('langevin', 'gauss', 62, launcher='launch_langevin_chain_gauss_shift', family='gauss_shift_langevin_fast_kernel', family_noise='gauss_shift_langevin_kernel'),
    _R('langevin', 'gauss', 63, launcher='launch_langevin_chain_gauss_shift', family='gauss_shift_langevin_fast_wide_kernel', family_noise='gauss_shift_langevin_kernel'),
    _R('langevin', 'gauss', 94, launcher='launch_langevin_chain_gauss_shift', family='gauss_shift_langevin_fast_wide_kernel', family_noise='gauss_shift_langevin_kernel'),
    _R('langevin', 'gauss', 95, launcher='launch_langevin_chain_gauss_shift', family='gauss_shift_langevin_fast_kernel', family_noise='gauss_shift_langevin_kernel'),
    _R('langevin', 'gauss', 224, image=False, launcher='launch_langevin_chain_gauss_big', family='gauss_res_langevin_kernel<false,false,false,false>'),
    _R('langevin', 'gauss', 228, image=False, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<1,false,false>'),
    _R('langevin', 'gauss', 256, image=False, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<1,false,false>'),
    _R('langevin', 'gauss', 256, launcher='launch_langevin_chain_gauss_big', family='gauss_res_langevin_kernel<false,true,true,false>', family_noise='gauss_res_langevin_kernel<false,true,false,false>'),
    _R('langevin', 'gauss', 260, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<2,false,true>'),
    _R('langevin', 'gauss', 320, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<2,false,true>'),
    _R('langevin', 'gauss', 324, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<2,true,true>'),
    _R('langevin', 'gauss', 260, image=False, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<2,false,false>'),
    _R('langevin', 'gauss', 384, image=False, n=200, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<2,true,false>'),
    # ---- records: the streamed-Ps forms without the image and on shifted rows, the wide mixtures
    _R('langevin', 'gauss', 256, records=True, image=False, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<1,true,false>'),
    _R('langevin', 'gauss', 200, records=True, image=False, launcher='launch_langevin_chain_gauss_big', family='gauss_res_langevin_kernel<true,false,false,false>'),
    # (two slices, above 256 dims: the records instantiation, which the plain call shares only from six out tiles)
    _R('langevin', 'gauss', 260, records=True, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<2,true,true>'),
    _R('langevin', 'gauss', 512, records=True, n=200, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<2,true,true>'),
    _R('langevin', 'gauss', 260, records=True, image=False, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<2,true,false>'),
    _R('langevin', 'gauss', 384, records=True, image=False, n=200, launcher='launch_langevin_chain_gauss_big', family='gauss_big_langevin_kernel<2,true,false>'),
    _R('langevin', 'gauss', 201, records=True, launcher='launch_langevin_chain_matrix_diag', family='gauss_res_langevin_kernel<true,true,false,true>'),
    _R('langevin', 'gauss', 254, records=True, launcher='launch_langevin_chain_matrix_diag', family='gauss_res_langevin_kernel<true,true,false,true>'),
    _R('langevin', 'gmm', 132, K=12, records=True, launcher='launch_langevin_chain_matrix_diag', family='gmm_wide_langevin_diag_kernel'),
    _R('langevin', 'gmm', 200, K=12, records=True, launcher='launch_langevin_chain_matrix_diag', family='gmm_wide_langevin_diag_kernel'),
    _R('langevin', 'gmm', 127, K=8, records=True, launcher='launch_langevin_chain_matrix_diag', family='gmm_wide_langevin_diag_kernel'),
    _R('langevin', 'gmm', 255, K=8, records=True, launcher='launch_langevin_chain_rows', family='langevin_chain_rows_kernel'),
    _R('heun', 'gauss', 64, launcher="launch_langevin_chain_rows", family="langevin_heun_rows_kernel"),
    _R('heun', 'gauss', 64, records=True, launcher="launch_langevin_chain_rows", family="langevin_heun_rows_kernel"),
    _R('heun', 'gmm', 20, K=8, launcher="launch_langevin_chain_rows", family="langevin_heun_rows_kernel"),
    _R('hmc', 'gauss', 20, launcher="launch_hmc_chain_gauss_mfma", family="gauss_hmc_mfma_kernel_w2<GaussE,DIAG=false,SH=false>"),
    _R('hmc', 'gauss', 20, mass='scalar', launcher="launch_hmc_chain_gauss_mfma", family="gauss_hmc_mfma_kernel_w2<GaussE,DIAG=false,SH=false>"),
    _R('hmc', 'gauss', 20, mass='diag', launcher="launch_hmc_chain_gauss_mfma", family="gauss_hmc_mfma_kernel_w2<GaussE,DIAG=false,SH=false>"),
    _R('hmc', 'gauss', 160, launcher="launch_hmc_chain_gauss_mfma", family="gauss_hmc_mfma_kernel<GaussE,DIAG=false,SH=false>"),
    _R('hmc', 'gauss', 160, mass='scalar', launcher="launch_hmc_chain_gauss_mfma", family="gauss_hmc_mfma_kernel<GaussE,DIAG=false,SH=false>"),
    _R('hmc', 'gauss', 160, mass='diag', launcher="launch_hmc_chain_gauss_mfma", family="gauss_hmc_mfma_kernel<GaussE,DIAG=false,SH=false>"),
    _R('hmc', 'gauss', 16, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gauss', 164, image=False, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gauss', 17, launcher="launch_hmc_chain_gauss_shift", family="gauss_hmc_mfma_kernel<GaussE,DIAG=false,SH=true>"),
    _R('hmc', 'gauss', 158, mass='diag', launcher="launch_hmc_chain_gauss_shift", family="gauss_hmc_mfma_kernel<GaussE,DIAG=false,SH=true>"),
    _R('hmc', 'gauss', 164, launcher="launch_hmc_chain_gauss_stream", family="gauss_hmc_mfma_kernel<GaussStreamE,DIAG=false,SH=false>"),
    _R('hmc', 'gauss', 256, mass='scalar', launcher="launch_hmc_chain_gauss_stream", family="gauss_hmc_mfma_kernel<GaussStreamE,DIAG=false,SH=false>"),
    _R('hmc', 'gauss', 260, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gauss', 159, launcher="launch_hmc_chain_gauss_stream_shift", family="gauss_hmc_mfma_kernel<GaussStreamE,DIAG=false,SH=true>"),
    _R('hmc', 'gauss', 254, mass='diag', launcher="launch_hmc_chain_gauss_stream_shift", family="gauss_hmc_mfma_kernel<GaussStreamE,DIAG=false,SH=true>"),
    _R('hmc', 'gauss', 255, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gauss', 192, image=False, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gauss', 64, records=True, launcher="launch_hmc_chain_matrix_diag", family="gauss_hmc_mfma_kernel<GaussE,DIAG=true,SH=false>"),
    _R('hmc', 'gauss', 96, records=True, launcher="launch_hmc_chain_matrix_diag", family="gauss_hmc_mfma_kernel<GaussE,DIAG=true,SH=false>"),
    _R('hmc', 'gauss', 100, records=True, launcher="launch_hmc_chain_matrix_diag", family="gauss_hmc_mfma_kernel<GaussE,DIAG=true,SH=false>"),
    _R('hmc', 'gauss', 21, records=True, launcher="launch_hmc_chain_gauss_shift_diag", family="gauss_hmc_mfma_kernel<GaussE,DIAG=true,SH=true>"),
    _R('hmc', 'gauss', 201, mass='scalar', records=True, launcher="launch_hmc_chain_gauss_stream_shift_diag", family="gauss_hmc_mfma_kernel<GaussStreamE,DIAG=true,SH=true>"),
    # ---- records of the streamed Ps at aligned widths (matrix_hmc_diag.hip), and past them
    _R('hmc', 'gauss', 200, records=True, launcher='launch_hmc_chain_matrix_diag', family='gauss_hmc_mfma_kernel<GaussStreamE,DIAG=true,SH=false>'),
    _R('hmc', 'gauss', 256, mass='diag', records=True, launcher='launch_hmc_chain_matrix_diag', family='gauss_hmc_mfma_kernel<GaussStreamE,DIAG=true,SH=false>'),
    _R('hmc', 'gauss', 260, records=True, launcher='launch_hmc_chain', family='hmc_chain_kernel'),
    _R('hmc', 'gauss', 200, records=True, image=False, launcher='launch_hmc_chain', family='hmc_chain_kernel'),
    _R('hmc', 'gmm', 20, K=8, launcher="launch_hmc_chain_gmm_mfma", family="gauss_hmc_mfma_kernel_w3<GmmE,DIAG=false,SH=false>"),
    _R('hmc', 'gmm', 16, K=8, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gmm', 12, K=9, launcher="launch_hmc_chain_gmm_mfma", family="gauss_hmc_mfma_kernel_w3<GmmE,DIAG=false,SH=false>"),
    _R('hmc', 'gmm', 8, K=9, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gmm', 128, K=32, mass='scalar', launcher="launch_hmc_chain_gmm_mfma", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=false>"),
    _R('hmc', 'gmm', 96, K=16, mass='diag', launcher="launch_hmc_chain_gmm_mfma", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=false>"),
    _R('hmc', 'gmm', 100, K=16, mass='diag', launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    # (dim 32, K <= 8, identity mass: both kernels are launched and each reads the active-column mask on the device --
    #  hmc_slot1 does the work for the ring, hmc_gmm32 for the dense mixture, the other returns at once.  The profiler sees the
    #  same launches for the two, so these rows pin the pair, not which of them computed; the one-step checks see the result.)
    _R('hmc', 'ring', 32, K=4, launcher="launch_hmc_chain", family="hmc_slot1_kernel hmc_slot1_kernel hmc_gmm32_kernel"),
    _R('hmc', 'gmm', 32, K=8, launcher="launch_hmc_chain", family="hmc_slot1_kernel hmc_slot1_kernel hmc_gmm32_kernel"),
    _R('hmc', 'gmm', 32, K=8, mass='scalar', launcher="launch_hmc_chain", family="hmc_chain_kernel_w2"),
    _R('hmc', 'gmm', 32, K=9, launcher="launch_hmc_chain_gmm_mfma", family="gauss_hmc_mfma_kernel_w3<GmmE,DIAG=false,SH=false>"),
    _R('hmc', 'gmm', 17, K=8, launcher="launch_hmc_chain_gmm_shift", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=true>"),
    _R('hmc', 'gmm', 13, K=8, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gmm', 9, K=9, launcher="launch_hmc_chain_gmm_shift", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=true>"),
    _R('hmc', 'gmm', 126, K=8, launcher="launch_hmc_chain_gmm_shift", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=true>"),
    _R('hmc', 'gmm', 94, K=8, mass='diag', launcher="launch_hmc_chain_gmm_shift", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=true>"),
    _R('hmc', 'gmm', 95, K=8, mass='diag', launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gmm', 94, K=8, records=True, launcher="launch_hmc_chain_gmm_shift_diag", family="gauss_hmc_mfma_kernel<GmmE,DIAG=true,SH=true>"),
    _R('hmc', 'gmm', 95, K=8, records=True, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gmm', 64, K=16, records=True, launcher="launch_hmc_chain_matrix_diag", family="gauss_hmc_mfma_kernel<GmmE,DIAG=true,SH=false>"),
    # (records of a wide mixture: the matrix-layout records stop at 96 dims, the lane-group kernel writes them)
    _R('hmc', 'gmm', 132, K=8, records=True, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gmm', 132, K=8, launcher="launch_hmc_chain_gmm_wide", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=false>"),
    _R('hmc', 'gmm', 224, K=16, launcher="launch_hmc_chain_gmm_wide", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=false>"),
    _R('hmc', 'gmm', 228, K=16, launcher="launch_hmc_chain_gmm_wide", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=false>"),
    _R('hmc', 'gmm', 252, K=32, launcher="launch_hmc_chain_gmm_wide", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=false>"),
    _R('hmc', 'gmm', 256, K=16, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gmm', 127, K=8, launcher="launch_hmc_chain_gmm_wide_shift", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=true>"),
    _R('hmc', 'gmm', 129, K=16, launcher="launch_hmc_chain_gmm_wide_shift", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=true>"),
    _R('hmc', 'gmm', 222, K=8, launcher="launch_hmc_chain_gmm_wide_shift", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=true>"),
    _R('hmc', 'gmm', 229, K=16, launcher="launch_hmc_chain_gmm_wide_shift", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=true>"),
    _R('hmc', 'gmm', 254, K=32, launcher="launch_hmc_chain_gmm_wide_shift", family="gauss_hmc_mfma_kernel<GmmE,DIAG=false,SH=true>"),
    _R('hmc', 'gmm', 255, K=16, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gmm', 132, K=8, mass='diag', launcher="launch_hmc_chain", family="hmc_chain_kernel"),
    _R('hmc', 'gmm', 64, K=33, launcher="launch_hmc_chain", family="hmc_chain_kernel"),
]


# ----------------------------------------------------------------------------------------------------------------
# Inputs (seeded, CPU, fp32)
# ----------------------------------------------------------------------------------------------------------------
def _gen(case: Case, salt: int) -> torch.Generator:
    h = (case.dim * 1009 + case.K * 131 + {"langevin": 1, "heun": 2, "hmc": 3}[case.sampler] * 7 + salt) & 0x7FFFFFFF
    return torch.Generator().manual_seed(h)


def gauss_params(case: Case, decades: float):
    """mean and covariance of a dense Gaussian whose coordinates span `decades` decades of scale (fp32)."""
    g = _gen(case, 11)
    dim = case.dim
    a = torch.randn(dim, dim, generator=g, dtype=torch.float64)
    scale = 10.0 ** (torch.rand(dim, generator=g, dtype=torch.float64) * decades - decades / 2)
    cov = (a @ a.t() / dim + 0.5 * torch.eye(dim, dtype=torch.float64)) * scale[:, None] * scale[None, :]
    mean = torch.randn(dim, generator=g, dtype=torch.float64)
    return mean.float(), cov.float()


def gmm_params(case: Case):
    """means [K, dim], sigma, weights of a mixture; "ring": the means differ in columns 0..3 only."""
    g = _gen(case, 13)
    K, dim = case.K, case.dim
    means = torch.randn(K, dim, generator=g) * 1.5
    if case.energy == "ring":
        means[:, 4:] = means[0:1, 4:]
    weights = torch.rand(K, generator=g) + 0.2
    return means, 0.8, weights


def sym_precision(cov_inv: torch.Tensor) -> torch.Tensor:
    """what GaussianModel.fused_spec hands the kernels: the symmetrised fp32 precision matrix."""
    return (0.5 * (cov_inv + cov_inv.t())).contiguous()


def gmm_log_weights(weights: torch.Tensor) -> torch.Tensor:
    """GaussianMixtureModel's fp32 log-weights."""
    w = weights.to(torch.float64)
    return torch.log(w / w.sum()).float()


def langevin_x0(case: Case, params):
    g = _gen(case, 17)
    n, dim = case.n, case.dim
    if case.energy == "gauss":
        return (torch.randn(n, dim, generator=g, dtype=torch.float64) *
                10.0 ** (torch.rand(n, dim, generator=g, dtype=torch.float64) * 6 - 3)).float()
    return gmm_x0(case, params, g)


def gmm_x0(case: Case, params, g):
    """states from deep inside a component (0.03 sigma) to its shell (2 sigma), a quarter of them on the ridge between two."""
    means, sigma, _ = params
    n, dim, K = case.n, case.dim, case.K
    pick = torch.randint(0, K, (n,), generator=g)
    spread = 10.0 ** (torch.rand(n, 1, generator=g) * 1.8 - 1.5)
    x0 = (means[pick] + torch.randn(n, dim, generator=g) * sigma * spread).float()
    q = n // 4
    x0[:q] = (0.5 * (means[pick[:q]] + means[(pick[:q] + 1) % K]) + 0.05 * torch.randn(q, dim, generator=g)).float()
    return x0


# ----------------------------------------------------------------------------------------------------------------
# float64 references of one evaluation, and their natural scales
# ----------------------------------------------------------------------------------------------------------------
def gauss_grad64(x, mean, ps):
    """float64 gradient P d of the fp32 parameters, and its natural scale sum_j |P_ij| |d_j|."""
    d = x.double() - mean.double()
    p = ps.double()
    return d @ p.t(), d.abs() @ p.abs().t()


def gmm_grad64(x, means, sigma, logw):
    en64 = oracle.GaussianMixture(means.double(), sigma, log_weights=logw)
    en64.means, en64.log_weights = means.double(), logw.double()
    return en64.grad(x.double())


def gmm_natural(x, means, sigma):
    """the expansion scale of the mixture's gradient, per row: the kernel forms |x|^2 - 2 x.mu + |mu|^2 (csrc/gmm_bf16x3.h),
    whose rounding is relative to |x|^2 + |mu|^2 (tests/test_edge_cases_gpu.py, the mixture matrix-path test)."""
    d = x.double()[:, None, :] - means.double()[None]
    logit_scale = (x.double().square().sum(dim=1) + means.double().square().sum(dim=1).max()) / (2.0 * sigma ** 2)
    return d.abs().amax(dim=(1, 2)) / sigma ** 2 * (1.0 + logit_scale)


def gmm_energy64(x, means, sigma, logw):
    sq = (x.double()[:, None, :] - means.double()[None]).square().sum(dim=-1)
    return -torch.logsumexp(logw.double() - sq / (2.0 * sigma ** 2), dim=1)


def gmm_energy_scale(x, means, sigma):
    return (x.double().square().sum(dim=1) + means.double().square().sum(dim=1).max()) / (2.0 * sigma ** 2)


def langevin_ref(case: Case, x0, fp, eta):
    """(want, natural) of one noise-free step in float64; `fp` the fp32 parameters the kernel was handed.
    Gaussian: natural per element; mixture: per row (the expansion scale)."""
    if case.energy == "gauss":
        mean, ps = fp
        g, gn = gauss_grad64(x0, mean, ps)
        if case.sampler == "heun":
            xt = x0.double() - eta * g
            g1, gn1 = gauss_grad64(xt, mean, ps)
            want = x0.double() - 0.5 * eta * (g + g1)
            nat_t = x0.double().abs() + eta * gn
            # the stage input's own rounding reaches the second evaluation through |P|
            natural = x0.double().abs() + 0.5 * eta * (gn + gn1) + 0.5 * eta * (nat_t @ ps.double().abs().t())
            return want, natural
        return x0.double() - eta * g, x0.double().abs() + eta * gn
    means, sigma, logw = fp
    g = gmm_grad64(x0, means, sigma, logw)
    nat = x0.double().abs().amax(dim=1) + eta * gmm_natural(x0, means, sigma)
    if case.sampler == "heun":
        xt = x0.double() - eta * g
        g1 = gmm_grad64(xt, means, sigma, logw)
        nat = nat + eta * gmm_natural(xt, means, sigma)
        return x0.double() - 0.5 * eta * (g + g1), nat
    return x0.double() - eta * g, nat


def langevin_ref32(case: Case, x0, fp, eta):
    """the fp32 oracle's own step (torch autograd in fp32) -- the yardstick of the mixtures."""
    en = _oracle32(case, fp)
    if case.sampler == "heun":
        return oracle.langevin.heun_step(en, x0, None, eta, None)
    return x0 - eta * en.grad(x0)


def _oracle32(case: Case, fp):
    if case.energy == "gauss":
        mean, ps = fp
        en = oracle.Gaussian(mean, torch.eye(mean.shape[0]))
        en.cov_inv = ps.float()
        return en
    means, sigma, logw = fp
    return oracle.GaussianMixture(means, sigma, log_weights=logw)


# ---- HMC ------------------------------------------------------------------------------------------------------
def hmc_mass(case: Case):
    """None | float | fp32 [dim] tensor, as the oracle and ebm_hmc_chain_f32 take it."""
    if case.mass == "none":
        return None
    if case.mass == "scalar":
        return 2.5
    g = _gen(case, 19)
    return (10.0 ** (torch.rand(case.dim, generator=g) * 2 - 1)).float()


def _mass64(mass, dim):
    if mass is None:
        return torch.ones(dim, dtype=torch.float64)
    if isinstance(mass, float):
        return torch.full((dim,), mass, dtype=torch.float64)
    return mass.double()


def hmc_inputs(case: Case, params):
    """x0, standard normals p (the kernel scales them by sqrt(m)) and the mass."""
    g = _gen(case, 23)
    n, dim = case.n, case.dim
    if case.energy == "gauss":
        mean = params[0]
        x0 = (mean.double() + torch.randn(n, dim, generator=g, dtype=torch.float64) *
              10.0 ** (torch.rand(n, dim, generator=g, dtype=torch.float64) * 3 - 2)).float()
    else:
        x0 = gmm_x0(case, params, g)
    p = torch.randn(n, dim, generator=g)
    return x0, p, hmc_mass(case)


def _force_terms(case, x0, fp):
    """(force64, force natural per element or row)"""
    if case.energy == "gauss":
        mean, ps = fp
        return gauss_grad64(x0, mean, ps)
    means, sigma, logw = fp
    return gmm_grad64(x0, means, sigma, logw), gmm_natural(x0, means, sigma)


def hmc_eps(case: Case, x0, p, mass, fp, target: float = 1.0) -> float:
    """the fp32 step size at which the force term 1/2 eps^2 / m sum |P||d| is `target` times the rest of the natural
    scale |x0| + eps |p sqrt m| / m in the median -- the force's error must not hide under the rounding of x0."""
    m = _mass64(mass, case.dim)
    _, fn = _force_terms(case, x0, fp)
    ps = p.double() * m.sqrt()
    if case.energy == "gauss":
        a, b, c = 0.5 * fn / m, x0.double().abs(), ps.abs() / m
    else:
        a, b, c = 0.5 * fn / m.min(), x0.double().abs().amax(dim=1), (ps.abs() / m).amax(dim=1)
    lo, hi = -8.0, 4.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        e = 10.0 ** mid
        if (a * e * e / (b + c * e)).median().item() < target:
            lo = mid
        else:
            hi = mid
    return float(torch.tensor(10.0 ** lo, dtype=torch.float32).item())


def hmc_ref(case: Case, x0, p, mass, fp, eps: float):
    """(x1, natural) of one leapfrog step in float64 with the oracle's fp32 eps and its force clamp at +-1e6."""
    m = _mass64(mass, case.dim)
    g, fn = _force_terms(case, x0, fp)
    f = (-g).clamp(-1e6, 1e6)
    ps = p.double() * m.sqrt()
    x1 = x0.double() + eps * (ps + 0.5 * eps * f) / m
    if case.energy == "gauss":
        natural = x0.double().abs() + eps * ps.abs() / m + 0.5 * eps * eps / m * fn
    else:
        natural = x0.double().abs().amax(dim=1) + (eps * ps.abs() / m).amax(dim=1) + 0.5 * eps * eps / m.min() * fn
    return x1, natural, g.abs().max().item()


def hmc_ref32(case: Case, x0, p, mass, fp, eps: float):
    """the fp32 oracle's leapfrog position after one step (the yardstick of the mixtures)."""
    en = _oracle32(case, fp)
    pm = p.clone()
    if mass is not None:
        pm = pm * (math.sqrt(mass) if isinstance(mass, float) else mass.sqrt())
    x1, _ = oracle.hmc.leapfrog(en, x0, pm, eps, 1, mass, safe=True)
    return x1


def energy64(case: Case, x, fp):
    """float64 energy of the fp32 parameters and its natural scale N(E), per chain: 1/2 |d|^T |P| |d| for a Gaussian, the
    expansion scale for a mixture."""
    x = x.double()
    if case.energy == "gauss":
        mean, P = fp
        d = x - mean.double()
        return 0.5 * ((d @ P.double().t()) * d).sum(dim=1), 0.5 * ((d.abs() @ P.double().abs().t()) * d.abs()).sum(dim=1)
    means, sigma, logw = fp
    return gmm_energy64(x, means, sigma, logw), gmm_energy_scale(x, means, sigma)


def hmc_hamiltonians64(case: Case, x0, p, mass, fp, eps: float):
    """float64 H0, H1 of one full leapfrog step (L = 1) and their natural scales N(H0), N(H1)."""
    m = _mass64(mass, case.dim)
    ps = p.double() * m.sqrt()

    def energy(x):
        return energy64(case, x, fp)

    def grad(x):
        if case.energy == "gauss":
            return gauss_grad64(x, fp[0], fp[1])[0]
        return gmm_grad64(x, fp[0], fp[1], fp[2])

    x = x0.double()
    f0 = (-grad(x)).clamp(-1e6, 1e6)
    ph = ps + 0.5 * eps * f0
    x1 = x + eps * ph / m
    f1 = (-grad(x1)).clamp(-1e6, 1e6)
    p1 = ph + 0.5 * eps * f1
    e0, n0 = energy(x)
    e1, n1 = energy(x1)
    k0, k1 = 0.5 * (ps.square() / m).sum(dim=1), 0.5 * (p1.square() / m).sum(dim=1)
    return e0 + k0, e1 + k1, n0 + k0, n1 + k1


def hmc_hamiltonians32(case: Case, x0, p, mass, fp, eps: float):
    """the fp32 oracle's H0, H1 of the same step."""
    en = _oracle32(case, fp)
    pm = p.clone()
    if mass is not None:
        pm = pm * (math.sqrt(mass) if isinstance(mass, float) else mass.sqrt())
    h0 = en.energy(x0) + oracle.hmc.kinetic(pm, mass)
    x1, p1 = oracle.hmc.leapfrog(en, x0, pm, eps, 1, mass, safe=True)
    h1 = en.energy(x1) + oracle.hmc.kinetic(p1, mass)
    return h0, h1


def accept_draws(h0, h1, n0, n1):
    """(keep, u, below): the chains with a64 = exp(H0 - H1) < 1 (and not vanishing), and the injected uniforms
    u = a64 (1 -+ delta) -- below the acceptance probability on even chains, above it on odd ones."""
    dh = (h0 - h1)
    a64 = torch.exp(dh.clamp(-50, 50))
    delta = C_H * U * (n0 + n1) + C_EXP * 2.0 ** -23
    keep = (a64 < 1.0) & (a64 > 1e-12) & (delta < 0.5)
    below = (torch.arange(h0.shape[0]) % 2) == 0
    u = torch.where(below, a64 * (1 - delta), a64 * (1 + delta))
    u = torch.where(keep, u, torch.full_like(u, 0.5))
    return keep, u.float(), below


def hmc_accept_x0(case: Case, x0, fp):
    """states for the accept decisions: a Gaussian's typical draws (mean + chol(cov) z) -- the wide-range states of the
    position check have energies of 1e6, whose fp32 rounding alone would decide the call; mixtures keep theirs."""
    if case.energy != "gauss":
        return x0
    mean, ps = fp
    g = _gen(case, 29)
    chol = torch.linalg.cholesky(torch.linalg.inv(ps.double()))
    z = torch.randn(case.n, case.dim, generator=g, dtype=torch.float64)
    return (mean.double() + z @ chol.t()).float()


def hmc_accept_eps(case: Case, x0, p, mass, fp) -> float:
    """a step size at which most chains have a64 in (1e-3, 1): half the stable step of the stiffest direction the
    rows see, scaled down until the median energy change is O(1)."""
    eps = hmc_eps(case, x0, p, mass, fp, target=1.0)
    for _ in range(40):
        h0, h1, _, _ = hmc_hamiltonians64(case, x0, p, mass, fp, eps)
        if (h1 - h0).abs().median().item() < 2.0:
            break
        eps = float(torch.tensor(eps * 0.5, dtype=torch.float32).item())
    return eps


# ----------------------------------------------------------------------------------------------------------------
# Diagnostics records: which chains a record holds, its float64 references and their bars
# ----------------------------------------------------------------------------------------------------------------
# The record-to-chain map below restates the documented geometry (include/ebm_hip.h under ebm_diag_layout, the header of
# csrc/diag.h), not any kernel: a layout is (n_blocks, S, E) as ebm_diag_layout returns it.
def diag_classes(dim: int) -> int:
    """K = 4 / gcd(dim, 4) alignment classes of the shifted rows."""
    return 4 // math.gcd(dim, 4)


def record_count(S: int, E: int, n: int, dim: int) -> int:
    """records per kept step: ceil(n dim / E) blocks of E flat elements; ceil(n / 32 K) K for interleaved classes (E < 0)."""
    if E < 0:
        K = diag_classes(dim)
        return -(-n // (32 * K)) * K
    return -(-(n * dim) // E)


def record_chains(layout, n: int, dim: int):
    """For every record b, the flat indices (into the row-major [n, dim] state) of the elements it holds, as a [rows, S]
    tensor: column s of it is what slot s sums.  rows = 0: a record without chains.
      E < 0            interleaved classes: record b = (group b / K, class b % K) holds chains 32 K g + K m + s, m = 0 .. 31
      S > dim          packed rows: the state read as n dim / S rows of width S, E / S of them per record
      E % dim == 0     E / dim whole chains per record
      dim % E == 0     one slice of E elements of one chain per record (slot s is column (b E) % dim + s)"""
    nb, S, E = layout
    cols = torch.arange(S)
    if E < 0:
        assert E == -32 * dim and S == dim, layout
        K = diag_classes(dim)
        out = []
        for b in range(nb):
            g, s = divmod(b, K)
            chains = 32 * K * g + K * torch.arange(32) + s
            out.append(chains[chains < n][:, None] * dim + cols[None])
        return out
    W = max(S, dim)  # the width of the rows the records speak of
    total = n * dim
    assert total % W == 0 and W % dim == 0, layout
    if E % W == 0:
        assert S == W, layout
        per, rows_total = E // W, total // W
        return [torch.arange(min(b * per, rows_total), min((b + 1) * per, rows_total))[:, None] * W + cols[None] for b in range(nb)]
    assert W == dim and dim % E == 0 and S == E, layout
    return [(b * E + cols)[None] if b * E < total else torch.empty(0, S, dtype=torch.long) for b in range(nb)]


def record_groups(layout, n: int, dim: int):
    """[(records, chains)]: the smallest runs of consecutive records that cover whole chains -- one record each, except
    where a chain is spread over dim / E records: only the sum of their energy and accept shares is defined."""
    nb, S, E = layout
    idx = record_chains(layout, n, dim)
    if 0 < E < dim:
        per = dim // E
        return [(list(range(b, b + per)), torch.unique(torch.cat([idx[r].flatten() for r in range(b, b + per)]) // dim))
                for b in range(0, nb, per)]
    return [([b], torch.unique(idx[b].flatten() // dim)) for b in range(nb)]


def wave_layout(n: int, dim: int):
    """the layout of a matrix-layout kernel's records, where a wave of 32 rows is the block: interleaved classes for widths
    off multiples of 4 (shifted rows), S / dim = 2, 4, .. chains packed into one row for Gaussians narrower than 20 (the
    first packing that is a multiple of 4 from 20 up and divides n: csrc/gauss_mfma.hip gauss_pack_factor)."""
    if dim >= 20 and dim % 4:
        return record_count(dim, -32 * dim, n, dim), dim, -32 * dim
    S = dim
    while S < 20 or S % 4:
        S *= 2
    assert S == dim or (n % (S // dim) == 0 and S <= 128), (n, dim)
    return record_count(S, 32 * S, n, dim), S, 32 * S


def rows_layout(n: int, dim: int, chains: int):
    """the layout of a lane-group kernel that keeps `chains` chains per workgroup"""
    return record_count(dim, chains * dim, n, dim), dim, chains * dim


# lane-group kernels: their records come from diag::emit, which adds a slot's rows one after the other; every other records
# family keeps 32 chains in a wave's matrix layout and adds them as a tree of five levels (diag.h half_wave_sum)
EMIT_FAMILIES = ("langevin_chain_rows_kernel", "langevin_heun_rows_kernel", "langevin_chain_pair_kernel", "hmc_chain_kernel",
                 "hmc_chain_kernel_w2")


def record_depth(case: Case, layout) -> int:
    """the longest chain of fp32 additions an element passes through on its way into a record's sum"""
    nb, S, E = layout
    if case.family in EMIT_FAMILIES:
        return max(1, E // max(S, case.dim))  # rows per block
    assert abs(E) == 32 * S, (case.id, layout)
    return 5


def gamma(d: int) -> float:
    """the bound of d chained fp32 roundings"""
    return d * U / (1.0 - d * U)


def sums_bar(depth: int, abs_sum):
    """|fl(sum x) - sum x| <= gamma(depth) sum |x|, whatever the order inside that depth"""
    return gamma(depth) * abs_sum


def m2_bar(depth: int, cnt, abs_sum, m2):
    """Two passes: the centre c = fl(fl(sum) / cnt) (or fl(sum) * fl(1 / cnt): two roundings) is off the mean by at most
    dmu = (gamma(depth) + 2 U) sum|x| / cnt, and sum (x - c)^2 = M2 + cnt (c - mean)^2 exactly; every term then takes one
    rounding of x - c (twice in the square), one of the fused multiply-add and `depth` additions."""
    cnt = cnt.clamp(min=1)
    shift = cnt * ((gamma(depth) + 2 * U) * abs_sum / cnt).square()
    return gamma(depth + 3) * (m2 + shift) + shift


# The energy share of a record of a wave's 32 chains, in units of U times sum N(E) over its chains.  tests/test_fp64_bars.py
# (test_record_energy_bars), worst record of each sampled case, n = 300 .. 1000:
#   Gaussians (10 .. 512 dims, Langevin and HMC with each mass form): the fp32 oracle summed in fp32 0.9 .. 11.4 U (512 dims);
#   energies from two-term bf16 operands 33 .. 106 U (the lowest: HMC at 200 dims, Langevin at 512 with 39)
#   mixtures (21 .. 200 dims): the fp32 oracle 0.1 .. 0.5 U, the kernels' expansion |x|^2 - 2 x.mu + |mu|^2 in fp32 0.2 .. 1.4 U
#   (HMC at 94 dims); two-term operands 2.9 .. 11.4 U (the lowest: Langevin at 200 dims)
K_REC_GAUSS = 16.0
K_REC_GMM = 2.0


def k_record_energy(case: Case, layout) -> float:
    """Wave records (32 chains): the measured constants above.  Records of the lane-group kernels hold E / dim chains, down
    to one, where nothing averages: there a chain's own bar holds.  Its gradient g = P d is good to k_step(dim) U per element
    of |P||d|, so the products d_i g_i are good to (k_step(dim) + 1) U |d_i| (|P||d|)_i; adding the dim of them as a tree (a
    lane group's reduction, torch's sum) costs log2(dim) roundings more, adding the record's chains its depth: in all
    (k_step(dim) + 1 + ceil(log2 dim) + depth) U N(E).  tests/test_fp64_bars.py: the fp32 oracle reaches 29 U at 516 dims on
    one-chain records (bar 44), 12 U at 260 (bar 43); two-term operands 175 and 233 U.  Mixtures: K_GMM + depth."""
    if case.family not in EMIT_FAMILIES:
        return K_REC_GAUSS if case.energy == "gauss" else K_REC_GMM
    depth = record_depth(case, layout)
    if case.energy == "gauss":
        return k_step(case.dim) + 1 + math.ceil(math.log2(case.dim)) + depth
    return K_GMM + depth


@dataclass
class RecordRefs:
    cnt: torch.Tensor      # [n_blocks, S] elements per slot
    sums: torch.Tensor     # [n_blocks, S] float64 column sums
    abs_sums: torch.Tensor  # ... of |x|: the sums' natural scale
    m2: torch.Tensor       # [n_blocks, S] sum (x - record mean)^2 about the float64 mean
    groups: list           # record_groups
    energy: torch.Tensor   # [groups] float64 energy sum of the group's chains
    energy_scale: torch.Tensor  # ... of N(E)
    accepts: torch.Tensor  # [groups] accepted chains


def record_refs(layout, n: int, dim: int, x, e64, nat, mask=None, clamp: Optional[float] = None) -> RecordRefs:
    """float64 references of every record from the state x [n, dim] the kernel itself returned; e64 / nat: energy64 of x;
    mask: the accept mask of the transition (HMC); clamp: the HMC records' energy clamp (1e10)."""
    nb, S, E = layout
    flat = x.double().flatten()
    cnt, sums, abs_sums, m2 = (torch.zeros(nb, S, dtype=torch.float64) for _ in range(4))
    for b, idx in enumerate(record_chains(layout, n, dim)):
        if idx.shape[0] == 0:
            continue
        v = flat[idx]
        cnt[b], sums[b], abs_sums[b] = idx.shape[0], v.sum(dim=0), v.abs().sum(dim=0)
        m2[b] = (v - v.mean(dim=0, keepdim=True)).square().sum(dim=0)
    groups = record_groups(layout, n, dim)
    e = e64 if clamp is None else e64.clamp(-clamp, clamp)
    energy = torch.stack([e[c].sum() for _, c in groups])
    scale = torch.stack([nat[c].sum() for _, c in groups])
    accepts = torch.stack([(mask[c] != 0).sum() if mask is not None else torch.tensor(0) for _, c in groups])
    return RecordRefs(cnt, sums, abs_sums, m2, groups, energy, scale, accepts)


def merge_records64(rec, layout, n: int, dim: int):
    """The exact merge of raw records [kept, n_blocks, 2 S + 8] in float64 by the pairwise-variance identity, as
    ebm_diag_finish_f32 documents it: (mean [kept, W], biased var [kept, W] clamped to [1e-10, 1e10] -- zero for a single
    row --, mean energy [kept], accepted fraction [kept]) over the n dim / W rows of width W = max(S, dim)."""
    nb, S, E = layout
    W = max(S, dim)
    rows = n * dim // W
    idx = record_chains(layout, n, dim)
    r = rec.double()
    kept = r.shape[0]
    tot, m2 = torch.zeros(kept, W, dtype=torch.float64), torch.zeros(kept, W, dtype=torch.float64)
    for b in range(nb):
        if idx[b].shape[0]:
            tot[:, idx[b][0] % W] += r[:, b, :S]
    mean = tot / rows
    for b in range(nb):
        m = idx[b].shape[0]
        if m:
            c = idx[b][0] % W
            m2[:, c] += r[:, b, S:2 * S] + m * (r[:, b, :S] / m - mean[:, c]).square()
    var = (m2 / rows).clamp(1e-10, 1e10) if rows > 1 else torch.zeros_like(m2)
    return mean, var, r[:, :, 2 * S:2 * S + 4].sum(dim=(1, 2)) / rows, r[:, :, 2 * S + 4:2 * S + 8].sum(dim=(1, 2)) / rows


# ----------------------------------------------------------------------------------------------------------------
# Running a case on the GPU
# ----------------------------------------------------------------------------------------------------------------
def device_model(case: Case, dev):
    """(model, fused spec, fp32 parameters as handed to the kernel: (mean, P) or (means, sigma, logw))."""
    import torchebm_amd as ta

    if case.energy == "gauss":
        mean, cov = gauss_params(case, 3.0 if case.sampler != "hmc" else 2.0)
        model = ta.GaussianModel(mean, cov, device=dev)
        spec = model.fused_spec()
        if not case.image:
            spec.aux = None
        torch.cuda.synchronize()
        return model, spec, (spec.dev0.cpu(), spec.dev1.cpu().view(case.dim, case.dim))
    means, sigma, weights = gmm_params(case)
    model = ta.GaussianMixtureModel(means, sigma=sigma, weights=weights, device=dev)
    spec = model.fused_spec()
    torch.cuda.synchronize()
    return model, spec, (means, sigma, model.log_weights.detach().cpu())


def cpu_params(case: Case):
    """the fp32 parameters a fused spec would hand the kernel, made on the CPU (GaussianModel / GaussianMixtureModel)."""
    import torchebm_amd as ta

    if case.energy == "gauss":
        mean, cov = gauss_params(case, 3.0 if case.sampler != "hmc" else 2.0)
        model = ta.GaussianModel(mean, cov)
        return model.mean.detach().clone(), sym_precision(model.cov_inv.detach())
    means, sigma, weights = gmm_params(case)
    model = ta.GaussianMixtureModel(means, sigma=sigma, weights=weights)
    return means, sigma, model.log_weights.detach().clone()


@dataclass
class Run:
    """what a chain call left behind (CPU tensors): the final state, the accept masks [T, n] (HMC), the trajectory
    [n, kept, dim], the raw records [kept, n_blocks, 2 S + 8] and their layout (n_blocks, S, E) as ebm_diag_layout gave it."""
    x: torch.Tensor
    mask: Optional[torch.Tensor] = None
    traj: Optional[torch.Tensor] = None
    rec: Optional[torch.Tensor] = None
    layout: Optional[Tuple[int, int, int]] = None


def _records(case: Case, spec, sampler_code, n, dim, injected, with_traj, kept, records, dev):
    from torchebm_amd import _lib

    if not (case.records if records is None else records):
        return None, None
    layout = _lib.diag_layout(spec.to_c(), sampler_code, n, dim, injected, with_traj)
    assert layout is not None, f"{case.id}: no in-kernel records for this shape"
    nb, S, _ = layout
    return layout, torch.zeros(max(kept, 1) * nb * (2 * S + 8), device=dev)


def _run(x, mask, traj, rec, layout, kept):
    torch.cuda.synchronize()
    if rec is not None:
        rec = rec.cpu().view(max(kept, 1), layout[0], 2 * layout[1] + 8)[:kept]
    return Run(x.cpu(), None if mask is None else mask.cpu(), None if traj is None else traj.cpu(), rec, layout)


def run_langevin(case: Case, spec, x0, eta: float, noise_field: bool, dev, k: int = 1, thin: int = 1, traj: bool = False,
                 records: Optional[bool] = None) -> Run:
    """k steps (one by default) through the fused chain entry: noise-free (noise_coef = 0, no noise pointer), or with an
    injected all-zero noise field and noise_coef != 0 (the kernels that read a noise field).  `records`: attach a record
    buffer (default: case.records -- that is what selects the records kernels); `traj`: hand over a trajectory pointer."""
    from torchebm_amd import _lib

    n, dim = case.n, case.dim
    heun = case.sampler == "heun"
    x = x0.to(dev).clone()
    noise = torch.zeros(k, n, dim, device=dev) if noise_field else None
    tr = torch.zeros(n, k // thin, dim, device=dev) if traj else None
    layout, rec = _records(case, spec, _lib.DIAG_LANGEVIN_HEUN if heun else _lib.DIAG_LANGEVIN, n, dim, noise_field, traj, k // thin,
                           records, dev)
    c = spec.to_c()
    _lib.call("ebm_langevin_heun_chain_f32" if heun else "ebm_langevin_chain_f32", c, x.data_ptr(), n, dim, k, eta, eta ** 0.5,
              1.4142135 if noise_field else 0.0, None, 0, 0.0, 0.0, thin, None if tr is None else tr.data_ptr(),
              None if rec is None else rec.data_ptr(), None if noise is None else noise.data_ptr(), 3, 0, _lib.stream_handle(dev))
    return _run(x, None, tr, rec, layout, k // thin)


def run_hmc(case: Case, spec, x0, p, u, mass, eps: float, dev, T: int = 1, L: int = 1, thin: int = 1, traj: bool = False,
            records: Optional[bool] = None) -> Run:
    """T transitions (one by default) of L leapfrog steps with injected momenta p [T, n, dim] and uniforms u [T, n]."""
    from torchebm_amd import _lib

    n, dim = case.n, case.dim
    x = x0.to(dev).clone()
    p_d, u_d = p.reshape(T, n, dim).to(dev).contiguous(), u.reshape(T, n).to(dev).contiguous()
    mask = torch.full((T, n), 7, dtype=torch.uint8, device=dev)
    tr = torch.zeros(n, T // thin, dim, device=dev) if traj else None
    kind, scalar, mdiag = _lib.MASS_NONE, 1.0, None
    if isinstance(mass, float):
        kind, scalar = _lib.MASS_SCALAR, mass
    elif mass is not None:
        kind, mdiag = _lib.MASS_DIAG, mass.to(dev).contiguous()
    layout, rec = _records(case, spec, _lib.DIAG_HMC, n, dim, True, traj, T // thin, records, dev)
    c = spec.to_c()
    _lib.call("ebm_hmc_chain_f32", c, x.data_ptr(), n, dim, T, L, eps, None, kind, scalar,
              None if mdiag is None else mdiag.data_ptr(), thin, None if tr is None else tr.data_ptr(),
              None if rec is None else rec.data_ptr(), mask.data_ptr(), None, p_d.data_ptr(), u_d.data_ptr(), 3, 0,
              _lib.stream_handle(dev))
    return _run(x, mask, tr, rec, layout, T // thin)


def diag_finish(run: Run, n: int, dim: int, dev, accept: bool):
    """ebm_diag_finish_f32 on the run's records: (mean [kept, W], var [kept, W], energy [kept], accept [kept] | None) with
    W = max(S, dim) -- packed rows (S > dim) are merged as the n dim / S rows of width S they are (include/ebm_hip.h)."""
    from torchebm_amd import _lib

    nb, S, E = run.layout
    kept = run.rec.shape[0]
    W = max(S, dim)
    rows = n * dim // W
    rec = run.rec.to(dev).contiguous()
    mean, var = torch.zeros(kept, W, device=dev), torch.zeros(kept, W, device=dev)
    energy, acc = torch.zeros(kept, device=dev), torch.zeros(kept, device=dev)
    work = torch.zeros(kept * (3 * W + 3), dtype=torch.float64, device=dev)
    _lib.call("ebm_diag_finish_f32", rec.data_ptr(), kept, nb, S, E, rows, W, mean.data_ptr(), var.data_ptr(), energy.data_ptr(),
              acc.data_ptr() if accept else None, work.data_ptr(), _lib.stream_handle(dev))
    torch.cuda.synchronize()
    return mean.cpu(), var.cpu(), energy.cpu(), acc.cpu() if accept else None
