// Generalized HMC, the three element-wise entries on the shared walker (ebm_ghmc_chain_f32, ebm_ghmc_adapt_chain_f32,
// ebm_ghmc_adapt_chain_mass_f32): geometry, refusals and dispatch to the per-energy units (ghmc_unit.hip, ghmc_adapt_unit.hip,
// ghmc_adapt_mass_unit.hip, one object per family and kind; the kernels: ghmc_kernel.h).  ebm_ghmc_chain_mass_f32: ghmc_mass.hip.
#include <cmath>

#include "ghmc_kernel.h"
#include "ghmc_adapt_mass_launch.h"

namespace ebm {

// The refusal that depends on the lane geometry (no launch, no device access): the entries call this in front of their early
// return for an empty call, so it needs no GPU.
int ghmc_check_geometry(int32_t dim) {
  rows::Geometry geo;
  if (dim < 1 || !rows::pick_geometry(dim, geo) || geo.NV != 1)
    return fail(EBM_EDIM, "ebm_ghmc_chain_f32: dim %d outside 1 .. 256 is not supported (one vector per lane)", dim);
  return 0;
}

int ghmc_adapt_check(const GhmcAdaptChainReq& q, const char* who) {
  if (!q.da) return fail(EBM_EINVAL, "%s: da pointer is NULL", who);
  if (q.n_adapt < 0 || q.n_adapt > q.n_mh)
    return fail(EBM_EINVAL, "%s: n_adapt=%d outside 0 .. n_mh=%d", who, q.n_adapt, q.n_mh);
  if (q.n_adapt > 0 && !q.da_table) return fail(EBM_EINVAL, "%s: da_table pointer is NULL with n_adapt=%d", who, q.n_adapt);
  if (q.init_da < 0 || q.init_da > (EBM_DA_INIT | EBM_DA_OPEN)) return fail(EBM_EINVAL, "%s: init_da=%d (bits 0 .. 1)", who, q.init_da);
  if (!(q.target_accept > 0.0 && q.target_accept < 1.0))
    return fail(EBM_EINVAL, "%s: target_accept=%g (must lie in (0, 1))", who, q.target_accept);
  if (!(q.eps0 > 0.0) || !(q.eps_min > 0.0) || !(q.eps_max > 0.0) || !std::isfinite(q.eps0) || !std::isfinite(q.eps_min) ||
      !std::isfinite(q.eps_max) || q.eps_min > q.eps_max)
    return fail(EBM_EINVAL, "%s: eps0=%g eps_min=%g eps_max=%g (all must be positive and finite, eps_min <= eps_max)", who, q.eps0,
                q.eps_min, q.eps_max);
  if (!std::isfinite(q.mu)) return fail(EBM_EINVAL, "%s: mu=%g (must be finite)", who, q.mu);
  return 0;
}

namespace {

// The step-size part and the two temperature constants: a fixed step's arrive rounded (GhmcChainReq) ...
void fill_step(ghmc::FixedStep& s, ghmc::WalkArgs& w, const GhmcChainReq& q) {
  s.eps = q.eps; s.c1 = q.c1; s.c2 = q.c2;
  w.sqrt_temp = q.sqrt_temp; w.beta = q.beta;
}

// ... an adapting step's as doubles: every double rounded once; gamma L and the two logs formed in double
void fill_step(ghmc::AdaptStep& s, ghmc::WalkArgs& w, const GhmcAdaptChainReq& q) {
  s.n_adapt = q.n_adapt; s.init_da = (q.init_da & EBM_DA_INIT) ? 1 : 0; s.keep_open = (q.init_da & EBM_DA_OPEN) ? 1 : 0;
  s.full_refresh = std::isinf(q.gamma) ? 1 : 0;
  s.eps0 = (float)q.eps0;
  s.gamma_l = s.full_refresh ? 0.0f : (float)(q.gamma * (double)q.n_leapfrog);
  s.temp = (float)q.temperature; w.sqrt_temp = (float)sqrt(q.temperature); w.beta = (float)(1.0 / q.temperature);
  s.delta = (float)q.target_accept; s.mu = (float)q.mu;
  s.log_eps_min = (float)log(q.eps_min); s.log_eps_max = (float)log(q.eps_max);
  s.da = q.da; s.da_table = q.da_table; s.eps_trace = q.eps_trace; s.alpha_mean = q.alpha_mean;
}

// What the three launches share: the geometry, the fields every walker reads (the two request types name them alike), the
// step-size part, the block-count refusal and the dispatch on the energy kind.  `a` arrives zeroed, its mass part filled.
template <class Args, class Req>
int launch(const char* who, const Req& q, Args& a, hipStream_t st) {
  using namespace rows;
  if (int r = ghmc_check_geometry(q.dim)) return r;
  Geometry geo;
  pick_geometry(q.dim, geo);
  ghmc::WalkArgs& w = a.w;
  w.x = q.x; w.v = q.v; w.n_chains = q.n_chains; w.dim = q.dim; w.n_mh = q.n_mh; w.n_leapfrog = q.n_leapfrog;
  w.thin = q.thin; w.n_kept = q.n_kept(); w.draw_v0 = q.draw_v0 ? 1 : 0;
  w.traj = q.traj; w.accept_mask = q.accept_mask; w.noise = q.noise; w.u = q.u;
  w.key = q.key(); w.step0 = q.offset;
  fill_step(a.step, w, q);
  size_t smem = 0;
  plan_params(q.e, q.dim, geo, w.energy, w.param_floats, smem);
  const int64_t blocks = blocks_for(q.n_chains, geo);
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  const dim3 grid((unsigned)blocks);
  for_kind(q.e.kind, [&](auto K) { ghmc::launch_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  return check_launch(who);
}

}  // namespace

int ghmc_chain_launch(const GhmcChainReq& q, hipStream_t st) {
  ghmc::GhmcArgs a{};
  return launch("ebm_ghmc_chain_f32", q, a, st);
}

int ghmc_adapt_chain_launch(const GhmcAdaptChainReq& q, hipStream_t st) {
  ghmc::GhmcAdaptArgs a{};
  return launch("ebm_ghmc_adapt_chain_f32", q, a, st);
}

int ghmc_adapt_mass_chain_launch(const GhmcAdaptMassChainReq& m, hipStream_t st) {
  ghmc::GhmcAdaptMassArgs a{};
  fill_mass(a.mass, m.mass);
  return launch("ebm_ghmc_adapt_chain_mass_f32", m.chain, a, st);
}

}  // namespace ebm
