// What the two massed walks on the wide MLP energy share (mlp_wide_kinetic_mass_body.h, mlp_wide_ghmc_mass_body.h;
// docs/design/mass_mlp.md): the per-column forms of a scalar or diagonal mass, kept as TABLES in LDS behind the layout of
// mlp_wide_setup.inc, and the launch that asks for them.  The walk kernels sit at the register limit (mlp_wide_rows.h): a lane
// holds 16 DT columns that depend on its K-half, so a mass form kept in registers through the evaluations would cost 16 DT
// registers each.  A table is kMassCols floats, 1 at and beyond dim (x and p stay 0 there); a register quad -- four aligned columns
// c0 = 32 td + 8 q + 4 hq -- reads one 16-byte LDS vector where it is used, through an address the compiler cannot carry from
// one use to the next.  Either mass form fills the same tables, so one kernel serves both; mass_kind stays a wave-uniform
// argument that selects the form of the kinetic energy.  The unit-mass walks include nothing of this.
#pragma once
#include "mlp_wide_rows.h"

namespace ebm {
namespace widemlp {

constexpr int kMassCols = 128;  // the widest state: four tiles of 32 columns

// LDS bytes of a massed walk: the unit-mass layout and TABLES tables behind it
__host__ __device__ constexpr size_t wide_mass_smem_bytes(int ht, int dt, int mode, int tables) {
  return wide_smem_bytes(ht, dt, mode) + (size_t)tables * kMassCols * sizeof(float);
}

// The three forms of the mass at column c as hmc::mass_forms builds them -- raw (kinetic energy), sqrt (refresh, start draw),
// clamped (drift) --, 1 at and beyond dim.  The scalar forms come formed in double and rounded once (fill_scalar_mass); sqrtf is
// correctly rounded (hipcc's default).  Args: mass_kind, mass_raw, mass_sqrt, mass_safe, mass_diag, dim (fill_mass).
template <class Args>
__device__ __forceinline__ void mass_forms_at(const Args& a, int c, float& m_raw, float& m_sqrt, float& m_safe) {
  m_raw = 1.0f; m_sqrt = 1.0f; m_safe = 1.0f;
  if (c < a.dim) {
    if (a.mass_kind == EBM_MASS_DIAG) {
      m_raw = a.mass_diag[c];
      m_sqrt = sqrtf(m_raw);
      m_safe = m_raw < 1e-10f ? 1e-10f : m_raw;
    } else {
      m_raw = a.mass_raw; m_sqrt = a.mass_sqrt; m_safe = a.mass_safe;
    }
  }
}

// the four entries of a table at the quad's first column c0 (a multiple of 4)
__device__ __forceinline__ void table_quad(float (&t)[4], const float* table, int c0) {
  const float4 w = *reinterpret_cast<const float4*>(table + c0);
  t[0] = w.x; t[1] = w.y; t[2] = w.z; t[3] = w.w;
}

// The start draw of the momentum, p = (sqrt_temp m_sqrt_j) z0 with z0 the field at step0, zero beyond dim (wave-uniform
// caller; the unit-mass walks' draw with the m_sqrt table's factor)
template <int DT, class Args>
__device__ __forceinline__ void draw_momentum(const Lanes& L, float (&p)[DT][16], const Args& a, const float* m_sqrt_table,
                                              int64_t row) {
#pragma unroll
  for (int td = 0; td < DT; ++td)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c0 = 32 * td + 8 * q + 4 * L.h;
      float z[4], ms[4];
      normal_quad(L, z, a.key, c0, row, a.step0);
      table_quad(ms, m_sqrt_table, c0);
#pragma unroll
      for (int i = 0; i < 4; ++i) p[td][4 * q + i] = (c0 + i < L.dim) ? (a.sqrt_temp * ms[i]) * z[i] : 0.0f;
    }
}

// launch_walk (mlp_wide_rows.h) with the tables' LDS behind the unit-mass layout
template <auto KERNEL, int HT, int DT, int MODE, int TABLES, class Args>
int launch_massed_walk(const Args& a, hipStream_t st, const char* who) {
  constexpr size_t smem = wide_mass_smem_bytes(HT, DT, MODE, TABLES);
  static_assert(wide_smem_bytes(HT, DT, MODE) % 16 == 0, "the tables are read as 16-byte vectors");
  static_assert(smem <= 160 * 1024, "one workgroup's LDS");
  static DeviceOnce attr_once;  // the LDS opt-in is a per-device function attribute
  if (attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  }
  const int64_t blocks = ceil_div64(a.n_chains, 32 * (kBlock / 64));
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)blocks), dim3(kBlock), smem, st, a);
  return check_launch(who);
}

// ... of the kernel for a.dim among a family's at hidden width 32 HT (launch_walk_by_dim); WALK also says `tables`
template <class WALK, int HT, class Args>
int launch_massed_walk_by_dim(const Args& a, hipStream_t st, const char* who) {
  const auto at = [&](auto dt) {
    constexpr int DT = decltype(dt)::value, MODE = wide_mode(HT, DT);
    return launch_massed_walk<WALK::template kernel<HT, DT, MODE>, HT, DT, MODE, WALK::tables>(a, st, who);
  };
  switch ((a.dim + 31) / 32) {
    case 1: return at(std::integral_constant<int, 1>{});
    case 2: return at(std::integral_constant<int, 2>{});
    case 3: return at(std::integral_constant<int, 3>{});
    default: return at(std::integral_constant<int, 4>{});
  }
}

}  // namespace widemlp
}  // namespace ebm
