// hmc_unit.hip WITH the in-kernel diagnostics records; its own objects so that they build beside the plain ones.
#define EBM_UNIT_DIAG true
#include "hmc_unit.hip"
