// The Langevin half of the running-moments family: see moments_unit.hip.
#define EBM_MOMENTS_HMC 0
#include "moments_unit.hip"
