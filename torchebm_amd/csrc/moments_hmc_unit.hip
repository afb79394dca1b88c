// The HMC half of the running-moments family: see moments_unit.hip.
#define EBM_MOMENTS_HMC 1
#include "moments_unit.hip"
