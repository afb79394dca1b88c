// The BAOAB half of the kinetic running-moments family: see kinetic_moments_unit.hip.
#define EBM_KINETIC_MOMENTS_GHMC 0
#include "kinetic_moments_unit.hip"
