// The three-hidden-layer MLP energy at hidden width 128, dim <= 32: mlp3_body.h at HT = 4, DT = 1 -- fp32 weights resident in
// LDS (151 040 of 163 840 bytes), every contraction on the exact-f32 matrix instruction (docs/design/mlp3.md).
#include "mlp3_body.h"

namespace ebm {
namespace mlp3 {

int launch_h128(const Args& a, hipStream_t st, const char* who) { return launch<4, 1>(a, st, who); }

}  // namespace mlp3
}  // namespace ebm
