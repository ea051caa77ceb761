// The WF_P12 instantiations of the MoE decode GEMVs, the pair form and the down projection fused with the
// top-2 combine (kernel body: gemv_core.h; geometry rule and lists: gemv_geom.h; launcher and lookup:
// gemv_launch.h). The expert stack [E, N, K] is packed as its [E * N, K] view, so row n of expert e is
// row e * N + n of the twin. A translation unit of its own, as gemv_p12.hip is, so that it compiles
// beside gemv.hip.
#include "gemv_launch.h"

namespace llmc {

GemvLaunch gemv_find_moe_p12(GemvOp op, int M, int pro, int epi, GemvGeom g) {
  return op == GEMV_MOE_COMBINE ? gemv_find<GEMV_MOE_COMBINE, WF_P12>(M, pro, epi, g, false)
                                : gemv_find<GEMV_MOE_PAIR, WF_P12>(M, pro, epi, g, false);
}

}  // namespace llmc
