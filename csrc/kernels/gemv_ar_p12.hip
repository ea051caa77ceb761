// The WF_P12 instantiations of the row-parallel decode GEMV with the all-reduce in its epilogue (EPI_AR;
// kernel body: gemv_core.h; geometry rule and list: gemv_geom.h, so the blocks, the accumulation order and
// the granule ownership are the bf16 launch's; launcher and lookup: gemv_launch.h). A translation unit of
// its own, as gemv_p12.hip and gemv_moe_p12.hip are, so that it compiles beside gemv.hip.
#include "gemv_launch.h"

namespace llmc {

GemvLaunch gemv_find_ar_p12(int M, int pro, int epi, GemvGeom g, bool tail) {
  return gemv_find<GEMV_AR, WF_P12>(M, pro, epi, g, tail);
}

}  // namespace llmc
