// The WF_P12 instantiations of the decode GEMV (kernel body: gemv_core.h; geometry rule and list:
// gemv_geom.h; launcher and lookup: gemv_launch.h). A translation unit of its own so that it compiles
// beside gemv.hip instead of doubling that file's build time.
#include "gemv_launch.h"

namespace llmc {

GemvLaunch gemv_find_dense_p12(int M, int pro, int epi, GemvGeom g, bool tail) {
  return gemv_find<GEMV_DENSE, WF_P12>(M, pro, epi, g, tail);
}

}  // namespace llmc
