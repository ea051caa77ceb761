// The WF_P12 instantiations of the decode GEMV (kernel body: gemv_core.h; geometry selection:
// gemv.hip, which hands the chosen (NT, RPW, UNROLL) over as data). A translation unit of its own so
// that it compiles beside gemv.hip instead of doubling that file's build time.
#include "gemv_core.h"

namespace llmc {

#define LLMC_P12_ARGS                                                                                             \
  const void *x, int x_stride, const void *nw, float eps, const void *W, const PackedW &pw, void *out, int out_stride, \
      int N, int K, const RopeEpi &rope, hipStream_t s
#define LLMC_P12_PASS x, x_stride, nw, eps, W, pw, out, out_stride, N, K, rope, s

template <int M, int NT, int RPW, int UNROLL, int PRO, int EPI, bool TAIL>
static int launch_p12(LLMC_P12_ARGS) {
  constexpr int WAVES = NT / kWave;
  auto kern = gemv_p12_kernel<M, NT, RPW, UNROLL, PRO, EPI, 1, TAIL>;
  const size_t lds = static_cast<size_t>(M) * K * sizeof(bf16_t) + 2 * M * WAVES * sizeof(float);
  if (lds > 160 * 1024) return -2;
  static bool attr_set = false;
  if (lds > 64 * 1024 && !attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr_set = true;
  }
  const int rows_per_block = WAVES * RPW;
  const int grid = (N + rows_per_block - 1) / rows_per_block;
  kern<<<grid, NT, lds, s>>>((const bf16_t*)x, x_stride, (const bf16_t*)nw, eps, (const bf16_t*)W, pw, out, out_stride,
                             N, K, rope);
  return static_cast<int>(hipGetLastError());
}

// the geometries of gemv.hip's launch_gemv
template <int M, int PRO, int EPI>
static int p12_geom(int NT, int RPW, int UNROLL, LLMC_P12_ARGS) {
  // two rows, 16 waves, 8 loads per lane with the RoPE epilogue kept 20 B per lane in scratch: one
  // unit per batch there. A lane sums its chunks in k order whatever the batch, so the bits stay.
  if (M == 2 && NT == 1024 && RPW == 1 && UNROLL == 8 && EPI == EPI_ROPE) UNROLL = 4;
  // DEPTH stays 1: two batches ahead (gemv_block's DEPTH = 2) measured slower on every 8B shape but
  // lm_head, where it was equal (profiles/r10_packed12.md §3), so it is not instantiated
  // A K off the 2048-weight unit runs the TAIL instantiation, a K on it the one without: the tail is a
  // template flag and not a branch of one kernel, so the kernels of the whole-unit shapes are the code
  // they were before there was a tail (profiles/r11_packed_tail.md §2)
  const bool tail = K % kP13UnitElems != 0;
  // ... and with a tail the two-row, 16-wave, 8-loads form kept 36 B per lane in scratch under every
  // epilogue (128 VGPRs are its limit): one unit per batch there too, the same order, the same bits
  if (tail && M == 2 && NT == 1024 && RPW == 1 && UNROLL == 8) UNROLL = 4;
#define LLMC_P12_GEOM(nt, rpw, un)                                                              \
  if (NT == nt && RPW == rpw && UNROLL == un) {                                                 \
    if constexpr (!(M == 2 && nt == 1024 && rpw == 1 && un == 8))                               \
      if (tail) return launch_p12<M, nt, rpw, un, PRO, EPI, true>(LLMC_P12_PASS);               \
    return launch_p12<M, nt, rpw, un, PRO, EPI, false>(LLMC_P12_PASS);                          \
  }
  LLMC_P12_GEOM(1024, 1, 4)
  LLMC_P12_GEOM(896, 1, 4)
  LLMC_P12_GEOM(768, 1, 4)
  LLMC_P12_GEOM(640, 1, 4)
  LLMC_P12_GEOM(512, 1, 4)
  LLMC_P12_GEOM(1024, 2, 4)
  LLMC_P12_GEOM(896, 2, 4)
  LLMC_P12_GEOM(768, 2, 4)
  LLMC_P12_GEOM(256, 2, 4)
  LLMC_P12_GEOM(640, 1, 8)
  LLMC_P12_GEOM(256, 1, 8)
  if constexpr (!(M == 2 && EPI == EPI_ROPE)) {
    LLMC_P12_GEOM(1024, 1, 8)
  }
#undef LLMC_P12_GEOM
  return -8;
}

template <int PRO, int EPI>
static int p12_rows(int M, int NT, int RPW, int UNROLL, LLMC_P12_ARGS) {
  switch (M) {
    case 1: return p12_geom<1, PRO, EPI>(NT, RPW, UNROLL, LLMC_P12_PASS);
    case 2: return p12_geom<2, PRO, EPI>(NT, RPW, UNROLL, LLMC_P12_PASS);
    default: return -3;
  }
}

int launch_gemv_p12(int M, int NT, int RPW, int UNROLL, int pro, int epi, LLMC_P12_ARGS) {
#define LLMC_P12_CASE(E)                                                                  \
  case E:                                                                                 \
    return pro == PRO_NORM ? p12_rows<PRO_NORM, E>(M, NT, RPW, UNROLL, LLMC_P12_PASS)     \
                           : p12_rows<PRO_NONE, E>(M, NT, RPW, UNROLL, LLMC_P12_PASS);
  switch (epi) {
    LLMC_P12_CASE(EPI_BF16)
    LLMC_P12_CASE(EPI_F32)
    LLMC_P12_CASE(EPI_RESADD)
    LLMC_P12_CASE(EPI_SILU)
    case EPI_ROPE:
      if (pro != PRO_NORM) return -5;
      return p12_rows<PRO_NORM, EPI_ROPE>(M, NT, RPW, UNROLL, LLMC_P12_PASS);
    default: return -4;
  }
#undef LLMC_P12_CASE
}

}  // namespace llmc
