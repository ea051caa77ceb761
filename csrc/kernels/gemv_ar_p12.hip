// The WF_P12 instantiations of the row-parallel decode GEMV with the all-reduce in its epilogue (EPI_AR;
// kernel body: gemv_core.h; geometry selection: gemv.hip's gemv_ar_geom, which hands the chosen (NT, UNROLL)
// over as data, so the blocks, the accumulation order and the granule ownership are the bf16 launch's). A
// translation unit of its own, as gemv_p12.hip and gemv_moe_p12.hip are, so that it compiles beside gemv.hip.
#include "gemv_core.h"

namespace llmc {

template <int M, int NT, int UNROLL, bool TAIL>
__global__ __launch_bounds__(NT) void gemv_ar_p12_kernel(const bf16_t* __restrict__ x, int x_stride,
                                                         const bf16_t* __restrict__ W, PackedW pw,
                                                         void* __restrict__ h, int h_stride, int N, int K,
                                                         CarArgs ar) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_block<M, NT, 1, UNROLL, PRO_NONE, EPI_AR, false, WF_P12, 1, TAIL>(blockIdx.x, blockIdx.y, smem, x, x_stride,
                                                                         nullptr, 0.f, W, h, h_stride, N, K, nullptr, 1,
                                                                         RopeEpi{}, ar, pw);
}

#define LLMC_AR_P12_ARGS                                                                                     \
  const void *x, int x_stride, const void *W, const PackedW &pw, void *h, int h_stride, int N, int K,        \
      const CarArgs &ar, hipStream_t s
#define LLMC_AR_P12_PASS x, x_stride, W, pw, h, h_stride, N, K, ar, s

template <int M, int NT, int UNROLL, bool TAIL>
static int launch_ar_p12(LLMC_AR_P12_ARGS) {
  constexpr int WAVES = NT / kWave;
  auto kern = gemv_ar_p12_kernel<M, NT, UNROLL, TAIL>;
  const size_t lds = static_cast<size_t>(M) * K * sizeof(bf16_t) + 2 * M * WAVES * sizeof(float);
  if (lds > 160 * 1024) return -2;
  static bool attr_set = false;
  if (lds > 64 * 1024 && !attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr_set = true;
  }
  const int grid = (N + WAVES - 1) / WAVES;
  if (grid > kMaxBlocks || static_cast<size_t>(grid) * kArGranulesPerBlock * 8 > static_cast<size_t>(ar.cap) / kMaxRanks)
    return -6;
  kern<<<grid, NT, lds, s>>>((const bf16_t*)x, x_stride, (const bf16_t*)W, pw, h, h_stride, N, K, ar);
  return static_cast<int>(hipGetLastError());
}

// every (NT, UNROLL) gemv_ar_geom returns
template <int M>
static int ar_p12_geom(int NT, int UNROLL, LLMC_AR_P12_ARGS) {
  const bool tail = K % kP13UnitElems != 0;
  // two rows, 16 waves, 8 loads per lane: 128 VGPRs are that block's limit, and the two-unit batch kept
  // per-lane state in scratch, as it does in gemv_p12.hip: one unit per batch there. A lane sums its
  // chunks in k order whatever the batch, so the bits stay (profiles/r13_packed_tp.md)
  if (M == 2 && NT == 1024 && UNROLL == 8) UNROLL = 4;
#define LLMC_AR_P12_GEOM(nt, un)                                                   \
  if (NT == nt && UNROLL == un) {                                                  \
    if constexpr (!(M == 2 && nt == 1024 && un == 8)) {                            \
      if (tail) return launch_ar_p12<M, nt, un, true>(LLMC_AR_P12_PASS);           \
      return launch_ar_p12<M, nt, un, false>(LLMC_AR_P12_PASS);                    \
    }                                                                              \
  }
  LLMC_AR_P12_GEOM(1024, 8)
  LLMC_AR_P12_GEOM(640, 8)
  LLMC_AR_P12_GEOM(1024, 4)
  LLMC_AR_P12_GEOM(768, 4)
  LLMC_AR_P12_GEOM(640, 4)
  LLMC_AR_P12_GEOM(512, 4)
  LLMC_AR_P12_GEOM(256, 8)
#undef LLMC_AR_P12_GEOM
  return -8;
}

int launch_gemv_ar_p12(int M, int NT, int UNROLL, LLMC_AR_P12_ARGS) {
  switch (M) {
    case 1: return ar_p12_geom<1>(NT, UNROLL, LLMC_AR_P12_PASS);
    case 2: return ar_p12_geom<2>(NT, UNROLL, LLMC_AR_P12_PASS);
    default: return -3;
  }
}

}  // namespace llmc
