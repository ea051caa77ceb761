// The WF_P12 instantiations of the MoE decode GEMVs (kernel body: gemv_core.h; geometry selection:
// gemv.hip's moe_gemv_geom, which hands the chosen (NT, RPW) over as data, and llmc_moe_down_combine's
// fixed 1024 x 2). The expert stack [E, N, K] is packed as its [E * N, K] view, so row n of expert e is
// row e * N + n of the twin. A translation unit of its own, as gemv_p12.hip is, so that it compiles
// beside gemv.hip.
#include "gemv_core.h"

namespace llmc {

// M = 1: the pair form (by = (token, slot) pair); M = 2 with EPI_COMBINE: by = token, RPW = M = top-k
template <int M, int NT, int RPW, int PRO, int EPI>
__global__ __launch_bounds__(NT) void gemv_moe_p12_kernel(const bf16_t* __restrict__ x, int x_stride,
                                                          const bf16_t* __restrict__ norm_w, float eps,
                                                          const bf16_t* __restrict__ W, PackedW pw,
                                                          void* __restrict__ out, int out_stride, int N, int K,
                                                          const int32_t* __restrict__ expert_ids, int x_div,
                                                          RopeEpi rope) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_block<M, NT, RPW, 4, PRO, EPI, true, WF_P12>(blockIdx.x, blockIdx.y, smem, x, x_stride, norm_w, eps, W, out,
                                                    out_stride, N, K, expert_ids, x_div, rope, CarArgs{}, pw);
}

#define LLMC_MOE_P12_ARGS                                                                                       \
  int npairs, const void *x, int x_stride, const void *nw, float eps, const void *W, const PackedW &pw,         \
      const void *ids, int x_div, void *out, int out_stride, int N, int K, hipStream_t s
#define LLMC_MOE_P12_PASS npairs, x, x_stride, nw, eps, W, pw, ids, x_div, out, out_stride, N, K, s

template <int NT, int RPW, int PRO, int EPI>
static int launch_moe_p12(LLMC_MOE_P12_ARGS) {
  constexpr int WAVES = NT / kWave;
  const size_t lds = static_cast<size_t>(K) * sizeof(bf16_t) + 2 * WAVES * sizeof(float);
  if (lds > 64 * 1024) return -2;
  dim3 grid((N + WAVES * RPW - 1) / (WAVES * RPW), npairs);
  gemv_moe_p12_kernel<1, NT, RPW, PRO, EPI><<<grid, NT, lds, s>>>(
      (const bf16_t*)x, x_stride, (const bf16_t*)nw, eps, (const bf16_t*)W, pw, out, out_stride, N, K,
      (const int32_t*)ids, x_div, RopeEpi{});
  return static_cast<int>(hipGetLastError());
}

// every (NT, RPW) moe_gemv_geom returns: the SiLU pairs in one wave (1024 / 896 x 2), one row per wave
// at pick_waves' block (14 waves: paired outputs only), and 256 x 2 where no paired block tiles
template <int PRO, int EPI>
static int moe_p12_geom(int NT, int RPW, LLMC_MOE_P12_ARGS) {
#define LLMC_MOE_P12_GEOM(nt, rpw) \
  if (NT == nt && RPW == rpw) return launch_moe_p12<nt, rpw, PRO, EPI>(LLMC_MOE_P12_PASS);
  LLMC_MOE_P12_GEOM(1024, 1)
  LLMC_MOE_P12_GEOM(768, 1)
  LLMC_MOE_P12_GEOM(640, 1)
  LLMC_MOE_P12_GEOM(512, 1)
  LLMC_MOE_P12_GEOM(256, 1)
  if constexpr (EPI == EPI_SILU) {
    LLMC_MOE_P12_GEOM(1024, 2)
    LLMC_MOE_P12_GEOM(896, 2)
    LLMC_MOE_P12_GEOM(896, 1)
    LLMC_MOE_P12_GEOM(256, 2)
  }
#undef LLMC_MOE_P12_GEOM
  return -8;
}

int launch_moe_gemv_p12(int NT, int RPW, int pro, int epi, LLMC_MOE_P12_ARGS) {
  if (epi == EPI_SILU)
    return pro == PRO_NORM ? moe_p12_geom<PRO_NORM, EPI_SILU>(NT, RPW, LLMC_MOE_P12_PASS)
                           : moe_p12_geom<PRO_NONE, EPI_SILU>(NT, RPW, LLMC_MOE_P12_PASS);
  if (epi == EPI_BF16 && pro == PRO_NONE) return moe_p12_geom<PRO_NONE, EPI_BF16>(NT, RPW, LLMC_MOE_P12_PASS);
  return -8;
}

int launch_moe_combine_p12(int T, const void* act, int act_stride, const void* W, const PackedW& pw, const void* ids,
                           const void* w, void* h, int h_stride, int N, int K, hipStream_t s) {
  constexpr int NT = 1024, WAVES = NT / kWave;
  auto kern = gemv_moe_p12_kernel<2, NT, 2, PRO_NONE, EPI_COMBINE>;
  const size_t lds = static_cast<size_t>(2) * K * sizeof(bf16_t) + 2 * 2 * WAVES * sizeof(float);
  if (lds > 160 * 1024) return -2;
  static bool attr_set = false;
  if (lds > 64 * 1024 && !attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr_set = true;
  }
  RopeEpi wts{};
  wts.cos_t = static_cast<const float*>(w);
  dim3 grid((N + WAVES - 1) / WAVES, T);
  kern<<<grid, NT, lds, s>>>((const bf16_t*)act, act_stride, nullptr, 0.f, (const bf16_t*)W, pw, h, h_stride, N, K,
                             (const int32_t*)ids, 1, wts);
  return static_cast<int>(hipGetLastError());
}

}  // namespace llmc
