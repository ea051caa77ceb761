// Host side of the decode GEMV launches (kernel body: gemv_core.h; geometry rule and the lists of
// instantiated geometries: gemv_geom.h), shared by gemv.hip (the bf16 and P13 kernels) and the three WF_P12
// translation units: one launcher and one "kernel of this geometry" lookup for every op and weight format.
// Lookup and launch are separate steps: the launch entries and llmc_gemv_plan ask the same lookup.
#pragma once
#include <utility>

#include "gemv_core.h"

namespace llmc {

// One launch's arguments, whatever the op. What an op does not take stays as initialised here.
struct GemvArgs {
  const void* x;  // [M or tokens][x_stride] bf16 (COMBINE: the slots' activations)
  int x_stride;
  const void* nw;  // PRO_NORM: the RMS-norm weights
  float eps;
  const void* W;
  PackedW pw;  // the packed twin of W; wf == WF_BF16: none
  void* out;   // (AR, COMBINE: h, accumulated in place)
  int out_stride, N, K;
  const void* ids;  // MoE: expert ids, read on device
  int x_div = 1;    // MOE_PAIR: pairs per x row
  int ny = 1;       // MoE: the grid's y, (token, slot) pairs or tokens
  RopeEpi rope;     // EPI_ROPE; COMBINE: the router weights in cos_t
  CarArgs ar;       // EPI_AR
  hipStream_t s;
};
using GemvLaunch = int (*)(const GemvArgs&);

// A block's dynamic LDS: x [M][K] bf16 | norm partials [M][WAVES] f32 | pair exchange or EPI_AR row values
// [M][WAVES] f32. Above 64 KiB the kernel's limit is raised, once per kernel. 0: above `limit`.
template <auto KERN>
static size_t gemv_lds(int M, int K, int waves, size_t limit) {
  const size_t lds = static_cast<size_t>(M) * K * sizeof(bf16_t) + 2 * M * waves * sizeof(float);
  if (lds > limit) return 0;
  static bool attr_set = false;
  if (lds > 64 * 1024 && !attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr_set = true;
  }
  return lds;
}

template <GemvOp OP, int WF, bool TAIL, int M, int NT, int RPW, int UNROLL, int PRO, int EPI>
constexpr auto gemv_kernel_of() {
  constexpr bool moe = OP == GEMV_MOE_PAIR || OP == GEMV_MOE_COMBINE;
  if constexpr (WF == WF_BF16) {
    return gemv_kernel<M, NT, RPW, UNROLL, PRO, EPI, moe>;
  } else if constexpr (WF == WF_P13) {
    return gemv_p13_kernel<M, NT, RPW, UNROLL, PRO, EPI>;
  } else if constexpr (OP == GEMV_DENSE) {
    // DEPTH stays 1: two batches ahead (gemv_block's DEPTH = 2) measured slower on every 8B shape but
    // lm_head, where it was equal (profiles/r10_packed12.md §3), so it is not instantiated.
    // A K off the 2048-weight unit runs the TAIL instantiation, a K on it the one without: the tail is a
    // template flag and not a branch of one kernel, so the kernels of the whole-unit shapes are the code
    // they were before there was a tail (profiles/r11_packed_tail.md §2)
    return gemv_p12_kernel<M, NT, RPW, UNROLL, PRO, EPI, 1, TAIL>;
  } else if constexpr (OP == GEMV_AR) {
    return gemv_ar_p12_kernel<M, NT, UNROLL, TAIL>;
  } else {
    static_assert(UNROLL == 4 && !TAIL, "packed expert weights: one unit per batch, no tail");
    return gemv_moe_p12_kernel<M, NT, RPW, PRO, EPI>;
  }
}

template <GemvOp OP, int WF, bool TAIL, int M, int NT, int RPW, int UNROLL, int PRO, int EPI>
static int gemv_launch(const GemvArgs& a) {
  constexpr int WAVES = NT / kWave;
  constexpr bool moe = OP == GEMV_MOE_PAIR || OP == GEMV_MOE_COMBINE;
  constexpr auto kern = gemv_kernel_of<OP, WF, TAIL, M, NT, RPW, UNROLL, PRO, EPI>();
  // the pair form keeps the default 64 KiB (one x row); 160 KiB is the CU's LDS
  const size_t lds = gemv_lds<kern>(M, a.K, WAVES, (OP == GEMV_MOE_PAIR ? 64 : 160) * 1024);
  if (lds == 0) return -2;
  // COMBINE: a wave's RPW rows are one output row of the token's RPW experts
  constexpr int rows_per_block = OP == GEMV_MOE_COMBINE ? WAVES : WAVES * RPW;
  const dim3 grid((a.N + rows_per_block - 1) / rows_per_block, moe ? a.ny : 1);
  if constexpr (OP == GEMV_AR) {
    if (static_cast<int>(grid.x) > kMaxBlocks ||
        static_cast<size_t>(grid.x) * kArGranulesPerBlock * 8 > static_cast<size_t>(a.ar.cap) / kMaxRanks)
      return -6;
  }
  const bf16_t *x = static_cast<const bf16_t*>(a.x), *nw = static_cast<const bf16_t*>(a.nw),
               *W = static_cast<const bf16_t*>(a.W);
  const int32_t* ids = static_cast<const int32_t*>(a.ids);
  if constexpr (WF == WF_BF16) {
    kern<<<grid, NT, lds, a.s>>>(x, a.x_stride, nw, a.eps, W, a.out, a.out_stride, a.N, a.K, ids, a.x_div, a.rope,
                                 a.ar);
  } else if constexpr (OP == GEMV_DENSE) {
    kern<<<grid, NT, lds, a.s>>>(x, a.x_stride, nw, a.eps, W, a.pw, a.out, a.out_stride, a.N, a.K, a.rope);
  } else if constexpr (OP == GEMV_AR) {
    kern<<<grid, NT, lds, a.s>>>(x, a.x_stride, W, a.pw, a.out, a.out_stride, a.N, a.K, a.ar);
  } else {
    kern<<<grid, NT, lds, a.s>>>(x, a.x_stride, nw, a.eps, W, a.pw, a.out, a.out_stride, a.N, a.K, ids, a.x_div,
                                 a.rope);
  }
  return static_cast<int>(hipGetLastError());
}

// The launcher of geometry g among the op's list (gemv_geom.h), or null. tail (WF_P12): K is off the
// 2048-weight unit. Kernels that gemv_geom never asks for are not instantiated: geometries past their
// rows or off their epilogues, and the packed two-row forms that run 4 loads per lane (p12_runs_4_loads).
template <GemvOp OP, int WF, int M, int PRO, int EPI>
static GemvLaunch gemv_find_geom(GemvGeom g, bool tail) {
  constexpr bool moe = OP == GEMV_MOE_PAIR || OP == GEMV_MOE_COMBINE;
#define LLMC_GEMV_X(nt, rpw, un, maxm, epis)                                                                  \
  if constexpr (M <= maxm && gemv_geom_serves(epis, EPI)) {                                                   \
    if (g == GemvGeom{nt, rpw, un}) {                                                                         \
      if constexpr (WF == WF_P12 && !moe && !p12_runs_4_loads(M, GemvGeom{nt, rpw, un}, EPI, true)) {         \
        if (tail) return gemv_launch<OP, WF, true, M, nt, rpw, un, PRO, EPI>;                                 \
      }                                                                                                       \
      if constexpr (!(WF == WF_P12 && p12_runs_4_loads(M, GemvGeom{nt, rpw, un}, EPI, false))) {              \
        if (!tail) return gemv_launch<OP, WF, false, M, nt, rpw, un, PRO, EPI>;                               \
      }                                                                                                       \
    }                                                                                                         \
  }
  if constexpr (OP == GEMV_DENSE) {
    LLMC_GEMV_DENSE_GEOMS(LLMC_GEMV_X)
  } else if constexpr (OP == GEMV_AR) {
    LLMC_GEMV_AR_GEOMS(LLMC_GEMV_X)
  } else if constexpr (OP == GEMV_MOE_PAIR) {
    LLMC_GEMV_MOE_GEOMS(LLMC_GEMV_X)
  } else {
    LLMC_GEMV_COMBINE_GEOMS(LLMC_GEMV_X)
  }
#undef LLMC_GEMV_X
  return nullptr;
}

// ... of the case (M rows per block, pro, epi), over every case the op has in this format (gemv_case_exists):
// I counts (M - 1, pro, epi)
template <GemvOp OP, int WF, int M, int PRO, int EPI>
static void gemv_find_case(int m, int pro, int epi, GemvGeom g, bool tail, GemvLaunch& f) {
  if constexpr (gemv_case_exists(OP, WF, M, EPI, PRO)) {
    if (m == M && pro == PRO && epi == EPI) f = gemv_find_geom<OP, WF, M, PRO, EPI>(g, tail);
  }
}
template <GemvOp OP, int WF, int... I>
static GemvLaunch gemv_find_cases(std::integer_sequence<int, I...>, int M, int pro, int epi, GemvGeom g, bool tail) {
  GemvLaunch f = nullptr;
  (gemv_find_case<OP, WF, I / 14 + 1, I / 7 % 2, I % 7>(M, pro, epi, g, tail, f), ...);
  return f;
}
template <GemvOp OP, int WF>
static GemvLaunch gemv_find(int M, int pro, int epi, GemvGeom g, bool tail) {
  return gemv_find_cases<OP, WF>(std::make_integer_sequence<int, kGemvValuMaxM * 2 * 7>{}, M, pro, epi, g, tail);
}

// gemv_find<op, WF_P12>: the P12 kernels are translation units of their own (gemv_p12.hip, gemv_ar_p12.hip,
// gemv_moe_p12.hip: the pair form and the combine), compiled beside gemv.hip instead of multiplying its
// build time.
GemvLaunch gemv_find_dense_p12(int M, int pro, int epi, GemvGeom g, bool tail);
GemvLaunch gemv_find_ar_p12(int M, int pro, int epi, GemvGeom g, bool tail);
GemvLaunch gemv_find_moe_p12(GemvOp op, int M, int pro, int epi, GemvGeom g);

}  // namespace llmc
