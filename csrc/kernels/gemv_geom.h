// The geometry rule of the decode GEMV (kernel body: gemv_core.h), as plain host code: which block
// (NT threads, RPW rows per wave, UNROLL 16-B loads per lane in flight) a launch (op, M, N, K, epilogue)
// runs, in every weight format, and the one list per op of the geometries that are instantiated. No HIP
// in here: llmc_gemv_plan answers from it without a GPU (tests/test_gemv_geometry_cpu.py).
//
// The bit-identity rule: a packed launch runs the blocks of the bf16 launch of the same (M, N, K,
// epilogue), so (nt, rpw) are the same by construction below; only `unroll` may differ (the three
// demotions of p12_runs_4_loads), and a lane sums its chunks in k order whatever the batch.
//
// Geometry (cold-weight sweep on MI355X, scripts/microbench_kernels.py sweep,
// profiles/r1_gemv_geometry_sweep.md): fat blocks (8-16 waves), one row per wave, 4 x 16 B loads
// per lane in flight (+ the next batch prefetched) were fastest on every Llama-3-8B shape: x is
// staged/normalised once per 8-16 rows, and 12-16 waves per CU keep streaming. The waves per
// block are picked so the grid fills whole rounds of the 256 CUs (pick_waves). Paired epilogues
// (SiLU gate/up, RoPE) meet their partner row of the next wave through LDS (PAIR_LDS); shapes
// that do not tile keep 256 threads x 2 rows/wave.
#pragma once
#include <cstdlib>
#include <initializer_list>

namespace llmc {

enum { PRO_NONE = 0, PRO_NORM = 1 };
enum { EPI_BF16 = 0, EPI_F32 = 1, EPI_RESADD = 2, EPI_SILU = 3, EPI_ROPE = 4, EPI_COMBINE = 5, EPI_AR = 6 };
enum { WF_BF16 = 0, WF_P13 = 1, WF_P12 = 2 };  // weight formats: gemv_core.h
constexpr int kP13UnitElems = 2048, kP12ChunkElems = 512;
constexpr int kP12MaxK = 65536 - kP13UnitElems;  // positions are 16 bits, and q = 127 marks the list's end
// The VALU GEMV serves M <= kGemvMaxM rows (and M <= 4 when K is off the MFMA form's 128-k tiles,
// gemv_mfma.hip); packed weights: the one- and two-row forms only.
constexpr int kGemvMaxM = 2, kGemvValuMaxM = 4;

struct GemvGeom {
  int nt, rpw, unroll;  // nt == 0: no such launch
};
constexpr bool operator==(const GemvGeom& a, const GemvGeom& b) {
  return a.nt == b.nt && a.rpw == b.rpw && a.unroll == b.unroll;
}
enum GemvOp { GEMV_DENSE = 0, GEMV_AR = 1, GEMV_MOE_PAIR = 2, GEMV_MOE_COMBINE = 3 };
// M: the rows of x a block multiplies. DENSE 1..4, AR 1..2; the MoE ops whatever the caller's count: a
// pair block has one row, a combine block the token's two expert slots.
constexpr int gemv_block_rows(GemvOp op, int M) { return op == GEMV_MOE_PAIR ? 1 : op == GEMV_MOE_COMBINE ? 2 : M; }

// Whether (op, weight format, M rows per block, epilogue, prologue) has a launch at all, whatever N and K.
// Packed weights: the one- and two-row forms only; P13 the dense op only; MoE pair the SiLU epilogue with
// or without the norm prologue, the bf16 epilogue without it.
constexpr bool gemv_case_exists(GemvOp op, int wf, int M, int epi, int pro) {
  if (wf < WF_BF16 || wf > WF_P12 || (pro != PRO_NONE && pro != PRO_NORM) || M != gemv_block_rows(op, M)) return false;
  switch (op) {
    case GEMV_DENSE:
      return M >= 1 && M <= (wf == WF_BF16 ? kGemvValuMaxM : kGemvMaxM) &&
             (epi == EPI_ROPE ? pro == PRO_NORM : epi >= EPI_BF16 && epi <= EPI_SILU);
    case GEMV_AR: return M >= 1 && M <= kGemvMaxM && epi == EPI_AR && pro == PRO_NONE && wf != WF_P13;
    case GEMV_MOE_PAIR:
      return wf != WF_P13 && (epi == EPI_SILU || (epi == EPI_BF16 && (wf == WF_BF16 || pro == PRO_NONE)));
    default: return epi == EPI_COMBINE && pro == PRO_NONE && wf != WF_P13;
  }
}

// ---- the instantiated geometries: one list per op, expanded by every format's kernels ----
// X(nt, rpw, unroll, max_m, epis): rows up to max_m, epilogues `epis` (gemv_geom_serves). Whatever
// gemv_geom returns is in its op's list, and nothing else is (tests/test_gemv_geometry_cpu.py sweeps it).
enum { GEOM_ANY, GEOM_PAIRED, GEOM_SILU, GEOM_ROPE };
constexpr bool gemv_geom_serves(int epis, int epi) {
  return epis == GEOM_ANY || (epis == GEOM_PAIRED && (epi == EPI_SILU || epi == EPI_ROPE)) ||
         (epis == GEOM_SILU && epi == EPI_SILU) || (epis == GEOM_ROPE && epi == EPI_ROPE);
}
#define LLMC_GEMV_DENSE_GEOMS(X)                                                                     \
  X(1024, 1, 4, 4, GEOM_ANY) X(896, 1, 4, 4, GEOM_PAIRED) X(768, 1, 4, 4, GEOM_ANY)                  \
  X(640, 1, 4, 4, GEOM_ANY) X(512, 1, 4, 4, GEOM_ANY) X(256, 1, 8, 4, GEOM_ANY)                      \
  X(256, 2, 4, 4, GEOM_PAIRED) X(1024, 2, 4, 2, GEOM_SILU) X(896, 2, 4, 2, GEOM_SILU)                \
  X(768, 2, 4, 2, GEOM_ROPE) X(1024, 1, 8, 2, GEOM_ANY) X(640, 1, 8, 2, GEOM_ANY)
#define LLMC_GEMV_AR_GEOMS(X)                                                                        \
  X(1024, 1, 4, 2, GEOM_ANY) X(768, 1, 4, 2, GEOM_ANY) X(640, 1, 4, 2, GEOM_ANY)                     \
  X(512, 1, 4, 2, GEOM_ANY) X(256, 1, 8, 2, GEOM_ANY) X(1024, 1, 8, 2, GEOM_ANY) X(640, 1, 8, 2, GEOM_ANY)
#define LLMC_GEMV_MOE_GEOMS(X)                                                                       \
  X(1024, 1, 4, 1, GEOM_ANY) X(768, 1, 4, 1, GEOM_ANY) X(640, 1, 4, 1, GEOM_ANY)                     \
  X(512, 1, 4, 1, GEOM_ANY) X(256, 1, 4, 1, GEOM_ANY) X(1024, 2, 4, 1, GEOM_SILU)                    \
  X(896, 2, 4, 1, GEOM_SILU) X(896, 1, 4, 1, GEOM_SILU) X(256, 2, 4, 1, GEOM_SILU)
// MoE decode down projection fused with the top-2 combine: one block per 16 output rows per token, each
// wave streaming its row of both experts. (Measured against 512 threads x 4 / 1024 x 2 / 512 x 8 loads
// per lane: none faster, profiles/r6_decode_experiments.md.)
#define LLMC_GEMV_COMBINE_GEOMS(X) X(1024, 2, 4, 2, GEOM_ANY)
// llmc_gemv_sweep's variants (microbenchmarks only): X(variant, nt, rpw, unroll)
#define LLMC_GEMV_SWEEP_GEOMS(X)                                                                     \
  X(0, 256, 1, 8) X(1, 256, 2, 4) X(2, 256, 4, 4) X(3, 512, 1, 8) X(4, 512, 2, 4) X(5, 128, 1, 8)    \
  X(6, 64, 1, 8) X(7, 1024, 1, 4) X(8, 256, 1, 4) X(9, 256, 2, 8) X(10, 512, 4, 2) X(11, 128, 2, 4)  \
  X(12, 1024, 1, 8) X(13, 1024, 2, 4) X(14, 1024, 2, 2) X(15, 1024, 1, 2) X(16, 768, 1, 4)           \
  X(17, 1024, 4, 2) X(18, 1024, 1, 6) X(19, 768, 2, 4) X(20, 640, 1, 8) X(21, 896, 1, 4)             \
  X(22, 768, 2, 2) X(23, 1024, 2, 2)

// The A/B environment switches (scripts/gpu/ab_*.sh), each read once per process.
struct GemvSwitches {
  bool no_w10, no_w14, rope_rpw1, silu_rpw1;
};
inline const GemvSwitches& gemv_switches() {
  static const GemvSwitches sw{std::getenv("LLMC_GEMV_NO_W10") != nullptr, std::getenv("LLMC_GEMV_NO_W14") != nullptr,
                               std::getenv("LLMC_GEMV_ROPE_RPW1") != nullptr,
                               std::getenv("LLMC_GEMV_SILU_RPW1") != nullptr};
  return sw;
}

// Waves per block so that the grid fills whole rounds of the 256 CUs (a 6144-row qkv at 16
// rows/block = 384 blocks leaves half the CUs with twice the work; 12 rows/block = 512 blocks
// is exact): the smallest idle fraction of the last round, ties to the larger block. 0: paired rows
// that no block tiles.
inline int pick_waves(int N, bool paired) {
  // short outputs (a TP rank's qkv: 768 / 1536 rows) cannot fill the chip with fat blocks: 4-wave
  // blocks with 8 loads per lane spread them over 3-6x the CUs (768x4096: 4.04 vs 5.68 us,
  // profiles/r1_attn_decode_tp_shapes.md)
  if (N < 2048 && (!paired || N % 8 == 0)) return 4;
  // 10-wave blocks: a 70B TP=4 rank's qkv (2560 rows) is 256 blocks of 10 rows instead of 160 of 16
  // (96 CUs idle)
  // 14-wave blocks (paired outputs): a TP=8 / TP=4 rank's gate_up (3584 / 7168 rows) is 256 / 512
  // blocks instead of 224 / 448
  const GemvSwitches& sw = gemv_switches();
  int best = 16;
  double best_idle = 2.0;
  for (int w : {16, 14, 12, 10, 8}) {
    if ((w == 10 && sw.no_w10) || (w == 14 && (sw.no_w14 || !paired))) continue;
    if (paired && N % (2 * w) != 0) continue;
    const long blocks = (N + w - 1) / w;
    const long slots = (blocks + 255) / 256 * 256;
    const double idle = static_cast<double>(slots - blocks) / static_cast<double>(slots);
    if (idle < best_idle - 1e-9) {
      best_idle = idle;
      best = w;
    }
  }
  return best_idle > 1.0 ? 0 : best;
}

// The bf16 launch of (op, M, N, K, epi).
inline GemvGeom gemv_geom(GemvOp op, int M, int N, int K, int epi) {
  const bool moe = op == GEMV_MOE_PAIR || op == GEMV_MOE_COMBINE;
  const bool paired = epi == EPI_SILU || epi == EPI_ROPE;
  M = gemv_block_rows(op, M);
  if (!gemv_case_exists(op, WF_BF16, M, epi, PRO_NONE) && !gemv_case_exists(op, WF_BF16, M, epi, PRO_NORM)) return {};
  if (N < 1 || K < 8 || K % 8 != 0 || (!moe && (paired || op == GEMV_AR) && N % 2 != 0)) return {};
  if (op == GEMV_MOE_COMBINE) return {1024, 2, 4};
  const GemvSwitches& sw = gemv_switches();
  // the MoE pair form follows the dense rule; the grid's y dimension (token, expert) pairs multiplies the
  // rounds, so whole rounds per pair are whole rounds overall
  const int w = pick_waves(N, paired);
  if (moe || M <= 2) {
    // the RoPE epilogue with both rows of a pair in one wave (no LDS pair exchange behind a block
    // barrier) where that still fills whole rounds: Llama-3-8B / Mixtral qkv (6144 rows) as 256
    // blocks of 12 waves x 2 rows
    if (epi == EPI_ROPE && w == 12 && N % (2 * 12 * 256) == 0 && !sw.rope_rpw1) return {768, 2, 4};
    // ... and the SiLU gate/up pairs, at the widest block that still fills whole rounds with two rows
    // per wave (8B gate_up and Mixtral's expert gate_up, 28672 rows: 14 waves, 1024 blocks; Phi-3 16384:
    // 16 waves, 512)
    if (epi == EPI_SILU && !sw.silu_rpw1 && K < 8192) {
      if (N % (2 * 16 * 256) == 0) return {1024, 2, 4};
      if (N % (2 * 14 * 256) == 0) return {896, 2, 4};
    }
    // long rows on few blocks (a 70B TP=4 rank's qkv: 2560 x 8192 = 160 fat blocks): 8 loads per
    // lane in flight instead of 4 (9.67 vs 10.99 us, profiles/r1_attn_decode_tp_shapes.md). One or
    // two rows only: with 3-4 rows (the VALU form runs them only when K is off the MFMA form's 128-k
    // tiles) that geometry kept 20-48 B per lane in scratch (tests/test_kernel_plan_cpu.py). Not the MoE
    // pair form: its kernels run 4 loads per lane at every block size
    if (!moe && w == 16 && K >= 8192 && N <= 4096) return {1024, 1, 8};
    if (!moe && w == 10 && K >= 8192) return {640, 1, 8};
  }
  if (w == 0) return {256, 2, 4};  // paired rows that do not tile by 16-32 rows: pairs inside one wave
  // 4-wave blocks run 8 loads per lane at every row count (pick_waves); the MoE pair form's run 4
  return {w * 64, 1, w == 4 && !moe ? 8 : 4};
}

// K of a packed twin (wpack.hip): P13 whole 2048-weight units; P12 whole units, or a multiple of 512 from
// 2048 up, the planes then with the row tail ("P12 with a tail"); expert stacks whole units only.
constexpr bool gemv_packed_k_ok(GemvOp op, int wf, int K) {
  const bool moe = op == GEMV_MOE_PAIR || op == GEMV_MOE_COMBINE;
  if (wf == WF_P13 || moe) return K % kP13UnitElems == 0 && (wf == WF_P13 || K <= kP12MaxK);
  return K % kP12ChunkElems == 0 && K >= kP13UnitElems && K <= kP12MaxK;
}

// Two rows on 16 waves with one row per wave run 4 loads per lane where 8 kept per-lane state in scratch
// (128 VGPRs are that block's limit): one unit per batch there. A lane sums its chunks in k order
// whatever the batch, so the bits stay.
//  * P12 with the RoPE epilogue: 20 B per lane
//  * P12 with a tail, under every epilogue: 36 B per lane (profiles/r11_packed_tail.md)
//  * packed EPI_AR, tail or not (profiles/r13_packed_tp.md)
// The kernels left out are not instantiated (the lists' expansions ask this too).
constexpr bool p12_runs_4_loads(int M, GemvGeom g, int epi, bool tail) {
  return M == 2 && g == GemvGeom{1024, 1, 8} && (epi == EPI_ROPE || epi == EPI_AR || tail);
}

// What the launch of (op, M, N, K, epi, pro) runs in weight format wf: the bf16 launch's blocks. nt == 0
// where the format has no kernel at all (gemv_case_exists) or K is off the format's (gemv_packed_k_ok).
// This is the geometry that runs: no launcher adjusts it.
inline GemvGeom gemv_geom(GemvOp op, int M, int N, int K, int epi, int wf, int pro) {
  M = gemv_block_rows(op, M);
  GemvGeom g = gemv_case_exists(op, wf, M, epi, pro) ? gemv_geom(op, M, N, K, epi) : GemvGeom{};
  if (wf == WF_BF16 || g.nt == 0) return g;
  if (!gemv_packed_k_ok(op, wf, K)) return {};
  if (wf == WF_P12 && p12_runs_4_loads(M, g, epi, K % kP13UnitElems != 0)) g.unroll = 4;
  return g;
}

}  // namespace llmc
