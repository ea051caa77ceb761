// K6 (decode class): skinny GEMM  y[m, n] = sum_k x[m, k] * W[n, k]   for M = 1..4 rows.
//
// Batch-1 decode is HBM-bound weight streaming (8B = 15 GB/token), so this is
// THE hot kernel. Design (cdna_hip_programming.md §5 row "GEMV / M <= 16"; MI355X_MICROARCH
// rows nt-weights, launches-baseline):
//  * W [N, K] bf16, K contiguous. A wave owns RPW output rows; lane l streams chunks
//    c = l + 64 i (16 B = 8 bf16 each) of all RPW rows -> RPW*UNROLL independent 16 B loads in
//    flight per lane, straight to VGPRs (no LDS round trip for W), non-temporal (read once).
//  * Geometry (NT threads, RPW rows/wave) is chosen per shape on the host so the grid is a
//    balanced multiple of the 256 CUs with >= 16 waves/CU in flight (gemv_geom in gemv_geom.h).
//  * x is staged ONCE per block in LDS (M*K bf16); every lane reads the same chunk index it
//    loads from W, so ds_read_b128 addresses are lane-consecutive (conflict-free).
//  * v_dot2_f32_bf16 does convert+multiply+accumulate of 2 elements per VALU op.
//  * Fused prologue  PRO_NORM: x <- bf16(rmsnorm(x) * w_norm)  (the layer's input norm).
//  * Fused epilogues: bf16 store | f32 store (logits) | in-place residual add h += W.x |
//    SiLU-mul over interleaved gate/up rows (row 2i = gate_i, 2i+1 = up_i) |
//    ROPE: qkv projection with pair-interleaved Q/K head rows -> rotate-half RoPE from the f32
//    accumulators, q to the q buffer, k/v straight into the paged KV cache at the device slot
//    (replaces the separate RoPE + KV-write launch of the decode step).
#pragma once
#include <type_traits>

#include "car_proto.h"
#include "common.h"
#include "gemv_geom.h"

namespace llmc {

// PRO_*, EPI_*: gemv_geom.h.
// EPI_AR: a tensor-parallel rank's row-parallel projection (decode o_proj / down_proj) with the
// all-reduce in its own epilogue: h = sum over ranks of (W_r . x_r), rank 0's term carrying the
// residual h. Block b of every rank owns the same rows, so block b only exchanges with block b
// of its peers, over car_proto.h's push protocol (its own buffer, granules [16 b, 16 b + NG) of
// every slot): the block's bf16 partials go straight into every peer's buffer as data-tagged
// granules, and it sums its peers' granules in rank order as they land — the numerics of a
// separate EPI_RESADD / EPI_BF16 GEMV followed by the one-shot all-reduce, bit for bit, without
// that kernel's launch, its boundary and its re-read of h. What holds: every wait is bounded (1 s,
// car_proto.h car_spin; a give-up fails the request on every rank). Forward progress within that
// bound is guaranteed only when each rank owns its GPU and no other engine's blocks can take the
// CUs a peer's blocks need: blocks are dispatched in index order, so on a GPU of its own the lowest
// unfinished block of every rank is resident. Ranks sharing a GPU, or a TP engine beside engines
// that decode at the same time, keep the separate all-reduce launch (comm.py enable_custom,
// placement.fused_ar_allowed). Granules per block: car_proto.h kArGranulesPerBlock.

struct RopeEpi {
  bf16_t* q_out;            // [M, q_stride], canonical head-major layout
  int q_stride;
  bf16_t* k_cache;          // [nb][nkv][bs][D]
  bf16_t* v_cache;
  const int32_t* positions; // [M]
  const int32_t* slots;     // [M]
  const float* cos_t;       // [max_pos][D/2]
  const float* sin_t;
  int nh, nkv, D, bs;
  // optional (qkv_attn.hip): every rotated q / k pair and v pair also published as an 8-B
  // {bf16x2, gtag} granule for the attention blocks of the same launch: q head h pair i at
  // [h][i] = dims (i, i + D/2); k head j at [nh + j][i], same dims; v head j at [nh + nkv + j][d/2]
  // = dims (d, d + 1); D/2 granules per head
  uint64_t* granules;
  uint32_t gtag;
  // optional (Qwen2): the q/k/v projection bias [N] bf16 in W's row order (pair-interleaved like
  // its rows; 4-B aligned), added to the f32 accumulators before the rotation; null = no bias
  const bf16_t* bias;
};

// Weight formats of the VALU GEMV. WF_P13: the lossless 13-bit planes of wpack.hip (layout there)
// beside the bf16 tensor. One wave unit = 4 chunks per lane = kP13UnitElems weights in
// kP13UnitBytes; a row whose header byte is kP13Raw is read from the bf16 tensor instead. The
// decoded chunks enter the same dot8_bf16 chain in the same order as the bf16 loop's, so for the
// same geometry the output bits are the bf16 kernel's.
//
// WF_P12: 12 bits per weight (wpack.hip, the P12 layout): the same units without the sign plane
// (kP12UnitBytes), the sign in the nibble's top bit and a 3-bit exponent code, a window of 16
// exponents. The few weights of a row outside its window are exceptions: the row's record
// (kP12RecDwords dwords: header = base | count << 8, or kP12Raw in the low byte, then kP12MaxExc slots
// value << 16 | k, sorted by k) comes through the scalar cache, and the decoded chunk is patched in
// the register before the dot product, so it is the bf16 chunk again. A row with more exceptions
// than slots is raw.
//
// WF_P12 with a tail (TAIL; wpack.hip, "P12 with a tail"): K a multiple of 512 (one wave chunk: 64
// lanes x 8 weights) off the 2048-weight unit. A row is its K / 2048 >= 1 whole units and then tailq =
// (K / 512) % 4 wave chunks of kP12TailChunkBytes. The tail rides through the packed loop as one more
// unit slot after the last whole one: its two or three loads fill the slot's registers where p12_chunk
// expects chunks 0..tailq-1, it is issued one batch ahead like every unit, and its chunks are patched (q =
// 4 units + c) and summed after the last whole unit's, which is the bf16 loop's order for the lane.
// (WF_*, kP13UnitElems, kP12ChunkElems, kP12MaxK: gemv_geom.h, the host rule needs them.)
constexpr int kP13UnitBytes = 3328, kP13Raw = 0xff;
constexpr int kP12UnitBytes = 3072, kP12Raw = 0xff, kP12MaxExc = 16, kP12RecDwords = 1 + kP12MaxExc;
constexpr int kP12TailChunkBytes = 768;  // a tail chunk: 512 low bytes, 256 nibble bytes
constexpr uint32_t kP12End = 0xffffffffu;
struct PackedW {
  const uint8_t* planes;  // P13 [N][K / 2048][3328] | P12 [N][K / 2048][3072] (+ [(K / 512) % 4][768] per row: the tail)
  const uint8_t* hdr;     // P13 [N] bytes (readable up to the next multiple of 4) | P12 [N][17] dwords
  int wf = WF_BF16;       // host side: which kernel reads it (WF_BF16: no twin, null planes)
};
struct P13Unit {  // one lane's share of a wave unit: 13 dwords for 32 weights
  u32x4 l0, l1, n;
  uint32_t s;
};
// chunk C (0..3) of a lane unit -> its 8 bf16 as the bf16 tensor's 16-B chunk
template <int C>
__device__ __forceinline__ u32x4 p13_chunk(const P13Unit& p, uint32_t base4) {
  const uint32_t n = p.n[C];
  const uint32_t e0 = (n & 0x0f0f0f0fu) + base4, e1 = ((n >> 4) & 0x0f0f0f0fu) + base4;
  const u32x4& L = C < 2 ? p.l0 : p.l1;
  const uint32_t lw0 = L[(2 * C) & 3], lw1 = L[(2 * C + 1) & 3];
  const uint32_t h0 = ((p.s << (7 - 2 * C)) & 0x80808080u) | e0;
  const uint32_t h1 = ((p.s << (6 - 2 * C)) & 0x80808080u) | e1;
  u32x4 w;
  w[0] = __builtin_amdgcn_perm(h0, lw0, 0x05010400u);
  w[1] = __builtin_amdgcn_perm(h0, lw0, 0x07030602u);
  w[2] = __builtin_amdgcn_perm(h1, lw1, 0x05010400u);
  w[3] = __builtin_amdgcn_perm(h1, lw1, 0x07030602u);
  return w;
}

struct P12Unit {  // 12 dwords for 32 weights
  u32x4 l0, l1, n;
};
struct alignas(4) P12TailN3 {  // a lane's three nibble dwords of a three-chunk tail
  uint32_t v[3];
};
template <int C>
__device__ __forceinline__ u32x4 p12_chunk(const P12Unit& p, uint32_t base4) {
  const uint32_t n = p.n[C];
  const uint32_t h0 = ((n & 0x07070707u) + base4) | ((n << 4) & 0x80808080u);
  const uint32_t h1 = (((n >> 4) & 0x07070707u) + base4) | (n & 0x80808080u);
  const u32x4& L = C < 2 ? p.l0 : p.l1;
  const uint32_t lw0 = L[(2 * C) & 3], lw1 = L[(2 * C + 1) & 3];
  u32x4 w;
  w[0] = __builtin_amdgcn_perm(h0, lw0, 0x05010400u);
  w[1] = __builtin_amdgcn_perm(h0, lw0, 0x07030602u);
  w[2] = __builtin_amdgcn_perm(h1, lw1, 0x05010400u);
  w[3] = __builtin_amdgcn_perm(h1, lw1, 0x07030602u);
  return w;
}
// exception entry `ent` (wave-uniform: value << 16 | q << 9 | lane << 3 | element) into the owning
// lane's decoded chunk
__device__ __forceinline__ void p12_patch(u32x4& w, uint32_t ent, int lane) {
  const bool mine = lane == static_cast<int>((ent >> 3) & 63u);
  const uint32_t e = ent & 7u, val = ent >> 16;
  const uint32_t keep = (e & 1u) ? 0x0000ffffu : 0xffff0000u, ins = (e & 1u) ? val << 16 : val;
#pragma unroll
  for (int d = 0; d < 4; ++d)
    if (mine && (e >> 1) == static_cast<uint32_t>(d)) w[d] = (w[d] & keep) | ins;
}

// Batched decode (3 <= M <= 32 rows): the MFMA form in gemv_mfma.hip, same prologue/epilogues
// (one 16-token MFMA column group up to 16 rows, two above). This kernel serves M <= kGemvMaxM
// (and M <= 4 when K is not a multiple of 128). MoE pairs stay within one token group.
constexpr int kGemvmMaxM = 32, kMoeGemvmMaxTokens = 16;  // kGemvMaxM: gemv_geom.h
int gemvm_dispatch(int M, const void* x, int x_stride, const void* norm_w, float eps, const void* W, void* out,
                   int out_stride, int N, int K, int epi, const RopeEpi& rope, hipStream_t st, int form = 0);

// One block of the GEMV (block (bx, by) of its grid; smem = the block's dynamic LDS): the body of
// gemv_kernel, also the projection role of fused launches (qkv_attn.hip).
// DEPTH (packed loop): batches in flight ahead of the one being consumed, 1 or 2. The summation
// order does not depend on it.
// TAIL (WF_P12): K is off the 2048-weight unit and the row ends in (K / 512) % 4 tail chunks.
template <int M, int NT, int RPW, int UNROLL, int PRO, int EPI, bool EXPERT = false, int WF = WF_BF16, int DEPTH = 1,
          bool TAIL = false>
__device__ __forceinline__ void gemv_block(const int bx, const int by, char* smem, const bf16_t* __restrict__ x,
                                           int x_stride, const bf16_t* __restrict__ norm_w, float eps,
                                           const bf16_t* __restrict__ W, void* __restrict__ out, int out_stride, int N,
                                           int K, const int32_t* __restrict__ expert_ids, int x_div, const RopeEpi& rope,
                                           const CarArgs& ar, const PackedW& pw = PackedW{}) {
  constexpr int WAVES = NT / kWave;
  constexpr bool P12 = WF == WF_P12;
  constexpr bool P13 = WF == WF_P13 || P12;  // the packed loop; P12 differs in the unit, the decode and the patch
  using PUnit = std::conditional_t<P12, P12Unit, P13Unit>;
  constexpr int kUnitBytes = P12 ? kP12UnitBytes : kP13UnitBytes;
  static_assert(DEPTH == 1 || (DEPTH == 2 && P13), "prefetch depth: the packed loop, 1 or 2 batches ahead");
  static_assert(!TAIL || (P12 && DEPTH == 1), "a tail: the 12-bit format, one batch ahead");
  static_assert(!P13 || (UNROLL % 4 == 0 && M <= 2), "packed weights: the one- and two-row decode forms");
  // EPI_AR streams the 12-bit planes only (gemv_ar_p12.hip), one row per wave, one batch ahead; no 13-bit form
  static_assert(!P13 || EPI != EPI_AR || (P12 && RPW == 1 && DEPTH == 1), "packed EPI_AR: 12 bits, one batch ahead");
  // MoE experts (pair form and EPI_COMBINE): the 12-bit twin of the [E * N, K] view of the expert stack, whole
  // units only, one unit per batch (the only unroll the MoE launchers use)
  static_assert(!P13 || !EXPERT || (P12 && !TAIL && DEPTH == 1 && UNROLL == 4),
                "packed expert weights: 12 bits, no tail, one unit per batch");
  constexpr bool PAIR_LDS = (EPI == EPI_SILU || EPI == EPI_ROPE) && RPW == 1;  // host: N % (2 * WAVES) == 0
  // RoPE operands through the scalar cache, early (below): one pair per wave (PAIR_LDS: the even
  // wave's row and its partner; RPW == 2: the wave's own two rows)
  constexpr bool ROPE_PRE = EPI == EPI_ROPE && (PAIR_LDS || RPW == 2);
  // EXPERT (MoE decode): by = (token, slot) pair; weights of expert expert_ids[pair],
  // input row pair / x_div, output row pair (M must be 1).
  // EPI_COMBINE (MoE decode down projection fused with the combine; EXPERT, M == RPW == top-k):
  // by = token t; wave row n streams row n of each of the token's k experts ("rows" r =
  // slots), x row r = the slot's activation; acc[r][r] is that expert's output and the epilogue
  // does h[t][n] += sum_r w[t][r] * acc[r][r] in a fixed order (replaces moe_combine's launch and
  // the y round trip). x_div carries nothing here; the router weights come in through `rope.cos_t`.
  constexpr bool COMBINE = EPI == EPI_COMBINE;
  static_assert(!COMBINE || (EXPERT && M == RPW), "combine: one x row per expert slot");
  if constexpr (EXPERT && !COMBINE) {
    const int pair = by;
    if (expert_ids[pair] < 0) return;  // another rank's expert (expert parallel): whole block exits
    W += static_cast<int64_t>(expert_ids[pair]) * N * K;
    x += static_cast<int64_t>(pair / x_div) * x_stride;
    out = reinterpret_cast<char*>(out) + static_cast<int64_t>(pair) * out_stride * (EPI == EPI_F32 ? 4 : 2);
  }
  if constexpr (COMBINE) {
    const int t = by;
    x += static_cast<int64_t>(t) * RPW * x_stride;
    out = reinterpret_cast<char*>(out) + static_cast<int64_t>(t) * out_stride * 2;
  }
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // [M][K]
  const int tid = threadIdx.x;
  const int nchunk = K / 8;
  const int wave = tid / kWave, lane = tid % kWave;
  const int row0 = COMBINE ? bx * WAVES + wave : (bx * WAVES + wave) * RPW;

  // Weight rows (clamped: waves past N still load a valid row and discard it, so no lane
  // diverges before the block barrier). The first UNROLL-batch of W is issued BEFORE the x
  // prologue: W does not depend on x, so the HBM latency of the first batch overlaps the
  // x staging / RMS norm, and the loop keeps the next batch in flight while it computes.
  const u32x4* wrow[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    if constexpr (COMBINE) {
      const int e = expert_ids[by * RPW + r];
      wrow[r] = reinterpret_cast<const u32x4*>(W + (static_cast<int64_t>(e) * N + min(row0, N - 1)) * K);
    } else {
      const int n = min(row0 + r, N - 1);
      wrow[r] = reinterpret_cast<const u32x4*>(W + static_cast<int64_t>(n) * K);
    }
  }
  constexpr int STEP = kWave * UNROLL;
  const int iters = (nchunk + STEP - 1) / STEP;
  u32x4 cur[RPW][UNROLL];
  auto issue = [&](u32x4 (&dst)[RPW][UNROLL], int cbase) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int c = min(cbase + u * kWave, nchunk - 1);  // clamped tail: loads stay batched
#pragma unroll
      for (int r = 0; r < RPW; ++r) dst[r][u] = load16<true>(wrow[r] + c);
    }
  };
  // x (and the norm weights) are loaded BEFORE the first weight batch: vmcnt retires loads in
  // issue order, so the prologue's wait for x then leaves the weight batch in flight, and the main
  // loop issues the second batch while the first is still landing (x last would make the
  // prologue wait for the whole first batch and open a bubble in every wave's stream).
  constexpr bool kXRegs = (PRO == PRO_NORM || PRO == PRO_NONE);
  const bool x_fast = nchunk <= 2 * NT;  // x fits in two 16-B chunks per thread
  u32x4 xr[2][M], gr[2];
  if constexpr (kXRegs) {
    if (x_fast) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = tid + j * NT;
        if (c < nchunk) {
          if constexpr (PRO == PRO_NORM) gr[j] = reinterpret_cast<const u32x4*>(norm_w)[c];
#pragma unroll
          for (int m = 0; m < M; ++m) xr[j][m] = reinterpret_cast<const u32x4*>(x + static_cast<int64_t>(m) * x_stride)[c];
        }
      }
    }
  }
  // WF_P13: UB wave units per batch, one batch ahead like the bf16 loop. Units are wave-wide, so
  // the tail (K is a whole number of units, the last batch maybe not) is masked wave-uniformly.
  constexpr int UB = P13 ? UNROLL / 4 : 1;
  const int units = K / kP13UnitElems;
  const int tailq = TAIL ? (K / kP12ChunkElems) % 4 : 0;  // host: 1..3 under TAIL, and units >= 1
  PUnit cur13[P13 ? RPW : 1][UB];
  PUnit nx13[P13 && DEPTH == 2 ? RPW : 1][UB];  // DEPTH 2: the batch after cur13
  const uint8_t* prow[RPW];
  uint32_t hdr_w[RPW];
  // P12: the row's record, its next exception entry (kP12End: none left) and that entry's index
  const uint32_t* rec12[RPW];
  uint32_t nxt12[RPW], idx12[RPW];
  auto issue13 = [&](PUnit (&dst)[P13 ? RPW : 1][UB], int ubase) {
#pragma unroll
    for (int j = 0; j < UB; ++j) {
      if constexpr (TAIL) {
        if (ubase + j >= units) {  // wave-uniform, as is tailq: the tail's slot (a slot past it loads the tail again and is not read)
#pragma unroll
          for (int r = 0; r < RPW; ++r) {
            const uint8_t* t = prow[r] + static_cast<int64_t>(units) * kUnitBytes;
            // the unit's registers, truncated: low bytes of chunks 0, 1 in l0, of chunk 2 in l1, nibble dword c in
            // n[c], fetched with the widest loads the tail's length allows: 2, 2 and 3 loads for 1, 2, 3 chunks.
            // (Three loads whatever tailq, the 8-B pieces split in two so that the count behind a wait never
            // depends on this branch, measured slower on every shape: profiles/r11_packed_tail.md section 1.)
            P12Unit d{};
            const uint8_t* tn = t + tailq * 512;
            if (tailq == 1) {
              const u32x2 lo = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(t + lane * 8));
              d.l0[0] = lo[0];
              d.l0[1] = lo[1];
              d.n[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(tn + lane * 4));
            } else {
              d.l0 = load16<true>(t + lane * 16);
              if (tailq == 2) {
                const u32x2 nn = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(tn + lane * 8));
                d.n[0] = nn[0];
                d.n[1] = nn[1];
              } else {
                const u32x2 lo = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(t + 1024 + lane * 8));
                d.l1[0] = lo[0];
                d.l1[1] = lo[1];
                const P12TailN3 nn = *reinterpret_cast<const P12TailN3*>(tn + lane * 12);  // 12 B, 4-B aligned
                d.n[0] = nn.v[0];
                d.n[1] = nn.v[1];
                d.n[2] = nn.v[2];
              }
            }
            dst[r][j] = d;
          }
          continue;
        }
      }
      const int u = min(ubase + j, units - 1);  // clamped tail: loads stay batched
#pragma unroll
      for (int r = 0; r < (P13 ? RPW : 1); ++r) {
        const uint8_t* p = prow[r] + static_cast<int64_t>(u) * kUnitBytes + lane * 16;
        dst[r][j].l0 = load16<true>(p);
        dst[r][j].l1 = load16<true>(p + 1024);
        dst[r][j].n = load16<true>(p + 2048);
        // signs: 4 B per lane at unit + 3072 + 4 lane (p already holds 16 lane)
        if constexpr (!P12)
          dst[r][j].s = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p + 3072 - lane * 12));
      }
    }
  };
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (P13) {
    // the row headers through the scalar cache (needed only when the first batch is consumed);
    // the first packed batch goes out whatever they say: a raw row's planes are valid memory
    const int w_u = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n_u = min((bx * WAVES + w_u) * RPW + r, N - 1);
      int64_t row_u = n_u;  // the row of the twin
      if constexpr (EXPERT) {
        // the twin is that of the [E * N, K] view: row n of expert e is its row e * N + n. Pair form: the pair's
        // expert (>= 0: the exit above); combine: slot r streams row n of its own expert, as wrow[r] does
        const int e_u = ld_scalar(expert_ids + (COMBINE ? by * RPW + r : by));
        row_u = static_cast<int64_t>(e_u) * N + (COMBINE ? min(bx * WAVES + w_u, N - 1) : n_u);
      }
      if constexpr (P12) {  // header and first slot together: no dependent load
        rec12[r] = reinterpret_cast<const uint32_t*>(pw.hdr) + row_u * kP12RecDwords;
        hdr_w[r] = ld_scalar(rec12[r]);
        nxt12[r] = ld_scalar(rec12[r] + 1);
      } else {
        hdr_w[r] = ld_scalar(reinterpret_cast<const uint32_t*>(pw.hdr + (n_u & ~3))) >> ((n_u & 3) * 8) & 0xffu;
      }
      prow[r] = pw.planes + row_u * units * kUnitBytes;
      if constexpr (TAIL) prow[r] += row_u * tailq * kP12TailChunkBytes;  // the row stride with a tail
    }
    issue13(cur13, 0);
    if constexpr (DEPTH == 2) {
      if (UB < units) issue13(nx13, UB);  // wave-uniform
    }
  } else {
    issue(cur, lane);
  }
  __builtin_amdgcn_sched_barrier(0);


  // EPI_AR: this block's epoch and (rank 0) the residual of this wave's row, both issued behind the
  // first weight batch (in-order retirement: waiting for them later waits for nothing else)
  uint32_t ar_epoch = 0;
  float ar_resid[M];
  if constexpr (EPI == EPI_AR) {
    static_assert(RPW == 1 && M <= 2 && M * WAVES / 2 <= kArGranulesPerBlock, "EPI_AR geometry");
    if (tid == 0)
      ar_epoch = __hip_atomic_load(car_ctr(ar.P.base[ar.rank]) + bx, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM) + 1;
#pragma unroll
    for (int m = 0; m < M; ++m)
      ar_resid[m] = ar.rank == 0 && row0 < N
                        ? bf16_to_f32(reinterpret_cast<const bf16_t*>(out)[static_cast<int64_t>(m) * out_stride + row0])
                        : 0.f;
  }

  // RoPE epilogue operands (PAIR_LDS: one row per even wave) are wave-uniform, so they come
  // through the SCALAR cache (s_load, counted by lgkmcnt): as vector loads they queued behind the
  // weight stream in the in-order vmcnt counter, and the position -> cos/sin dependency held the
  // second weight batch back by a memory round trip (qkv 11.2 -> ~10.3 us for Llama-3-8B
  // without them). Position and slot are issued here, behind the first weight batch; the
  // dependent cos/sin loads after the prologue, when the position has landed.
  int pre_pos[M], pre_slot[M];
  float pre_c[M], pre_s[M];
  uint32_t pre_b = 0;  // the pair's two biases (bf16x2: rows 2j, 2j + 1)
  if constexpr (ROPE_PRE) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      pre_slot[m] = ld_scalar(rope.slots + m);
      pre_pos[m] = ld_scalar(rope.positions + m);
    }
    if (rope.bias != nullptr) {  // launch-uniform; the pair's row is even (N is even: host)
      const int w_u = __builtin_amdgcn_readfirstlane(wave);
      const int r_u = min(((bx * WAVES + w_u) * RPW) & ~1, N - 2);
      pre_b = ld_scalar(reinterpret_cast<const uint32_t*>(rope.bias + r_u));
    }
  }

  // ---- prologue: x -> LDS (optionally RMS-normalised) ----
  if constexpr (PRO == PRO_NORM) {
    float(*red)[WAVES] = reinterpret_cast<float(*)[WAVES]>(smem + static_cast<size_t>(M) * K * sizeof(bf16_t));
    float ss[M];
#pragma unroll
    for (int m = 0; m < M; ++m) ss[m] = 0.f;
    if (x_fast) {
      // ONE global round trip (issued above): x and the norm weights stay in registers between
      // the sum of squares and the normalisation (K <= 16 Ki at 1024 threads)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (tid + j * NT < nchunk) {
#pragma unroll
          for (int m = 0; m < M; ++m) {
            float f[8];
            unpack8(xr[j][m], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) ss[m] += f[e] * f[e];
          }
        }
      }
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const float sm = wave_sum(ss[m]);
        if ((tid & 63) == 0) red[m][tid / 64] = sm;
      }
      __syncthreads();
      float inv[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += red[m][w];
        inv[m] = rsqrtf(t / K + eps);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = tid + j * NT;
        if (c < nchunk) {
          float g[8];
          unpack8(gr[j], g);
#pragma unroll
          for (int m = 0; m < M; ++m) {
            float f[8];
            unpack8(xr[j][m], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = f[e] * inv[m] * g[e];
            reinterpret_cast<u32x4*>(xs + m * K)[c] = pack8(f);
          }
        }
      }
    } else {  // long rows: two passes over x (L2-resident)
      for (int c = tid; c < nchunk; c += NT) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
          float f[8];
          unpack8(reinterpret_cast<const u32x4*>(x + static_cast<int64_t>(m) * x_stride)[c], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) ss[m] += f[j] * f[j];
        }
      }
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const float sm = wave_sum(ss[m]);
        if ((tid & 63) == 0) red[m][tid / 64] = sm;
      }
      __syncthreads();
      float inv[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += red[m][w];
        inv[m] = rsqrtf(t / K + eps);
      }
      for (int c = tid; c < nchunk; c += NT) {
        float g[8];
        unpack8(reinterpret_cast<const u32x4*>(norm_w)[c], g);
#pragma unroll
        for (int m = 0; m < M; ++m) {
          float f[8];
          unpack8(reinterpret_cast<const u32x4*>(x + static_cast<int64_t>(m) * x_stride)[c], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = f[j] * inv[m] * g[j];
          reinterpret_cast<u32x4*>(xs + m * K)[c] = pack8(f);
        }
      }
    }
  } else if (x_fast) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = tid + j * NT;
      if (c < nchunk) {
#pragma unroll
        for (int m = 0; m < M; ++m) reinterpret_cast<u32x4*>(xs + m * K)[c] = xr[j][m];
      }
    }
  } else {
    for (int c = tid; c < nchunk; c += NT) {
#pragma unroll
      for (int m = 0; m < M; ++m)
        reinterpret_cast<u32x4*>(xs + m * K)[c] =
            reinterpret_cast<const u32x4*>(x + static_cast<int64_t>(m) * x_stride)[c];
    }
  }
  __syncthreads();
  if (!PAIR_LDS && EPI != EPI_AR && row0 >= N) return;  // PAIR_LDS / EPI_AR: every wave reaches the barriers
  if constexpr (ROPE_PRE) {
    const int w_u = __builtin_amdgcn_readfirstlane(wave);
    const int r_u = (bx * WAVES + w_u) * RPW;
    const int D = rope.D, half = D / 2;
    const bool qk = r_u / D < rope.nh + rope.nkv;
    const int i = (r_u % D) / 2;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      pre_c[m] = 1.f;
      pre_s[m] = 0.f;
      if (qk) {
        const int64_t t = static_cast<int64_t>(pre_pos[m]) * half + i;
        pre_c[m] = ld_scalar(rope.cos_t + t);
        pre_s[m] = ld_scalar(rope.sin_t + t);
      }
    }
  }

  // ---- main loop: RPW weight rows per wave, one UNROLL-batch ahead ----
  float acc[RPW][M];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < M; ++m) acc[r][m] = 0.f;

  const u32x4* xv = reinterpret_cast<const u32x4*>(xs);
  // MASKED only for the last batch when K is not a multiple of 64 * 8 * UNROLL elements: the
  // full batches run branch-free (no per-chunk exec-mask juggling between the waits)
  auto consume = [&](const u32x4 (&wv)[RPW][UNROLL], int cbase, auto masked) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int c = cbase + u * kWave;
      if (!decltype(masked)::value || c < nchunk) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const u32x4 xx = xv[m * nchunk + c];
#pragma unroll
          for (int r = 0; r < RPW; ++r)
            if (!COMBINE || r == m) acc[r][m] = dot8_bf16(wv[r][u], xx, acc[r][m]);
        }
      }
    }
  };
  using Full = std::integral_constant<bool, false>;
  using Masked = std::integral_constant<bool, true>;
  auto stream_bf16 = [&]() {
    const int full = nchunk / STEP;  // batches in which every lane's chunks are all in range
    int c0 = lane;
    for (int it = 0; it + 1 < iters; ++it, c0 += STEP) {  // it < iters - 1 <= full
      u32x4 nxt[RPW][UNROLL];
      issue(nxt, c0 + STEP);
      consume(cur, c0, Full{});
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
#pragma unroll
        for (int r = 0; r < RPW; ++r) cur[r][u] = nxt[r][u];
    }
    if (full == iters) {
      consume(cur, c0, Full{});
    } else {
      consume(cur, c0, Masked{});
    }
  };
  if constexpr (P13) {
    bool raw = false;
    uint32_t base4[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      raw |= (hdr_w[r] & 0xffu) == kP13Raw;  // kP12Raw is the same byte
      base4[r] = (hdr_w[r] & 0xffu) * 0x01010101u;
      if constexpr (P12) {
        idx12[r] = 0;
        if ((hdr_w[r] >> 8 & 0xffu) == 0) nxt12[r] = kP12End;  // slot 0 of an empty list is zero, not an entry
      }
    }
    if (raw) {  // wave-uniform: a raw row (or its RPW partner) streams the bf16 tensor
      issue(cur, lane);
      stream_bf16();
    } else {
      // chunk c of unit u is the bf16 loop's chunk lane + 64 (4 u + c): same x chunk, same order
      // masked: the row's last batch. Its slots past the last whole unit are skipped, but for the tail's
      // slot (TAIL: slot `units`), of which chunks 0..tailq-1 are summed; all of it is wave-uniform
      auto consume13 = [&](const PUnit (&wv)[RPW][UB], int ubase, auto masked) {
#pragma unroll
        for (int j = 0; j < UB; ++j) {
          const bool part = TAIL && decltype(masked)::value && ubase + j == units;
          if (!decltype(masked)::value || ubase + j < units || part) {
            const int live = part ? tailq : 4;  // the slot's chunks
            const int cb = lane + kWave * 4 * (ubase + j);
            auto chunk = [&](auto cc) {
              constexpr int C = decltype(cc)::value;
              if (TAIL && decltype(masked)::value && C >= live) return;
              u32x4 w[RPW];
#pragma unroll
              for (int r = 0; r < RPW; ++r) {
                if constexpr (P12) {
                  w[r] = p12_chunk<C>(wv[r][j], base4[r]);
                  // wave-uniform and rare: entries of this wave chunk (q = k / 512), in k order
                  const uint32_t q = 4u * static_cast<uint32_t>(ubase + j) + C;
                  while ((nxt12[r] >> 9 & 0x7fu) == q) {
                    p12_patch(w[r], nxt12[r], lane);
                    ++idx12[r];
                    const uint32_t e = ld_scalar(rec12[r] + 1 + min(idx12[r], static_cast<uint32_t>(kP12MaxExc - 1)));
                    nxt12[r] = idx12[r] < (hdr_w[r] >> 8 & 0xffu) ? e : kP12End;
                  }
                } else {
                  w[r] = p13_chunk<C>(wv[r][j], base4[r]);
                }
              }
#pragma unroll
              for (int m = 0; m < M; ++m) {
                const u32x4 xx = xv[m * nchunk + cb + C * kWave];
#pragma unroll
                for (int r = 0; r < RPW; ++r)
                  if (!COMBINE || r == m) acc[r][m] = dot8_bf16(w[r], xx, acc[r][m]);
              }
            };
            chunk(std::integral_constant<int, 0>{});
            chunk(std::integral_constant<int, 1>{});
            chunk(std::integral_constant<int, 2>{});
            chunk(std::integral_constant<int, 3>{});
          }
        }
      };
      const int it13 = (units + (TAIL ? 1 : 0) + UB - 1) / UB;  // TAIL: the tail is one more slot
      int u0 = 0;
      for (int it = 0; it + 1 < it13; ++it, u0 += UB) {
        PUnit nxt[RPW][UB];
        if constexpr (DEPTH == 2) {
          // two batches ahead; past the row's end nothing is issued (a clamped batch would be bytes
          // streamed for nothing) and nx13 is not read again
          const bool more = u0 + 2 * UB < units;  // wave-uniform
          if (more) issue13(nxt, u0 + 2 * UB);
          consume13(cur13, u0, Full{});
#pragma unroll
          for (int j = 0; j < UB; ++j)
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
              cur13[r][j] = nx13[r][j];
              if (more) nx13[r][j] = nxt[r][j];
            }
        } else {
          issue13(nxt, u0 + UB);
          consume13(cur13, u0, Full{});
#pragma unroll
          for (int j = 0; j < UB; ++j)
#pragma unroll
            for (int r = 0; r < RPW; ++r) cur13[r][j] = nxt[r][j];
        }
      }
      if (!TAIL && units % UB == 0) {
        consume13(cur13, u0, Full{});
      } else {
        consume13(cur13, u0, Masked{});
      }
    }
  } else {
    stream_bf16();
  }

#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < M; ++m)
      if (!COMBINE || r == m) acc[r][m] = wave_sum(acc[r][m]);

  // ---- epilogue ----
  // paired epilogues (SiLU, RoPE) combine rows (2j, 2j + 1): the same wave holds both when
  // RPW >= 2; with RPW == 1 they sit in waves (w, w + 1) and meet through LDS (PAIR_LDS).
  // RoPE operands of (row n, token m): cos/sin of the pair's frequency and the KV slot
  auto rope_ops = [&](int n, int m, float& c, float& sn, int& slot, uint32_t& b2) {
    const int D = rope.D, half = D / 2;
    slot = rope.slots[m];
    b2 = rope.bias != nullptr ? *reinterpret_cast<const uint32_t*>(rope.bias + n) : 0u;
    c = 1.f;
    sn = 0.f;
    if (n / D < rope.nh + rope.nkv) {
      const int i = (n % D) / 2;
      const int pos = rope.positions[m];
      c = rope.cos_t[static_cast<int64_t>(pos) * half + i];
      sn = rope.sin_t[static_cast<int64_t>(pos) * half + i];
    }
  };
  // b2: the biases of rows (n, n + 1) (EPI_ROPE with a bias only)
  auto pair_epi = [&](int n, int m, float v, float x2, float c, float sn, int slot, uint32_t b2) {
    if constexpr (EPI == EPI_ROPE) {
      if (rope.bias != nullptr) {  // launch-uniform: a launch without a bias runs the arithmetic it always ran
        v += bf16_lo(b2);
        x2 += bf16_hi(b2);
      }
    }
    if constexpr (EPI == EPI_SILU) {  // rows (2j, 2j+1) = (gate, up) -> output column n/2
      reinterpret_cast<bf16_t*>(out)[static_cast<int64_t>(m) * out_stride + n / 2] = f32_to_bf16(silu(v) * x2);
    } else if constexpr (EPI == EPI_ROPE) {  // rows (2j, 2j+1) of a Q/K head = dims (i, i + D/2)
      const int D = rope.D, half = D / 2;
      const int head = n / D;
      const int64_t page = slot >= 0 ? slot / rope.bs : 0;
      const int off = slot >= 0 ? slot % rope.bs : 0;
      if (head < rope.nh + rope.nkv) {
        const int i = (n % D) / 2;
        const float o1 = v * c - x2 * sn, o2 = x2 * c + v * sn;
        if (head < rope.nh) {
          bf16_t* qo = rope.q_out + static_cast<int64_t>(m) * rope.q_stride + head * D;
          qo[i] = f32_to_bf16(o1);
          qo[i + half] = f32_to_bf16(o2);
        } else if (slot >= 0) {
          bf16_t* ko = rope.k_cache + ((page * rope.nkv + (head - rope.nh)) * rope.bs + off) * D;
          ko[i] = f32_to_bf16(o1);
          ko[i + half] = f32_to_bf16(o2);
        }
        if (rope.granules != nullptr)  // one row (M == 1): rows are heads x D
          __hip_atomic_store(rope.granules + head * half + i,
                             static_cast<uint64_t>(pack_bf16x2(o1, o2)) | (static_cast<uint64_t>(rope.gtag) << 32),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {  // V rows keep canonical order
        const int vh = head - rope.nh - rope.nkv, d = n % D;
        if (slot >= 0) {
          bf16_t* vv = rope.v_cache + ((page * rope.nkv + vh) * rope.bs + off) * D;
          vv[d] = f32_to_bf16(v);
          vv[d + 1] = f32_to_bf16(x2);
        }
        if (rope.granules != nullptr)
          __hip_atomic_store(rope.granules + head * half + d / 2,
                             static_cast<uint64_t>(pack_bf16x2(v, x2)) | (static_cast<uint64_t>(rope.gtag) << 32),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  };
  if constexpr (PAIR_LDS) {
    float* pairx = reinterpret_cast<float*>(smem + static_cast<size_t>(M) * K * sizeof(bf16_t)) + M * WAVES;
    if ((wave & 1) && lane < M) {
#pragma unroll
      for (int m = 0; m < M; ++m)
        if (lane == m) pairx[(wave >> 1) * M + m] = acc[0][m];
    }
    __syncthreads();
    if (!(wave & 1)) {
#pragma unroll
      for (int m = 0; m < M; ++m)
        if (lane == m && row0 < N) {
          if constexpr (EPI == EPI_ROPE) {
            pair_epi(row0, m, acc[0][m], pairx[(wave >> 1) * M + m], pre_c[m], pre_s[m], pre_slot[m], pre_b);
          } else {
            pair_epi(row0, m, acc[0][m], pairx[(wave >> 1) * M + m], 1.f, 0.f, -1, 0u);
          }
        }
    }
    return;
  }
  if constexpr (EPI == EPI_AR) {
    constexpr int HP = WAVES / 2, NG = M * HP;  // row pairs per block; granules per rank
    // the block's values (rank 0: + residual), [M][WAVES] f32 after the norm-partials area
    float* rowv = reinterpret_cast<float*>(smem + static_cast<size_t>(M) * K * sizeof(bf16_t)) + M * WAVES;
#pragma unroll
    for (int m = 0; m < M; ++m)
      if (lane == m) rowv[m * WAVES + wave] = acc[0][m] + ar_resid[m];
    __syncthreads();
    if (wave != 0) return;
    const uint32_t epoch = __shfl(ar_epoch, 0, 64);
    const int rb = bx * WAVES;
    const int pairs = max(0, min(WAVES, N - rb)) / 2;  // N even: a pair is whole or absent
    const long gbase = static_cast<long>(bx) * kArGranulesPerBlock;
    auto payload = [&](int gi) {  // my bf16 pair of granule gi (rows 2j, 2j + 1 of token m)
      const int m = gi / HP, j = gi % HP;
      return pack_bf16x2(rowv[m * WAVES + 2 * j], rowv[m * WAVES + 2 * j + 1]);
    };
    for (int idx = lane; idx < ar.world * NG; idx += kWave) {  // push: (peer, granule)
      const int p = idx / NG, gi = idx % NG;
      if (p != ar.rank && gi % HP < pairs)
        car_put(ar.P.base[p] + car_granule_off(epoch, ar.cap, ar.rank, gbase + gi), payload(gi), epoch);
    }
    if (lane < NG && lane % HP < pairs) {  // collect my granule of every peer, sum in rank order
      const long g[1] = {gbase + lane};
      uint32_t in[kMaxRanks][1];
      car_collect<1>(ar.P, ar.rank, ar.world, ar.cap, epoch, g, in);
      in[ar.rank][0] = payload(lane);
      float lo = 0.f, hi = 0.f;
#pragma unroll
      for (int r = 0; r < kMaxRanks; ++r) {
        if (r < ar.world) {
          lo += bf16_lo(in[r][0]);
          hi += bf16_hi(in[r][0]);
        }
      }
      const int m = lane / HP, j = lane % HP;
      *reinterpret_cast<uint32_t*>(reinterpret_cast<bf16_t*>(out) + static_cast<int64_t>(m) * out_stride + rb + 2 * j) =
          pack_bf16x2(lo, hi);
    }
    if (lane == 0)
      __hip_atomic_store(car_ctr(ar.P.base[ar.rank]) + bx, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  if constexpr (COMBINE) {
    if (lane == 0 && row0 < N) {
      const float* wt = rope.cos_t + by * RPW;  // router weights [T, k]
      bf16_t* h = reinterpret_cast<bf16_t*>(out) + row0;
      float v = bf16_to_f32(*h);
#pragma unroll
      for (int r = 0; r < RPW; ++r) v += wt[r] * acc[r][r];
      *h = f32_to_bf16(v);
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int n = row0 + r;
      if (lane != r * M + m || n >= N) continue;
      const float v = acc[r][m];
      if constexpr (EPI == EPI_BF16) {
        reinterpret_cast<bf16_t*>(out)[static_cast<int64_t>(m) * out_stride + n] = f32_to_bf16(v);
      } else if constexpr (EPI == EPI_F32) {
        reinterpret_cast<float*>(out)[static_cast<int64_t>(m) * out_stride + n] = v;
      } else if constexpr (EPI == EPI_RESADD) {
        bf16_t* h = reinterpret_cast<bf16_t*>(out) + static_cast<int64_t>(m) * out_stride + n;
        *h = f32_to_bf16(bf16_to_f32(*h) + v);
      } else {
        if constexpr (RPW >= 2) {
          if ((r & 1) == 0) {
            float c = 1.f, sn = 0.f;
            int slot = -1;
            uint32_t b2 = 0;
            if constexpr (EPI == EPI_ROPE && RPW == 2) {  // r == 0: the wave's pair, preloaded
              c = pre_c[m];
              sn = pre_s[m];
              slot = pre_slot[m];
              b2 = pre_b;
            } else if constexpr (EPI == EPI_ROPE) {
              rope_ops(n, m, c, sn, slot, b2);
            }
            pair_epi(n, m, v, acc[r + 1][m], c, sn, slot, b2);
          }
        }
      }
    }
  }
}

template <int M, int NT, int RPW, int UNROLL, int PRO, int EPI, bool EXPERT = false>
__global__ __launch_bounds__(NT) void gemv_kernel(const bf16_t* __restrict__ x, int x_stride,
                                                  const bf16_t* __restrict__ norm_w, float eps,
                                                  const bf16_t* __restrict__ W, void* __restrict__ out,
                                                  int out_stride, int N, int K, const int32_t* __restrict__ expert_ids,
                                                  int x_div, RopeEpi rope, CarArgs ar) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_block<M, NT, RPW, UNROLL, PRO, EPI, EXPERT>(blockIdx.x, blockIdx.y, smem, x, x_stride, norm_w, eps, W, out,
                                                   out_stride, N, K, expert_ids, x_div, rope, ar);
}


// WF_P13 form of gemv_kernel (dense, M <= 2): W stays the bf16 tensor (raw rows), pw its planes
template <int M, int NT, int RPW, int UNROLL, int PRO, int EPI>
__global__ __launch_bounds__(NT) void gemv_p13_kernel(const bf16_t* __restrict__ x, int x_stride,
                                                      const bf16_t* __restrict__ norm_w, float eps,
                                                      const bf16_t* __restrict__ W, PackedW pw,
                                                      void* __restrict__ out, int out_stride, int N, int K,
                                                      RopeEpi rope) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_block<M, NT, RPW, UNROLL, PRO, EPI, false, WF_P13>(blockIdx.x, blockIdx.y, smem, x, x_stride, norm_w, eps, W,
                                                          out, out_stride, N, K, nullptr, 1, rope, CarArgs{}, pw);
}


// WF_P12 form (as gemv_p13_kernel; pw.hdr: the rows' records); TAIL: for K off the 2048-weight unit
template <int M, int NT, int RPW, int UNROLL, int PRO, int EPI, int DEPTH = 1, bool TAIL = false>
__global__ __launch_bounds__(NT) void gemv_p12_kernel(const bf16_t* __restrict__ x, int x_stride,
                                                      const bf16_t* __restrict__ norm_w, float eps,
                                                      const bf16_t* __restrict__ W, PackedW pw,
                                                      void* __restrict__ out, int out_stride, int N, int K,
                                                      RopeEpi rope) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_block<M, NT, RPW, UNROLL, PRO, EPI, false, WF_P12, DEPTH, TAIL>(blockIdx.x, blockIdx.y, smem, x, x_stride, norm_w, eps, W,
                                                          out, out_stride, N, K, nullptr, 1, rope, CarArgs{}, pw);
}

// WF_P12 form of the row-parallel GEMV with the all-reduce in its epilogue (EPI_AR)
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

// WF_P12 form of the MoE decode GEMVs, pw the twin of the [E * N, K] view of the expert stack W, so row n of
// expert e is row e * N + n of the twin. M = 1: the pair form (by = (token, slot) pair); M = 2 with
// EPI_COMBINE: by = token, RPW = M = top-k
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

}  // namespace llmc
