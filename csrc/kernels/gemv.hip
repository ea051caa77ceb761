// The launch entries of the decode GEMV, and its bf16 and WF_P13 kernels (kernel body: gemv_core.h;
// geometry rule and the lists of instantiated geometries: gemv_geom.h; launcher and lookup: gemv_launch.h).
// A packed launch asks the rule of its bf16 launch, so it runs the same blocks and summation order, hence
// gives the same bits, as the bf16 launch of the same (M, N, K, epilogue).
#include <cstdint>

#include "gemv_launch.h"

namespace llmc {

// The launcher of geometry g for (op, weight format, case), or null: every launch below and llmc_gemv_plan
// ask this one lookup.
static GemvLaunch gemv_find_any(GemvOp op, int wf, int M, int pro, int epi, GemvGeom g, int K) {
  M = gemv_block_rows(op, M);
  if (wf == WF_P12) {
    const bool tail = K % kP13UnitElems != 0;
    if (op == GEMV_DENSE) return gemv_find_dense_p12(M, pro, epi, g, tail);
    if (op == GEMV_AR) return gemv_find_ar_p12(M, pro, epi, g, tail);
    return tail ? nullptr : gemv_find_moe_p12(op, M, pro, epi, g);
  }
  if (wf == WF_P13) return op == GEMV_DENSE ? gemv_find<GEMV_DENSE, WF_P13>(M, pro, epi, g, false) : nullptr;
  switch (op) {
    case GEMV_DENSE: return gemv_find<GEMV_DENSE, WF_BF16>(M, pro, epi, g, false);
    case GEMV_AR: return gemv_find<GEMV_AR, WF_BF16>(M, pro, epi, g, false);
    case GEMV_MOE_PAIR: return gemv_find<GEMV_MOE_PAIR, WF_BF16>(M, pro, epi, g, false);
    default: return gemv_find<GEMV_MOE_COMBINE, WF_BF16>(M, pro, epi, g, false);
  }
}

// Geometry, lookup, launch. -8: no packed kernel for this launch, nothing was launched (EPI_AR, MoE: the
// caller launches the bf16 entry, the same bits); -7: no bf16 kernel, which the rule and the lists exclude.
static int gemv_run(GemvOp op, int M, int pro, int epi, const GemvArgs& a) {
  const GemvGeom g = gemv_geom(op, M, a.N, a.K, epi, a.pw.wf, pro);
  const GemvLaunch f = g.nt != 0 ? gemv_find_any(op, a.pw.wf, M, pro, epi, g, a.K) : nullptr;
  if (f == nullptr) return a.pw.wf == WF_BF16 ? -7 : -8;
  return f(a);
}

static GemvArgs gemv_args(const void* x, int x_stride, const void* nw, float eps, const void* W, void* out,
                          int out_stride, int N, int K, hipStream_t s) {
  GemvArgs a{};
  a.x = x, a.x_stride = x_stride, a.nw = nw, a.eps = eps, a.W = W;
  a.out = out, a.out_stride = out_stride, a.N = N, a.K = K, a.s = s;
  return a;
}

// The packed twin an entry was handed (`recs`: P12's row records, P13's row headers): both pointers, the
// records 4-B aligned, K on the format's and the op's rule, M a packed row count. False: the entry answers -1.
static bool packed_arg(GemvOp op, int wf, int M, int K, const void* planes, const void* recs, PackedW* pw) {
  const int rows = gemv_block_rows(op, M);
  if (planes == nullptr || recs == nullptr || (wf == WF_P12 && reinterpret_cast<uintptr_t>(recs) % 4 != 0) ||
      !gemv_packed_k_ok(op, wf, K) || rows < 1 || rows > kGemvMaxM)
    return false;
  *pw = PackedW{static_cast<const uint8_t*>(planes), static_cast<const uint8_t*>(recs), wf};
  return true;
}

static int gemv_dispatch(int M, const GemvArgs& a, int epi, bool mfma) {
  if (a.K % 8 != 0) return -1;
  if ((epi == EPI_SILU || epi == EPI_ROPE) && (a.N % 2 != 0)) return -1;
  // 3-16 rows: the MFMA form (profiles/r2_batched_decode.md: from 3 rows on the VALU dot products,
  // not the weight stream, set this kernel's time); 1-2 rows, or K off the 128-k tiles: VALU GEMV.
  // `mfma` pins the MFMA form at every row count: an engine that batches >= 3 rows decodes all its
  // steps on one form, so a request's tokens do not depend on how many rows shared its steps.
  if ((M > kGemvMaxM || mfma) && a.K % 128 == 0 && a.x_stride % 8 == 0)
    return gemvm_dispatch(M, a.x, a.x_stride, a.nw, a.eps, a.W, a.out, a.out_stride, a.N, a.K, epi, a.rope, a.s);
  if (epi < EPI_BF16 || epi > EPI_ROPE) return -4;
  if (epi == EPI_ROPE && a.nw == nullptr) return -5;
  if (M < 1 || M > kGemvValuMaxM) return -3;
  return gemv_run(GEMV_DENSE, M, a.nw != nullptr ? PRO_NORM : PRO_NONE, epi, a);
}

}  // namespace llmc

using namespace llmc;

extern "C" int llmc_gemv(int M, const void* x, int x_stride, const void* norm_w, float eps, const void* W, void* out,
                         int out_stride, int N, int K, int epi, int mfma, hipStream_t s) {
  if (epi == EPI_ROPE) return -5;
  return gemv_dispatch(M, gemv_args(x, x_stride, norm_w, eps, W, out, out_stride, N, K, s), epi, mfma != 0);
}

// llmc_gemv for M <= 2 with the weights streamed from their 13-bit planes (`planes`, `hdr`: wpack.hip;
// W: the bf16 tensor, read for raw rows). Same geometry, same bits as llmc_gemv.
extern "C" int llmc_gemv_p13(int M, const void* x, int x_stride, const void* norm_w, float eps, const void* W,
                             const void* planes, const void* hdr, void* out, int out_stride, int N, int K, int epi,
                             hipStream_t s) {
  if (epi == EPI_ROPE) return -5;
  GemvArgs a = gemv_args(x, x_stride, norm_w, eps, W, out, out_stride, N, K, s);
  if (!packed_arg(GEMV_DENSE, WF_P13, M, K, planes, hdr, &a.pw)) return -1;
  return gemv_dispatch(M, a, epi, false);
}

// llmc_gemv_p13 from the 12-bit planes and the row records (`recs`: wpack.hip, the P12 layout). K: whole
// 2048-weight units, or a multiple of 512 from 2048 up, the planes then with the row tail ("P12 with a tail").
extern "C" int llmc_gemv_p12(int M, const void* x, int x_stride, const void* norm_w, float eps, const void* W,
                             const void* planes, const void* recs, void* out, int out_stride, int N, int K, int epi,
                             hipStream_t s) {
  if (epi == EPI_ROPE) return -5;
  GemvArgs a = gemv_args(x, x_stride, norm_w, eps, W, out, out_stride, N, K, s);
  if (!packed_arg(GEMV_DENSE, WF_P12, M, K, planes, recs, &a.pw)) return -1;
  return gemv_dispatch(M, a, epi, false);
}

// The RoPE + paged-KV-write epilogue of a qkv projection of N rows. False: the entry answers -1.
static bool rope_epi(int N, void* q_out, int q_stride, void* k_cache, void* v_cache, const void* positions,
                     const void* slots, const void* cos_t, const void* sin_t, int nh, int nkv, int D, int bs,
                     const void* bias, RopeEpi* rope) {
  if (N != (nh + 2 * nkv) * D || D % 2 != 0 || reinterpret_cast<uintptr_t>(bias) % 4 != 0) return false;
  *rope = RopeEpi{(bf16_t*)q_out, q_stride, (bf16_t*)k_cache, (bf16_t*)v_cache, (const int32_t*)positions,
                  (const int32_t*)slots, (const float*)cos_t, (const float*)sin_t, nh, nkv, D, bs};
  rope->bias = static_cast<const bf16_t*>(bias);
  return true;
}

// qkv projection for decode with fused RMSNorm prologue and RoPE + paged-KV-write epilogue.
// bias (nullable): the projection's bias [N] bf16 in W's row order, added in f32 before the rotation.
extern "C" int llmc_gemv_qkv_rope(int M, const void* x, int x_stride, const void* norm_w, float eps, const void* W,
                                  int N, int K, void* q_out, int q_stride, void* k_cache, void* v_cache,
                                  const void* positions, const void* slots, const void* cos_t, const void* sin_t,
                                  int nh, int nkv, int D, int bs, int mfma, const void* bias, hipStream_t s) {
  GemvArgs a = gemv_args(x, x_stride, norm_w, eps, W, nullptr, 0, N, K, s);
  if (!rope_epi(N, q_out, q_stride, k_cache, v_cache, positions, slots, cos_t, sin_t, nh, nkv, D, bs, bias, &a.rope))
    return -1;
  return gemv_dispatch(M, a, EPI_ROPE, mfma != 0);
}

// llmc_gemv_qkv_rope for M <= 2 from the 13-bit planes of W (as llmc_gemv_p13).
extern "C" int llmc_gemv_qkv_rope_p13(int M, const void* x, int x_stride, const void* norm_w, float eps,
                                      const void* W, const void* planes, const void* hdr, int N, int K, void* q_out,
                                      int q_stride, void* k_cache, void* v_cache, const void* positions,
                                      const void* slots, const void* cos_t, const void* sin_t, int nh, int nkv, int D,
                                      int bs, const void* bias, hipStream_t s) {
  GemvArgs a = gemv_args(x, x_stride, norm_w, eps, W, nullptr, 0, N, K, s);
  if (!rope_epi(N, q_out, q_stride, k_cache, v_cache, positions, slots, cos_t, sin_t, nh, nkv, D, bs, bias, &a.rope) ||
      !packed_arg(GEMV_DENSE, WF_P13, M, K, planes, hdr, &a.pw))
    return -1;
  return gemv_dispatch(M, a, EPI_ROPE, false);
}

// llmc_gemv_qkv_rope for M <= 2 from the 12-bit planes of W (as llmc_gemv_p12).
extern "C" int llmc_gemv_qkv_rope_p12(int M, const void* x, int x_stride, const void* norm_w, float eps,
                                      const void* W, const void* planes, const void* recs, int N, int K, void* q_out,
                                      int q_stride, void* k_cache, void* v_cache, const void* positions,
                                      const void* slots, const void* cos_t, const void* sin_t, int nh, int nkv, int D,
                                      int bs, const void* bias, hipStream_t s) {
  GemvArgs a = gemv_args(x, x_stride, norm_w, eps, W, nullptr, 0, N, K, s);
  if (!rope_epi(N, q_out, q_stride, k_cache, v_cache, positions, slots, cos_t, sin_t, nh, nkv, D, bs, bias, &a.rope) ||
      !packed_arg(GEMV_DENSE, WF_P12, M, K, planes, recs, &a.pw))
    return -1;
  return gemv_dispatch(M, a, EPI_ROPE, false);
}

// Row-parallel decode projection with the all-reduce fused into the epilogue (EPI_AR, gemv_core.h):
// h = sum over ranks of W_r . x_r (+ h on rank 0), for M <= 2 tokens. `bases`: every rank's fused-AR
// buffer (car_proto.h layout), `cap` its bytes per data parity. The dense GEMV's geometry rule: same
// blocks, same accumulation order, same bits.
static int gemv_ar_entry(int M, GemvArgs a, const void* const* bases, void* host, int rank, int world, size_t cap) {
  if (a.K % 8 != 0 || a.N % 2 != 0 || world < 1 || world > kMaxRanks || rank < 0 || rank >= world) return -1;
  for (int r = 0; r < kMaxRanks; ++r)
    a.ar.P.base[r] = r < world ? static_cast<char*>(const_cast<void*>(bases[r])) : nullptr;
  a.ar.P.host = static_cast<uint32_t*>(host);
  a.ar.rank = rank;
  a.ar.world = world;
  a.ar.cap = static_cast<long>(cap);
  if (M < 1 || M > kGemvMaxM) return -3;
  return gemv_run(GEMV_AR, M, PRO_NONE, EPI_AR, a);
}

extern "C" int llmc_gemv_ar(int M, const void* x, int x_stride, const void* W, void* h, int h_stride, int N, int K,
                            const void* const* bases, void* host, int rank, int world, size_t cap, hipStream_t s) {
  return gemv_ar_entry(M, gemv_args(x, x_stride, nullptr, 0.f, W, h, h_stride, N, K, s), bases, host, rank, world, cap);
}

// llmc_gemv_ar with W_r streamed from its 12-bit planes and row records (`planes`, `recs`: wpack.hip, the P12
// layout, with the row tail where K is off the 2048-weight unit; W is read for raw rows). Same geometry, same
// blocks and granules, same bits as llmc_gemv_ar, so a rank may run this beside peers that run the bf16 launch.
// -8: no packed kernel for this geometry, nothing was launched (the caller launches llmc_gemv_ar).
extern "C" int llmc_gemv_ar_p12(int M, const void* x, int x_stride, const void* W, const void* planes, const void* recs,
                                void* h, int h_stride, int N, int K, const void* const* bases, void* host, int rank,
                                int world, size_t cap, hipStream_t s) {
  GemvArgs a = gemv_args(x, x_stride, nullptr, 0.f, W, h, h_stride, N, K, s);
  if (!packed_arg(GEMV_AR, WF_P12, M, K, planes, recs, &a.pw)) return -1;
  return gemv_ar_entry(M, a, bases, host, rank, world, cap);
}

// MoE decode (K11 at batch 1): one GEMV per (token, top-k slot) pair against the selected
// expert's weights; expert ids are read on device, so the launch is graph-replayable.
// norm_w: x is the raw hidden row, RMS-normalised in the prologue (the decode gate_up after the
// fused router); nullptr: x is used as is (down projection)
static int moe_gemv_entry(int npairs, GemvArgs a, const void* ids, int x_div, int epi) {
  if (a.K % 8 != 0) return -1;
  if (epi != EPI_BF16 && epi != EPI_SILU) return -4;
  a.ids = ids, a.x_div = x_div, a.ny = npairs;
  return gemv_run(GEMV_MOE_PAIR, 1, a.nw != nullptr ? PRO_NORM : PRO_NONE, epi, a);
}

extern "C" int llmc_moe_gemv(int npairs, const void* x, int x_stride, const void* norm_w, float eps, const void* W,
                             const void* ids, int x_div, void* out, int out_stride, int N, int K, int epi,
                             hipStream_t s) {
  return moe_gemv_entry(npairs, gemv_args(x, x_stride, norm_w, eps, W, out, out_stride, N, K, s), ids, x_div, epi);
}

// llmc_moe_gemv with the expert weights streamed from the 12-bit twin of the [E * N, K] view of the stack W
// (`planes`, `recs`: wpack.hip, the P12 layout; W is read for raw rows). K: whole 2048-weight units. Same
// geometry, same bits as llmc_moe_gemv; -8: no packed kernel for this geometry or epilogue, nothing was
// launched (the caller launches llmc_moe_gemv).
extern "C" int llmc_moe_gemv_p12(int npairs, const void* x, int x_stride, const void* norm_w, float eps, const void* W,
                                 const void* planes, const void* recs, const void* ids, int x_div, void* out,
                                 int out_stride, int N, int K, int epi, hipStream_t s) {
  GemvArgs a = gemv_args(x, x_stride, norm_w, eps, W, out, out_stride, N, K, s);
  if (!packed_arg(GEMV_MOE_PAIR, WF_P12, 1, K, planes, recs, &a.pw)) return -1;
  return moe_gemv_entry(npairs, a, ids, x_div, epi);
}

// MoE decode down projection fused with the combine: h[t] += sum_j w[t, j] * (W_down[ids[t, j]] . act[t*k + j])
// for top-2 routing (k == 2), one block per 16 output rows per token, each wave streaming its row
// of both experts (the geometry: gemv_geom.h). Expert-parallel ranks (ids -1) keep the separate GEMV + combine.
static int moe_combine_entry(int T, GemvArgs a, const void* ids, const void* w, int k) {
  if (k != 2 || a.K % 8 != 0) return -1;
  a.ids = ids, a.ny = T;
  a.rope.cos_t = static_cast<const float*>(w);  // the router weights [T, k]
  return gemv_run(GEMV_MOE_COMBINE, k, PRO_NONE, EPI_COMBINE, a);
}

extern "C" int llmc_moe_down_combine(int T, const void* act, int act_stride, const void* W, const void* ids,
                                     const void* w, void* h, int h_stride, int N, int K, int k, hipStream_t s) {
  return moe_combine_entry(T, gemv_args(act, act_stride, nullptr, 0.f, W, h, h_stride, N, K, s), ids, w, k);
}

// llmc_moe_down_combine from the 12-bit twin of W_down's [E * N, K] view (as llmc_moe_gemv_p12): the same
// fixed geometry, the same bits.
extern "C" int llmc_moe_down_combine_p12(int T, const void* act, int act_stride, const void* W, const void* planes,
                                         const void* recs, const void* ids, const void* w, void* h, int h_stride,
                                         int N, int K, int k, hipStream_t s) {
  GemvArgs a = gemv_args(act, act_stride, nullptr, 0.f, W, h, h_stride, N, K, s);
  if (!packed_arg(GEMV_MOE_COMBINE, WF_P12, k, K, planes, recs, &a.pw)) return -1;
  return moe_combine_entry(T, a, ids, w, k);
}

// What the launch of (op, M, N, K, epi) in weight format wf would run, from the functions the launches use;
// touches no GPU. out: nt, rpw, unroll (zeros: no such launch), and whether the library holds that kernel
// for every prologue the launch takes.
extern "C" int llmc_gemv_plan(int op, int M, int N, int K, int epi, int wf, int* out) {
  out[0] = out[1] = out[2] = out[3] = 0;
  if (op < GEMV_DENSE || op > GEMV_MOE_COMBINE) return -1;
  bool found = true;
  for (int pro : {PRO_NONE, PRO_NORM}) {
    const GemvGeom g = gemv_geom(static_cast<GemvOp>(op), M, N, K, epi, wf, pro);
    if (g.nt == 0) continue;
    out[0] = g.nt, out[1] = g.rpw, out[2] = g.unroll;
    found = found && gemv_find_any(static_cast<GemvOp>(op), wf, M, pro, epi, g, K) != nullptr;
  }
  out[3] = out[0] != 0 && found;
  return 0;
}

// ---- geometry sweep entry (microbenchmarks only: M = 1, fused norm, bf16 out) ----
namespace llmc {
template <int NT, int RPW, int UNROLL>
static int launch_sweep(const void* x, const void* nw, const void* W, void* out, int N, int K, hipStream_t s) {
  constexpr int WAVES = NT / kWave;
  const size_t lds = static_cast<size_t>(K) * sizeof(bf16_t) + WAVES * sizeof(float);
  const int grid = (N + WAVES * RPW - 1) / (WAVES * RPW);
  gemv_kernel<1, NT, RPW, UNROLL, PRO_NORM, EPI_BF16, false><<<grid, NT, lds, s>>>(
      (const bf16_t*)x, K, (const bf16_t*)nw, 1e-5f, (const bf16_t*)W, out, N, N, K, nullptr, 1, RopeEpi{}, CarArgs{});
  return static_cast<int>(hipGetLastError());
}
}  // namespace llmc

extern "C" int llmc_gemv_sweep(int variant, const void* x, const void* nw, const void* W, void* out, int N, int K,
                               hipStream_t s) {
  if (K % 8 != 0 || K * 2 > 64 * 1024) return -1;
  switch (variant) {
#define LLMC_SWEEP_X(v, nt, rpw, un) \
  case v: return launch_sweep<nt, rpw, un>(x, nw, W, out, N, K, s);
    LLMC_GEMV_SWEEP_GEOMS(LLMC_SWEEP_X)
#undef LLMC_SWEEP_X
    default: return -2;
  }
}
