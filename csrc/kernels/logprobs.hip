// Token log-probabilities of a decode row, raw (before penalties, temperature and truncation):
//   lp[j] = l[j] - lse,   lse = M + ln(sum_i exp(l[i] - M)),   M = the row maximum, NaN entries left out.
// Two launches in the sampler's shape, both capturable, no atomics, a fixed reduction order (two runs
// give the same bits):
//   stage 1, grid (kParts, B) x 256: per part its maximum m_p, its sum s_p = sum exp(l - m_p) and its
//     top-N (logit, id) candidates ordered by (logit descending, id ascending), the sampler's
//     argmax_merge rule. A thread keeps its <= 16 entries of the part in registers; each of the four
//     waves takes its own top-N by N argmax rounds that knock out their winner, then the <= 80 entries of
//     the four lists are placed by counting the entries better than each. Runs BEFORE penalize_logits rewrites the row.
//   stage 2, grid B x 64, AFTER the sampler's launch: lse from the parts, a 64-way merge of the
//     candidate lists (lane p walks part p's list), the sampled id's raw logit, and the results at
//     column out_count[b] - 1 of the rings (the sampler's advance has counted the token already).
#include "common.h"

namespace llmc {

constexpr int kLpParts = 64;      // = the sampler's kParts: the same partition of the row
constexpr int kLpMaxTop = 20;     // widest top list
constexpr int kLpMaxPer = 4096;   // floats of one part's slice: 16 registers of each of 256 threads
constexpr int kLpNone = 0x7fffffff;

// better(a) if larger value, ties -> smaller index; NaN never wins
__device__ __forceinline__ void lp_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// The sampler's wave_argmax butterfly with the exchanges in the VALU (common.h xor_shfl: no LDS round
// trip per step; N rounds of it are this file's critical path). Needs all 64 lanes active.
template <int M>
__device__ __forceinline__ void lp_argmax_step(float& v, int& i, int lane) {
  const float ov = xor_shfl<M>(v, lane);
  const int oi = static_cast<int>(fbits(xor_shfl<M>(bitsf(static_cast<uint32_t>(i)), lane)));
  lp_merge(v, i, ov, oi);
}
__device__ __forceinline__ void lp_wave_argmax(float& v, int& i, int lane) {
  lp_argmax_step<32>(v, i, lane);
  lp_argmax_step<16>(v, i, lane);
  lp_argmax_step<8>(v, i, lane);
  lp_argmax_step<4>(v, i, lane);
  lp_argmax_step<2>(v, i, lane);
  lp_argmax_step<1>(v, i, lane);
}

// Merge of `nlists` ordered candidate lists ([nlists][N] in LDS, id -1 ends a list) by one full wave:
// lane p < nlists offers the head of list p, N rounds of the wave argmax, the winner's lane steps on.
// Lane r < N ends with the r-th best of all lists (id -1, -inf when they hold fewer).
__device__ __forceinline__ void lp_merge_lists(const float* cv, const int* ci, int nlists, int N, int lane,
                                               float& myv, int& myi) {
  int head = 0;
  float hv = -INFINITY;
  int hi = kLpNone;
  if (lane < nlists && N > 0 && ci[lane * N] >= 0) {
    hv = cv[lane * N];
    hi = ci[lane * N];
  }
  myv = -INFINITY;
  myi = -1;
  for (int r = 0; r < N; ++r) {
    float v = hv;
    int i = hi;
    lp_wave_argmax(v, i, lane);
    if (lane == r) {
      myv = v;
      myi = i == kLpNone ? -1 : i;
    }
    if (i != kLpNone && i == hi) {  // ids are unique: one lane
      ++head;
      hv = -INFINITY;
      hi = kLpNone;
      if (head < N && ci[lane * N + head] >= 0) {
        hv = cv[lane * N + head];
        hi = ci[lane * N + head];
      }
    }
  }
}

constexpr int kLpPerThread = kLpMaxPer / 256;  // slice entries a thread keeps in registers

// grid (kLpParts, B), 256 threads. part_m / part_s [B, kLpParts], cand_v / cand_i [B, kLpParts, N].
__global__ __launch_bounds__(256) void logprobs_stage1_kernel(const float* __restrict__ logits, int64_t row_stride,
                                                              int V, int N, float* __restrict__ part_m,
                                                              float* __restrict__ part_s, float* __restrict__ cand_v,
                                                              int* __restrict__ cand_i) {
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* row = logits + b * row_stride;
  const int per = (V + kLpParts - 1) / kLpParts;  // <= kLpMaxPer, checked by the launcher
  const int lo = min(V, p * per), hi = min(V, lo + per);
  const int n = hi - lo;
  const int kmax = (n + 255) >> 8;  // block-uniform
  __shared__ float red[4];
  __shared__ float lv[4 * kLpMaxTop];
  __shared__ int li[4 * kLpMaxTop];

  // entry k of this thread is slice index tid + 256 k; NaN marks "no entry" (padding, NaN input, knocked out)
  float e[kLpPerThread];
#pragma unroll
  for (int k = 0; k < kLpPerThread; ++k) {
    const int j = tid + 256 * k;
    e[k] = (k < kmax && j < n) ? row[lo + j] : __builtin_nanf("");
  }
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kLpPerThread; ++k) m = fmaxf(m, e[k]);  // fmaxf drops a NaN operand
  m = wave_max(m);
  if (lane == 0) red[w] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.f;
  if (m > -INFINITY) {  // an empty or all -inf part: s_p = 0, never exp(-inf - -inf)
#pragma unroll
    for (int k = 0; k < kLpPerThread; ++k)
      if (e[k] == e[k]) s += __expf(e[k] - m);
  }
  s = block_sum<256>(s, red);
  if (tid == 0) {
    part_m[b * kLpParts + p] = m;
    part_s[b * kLpParts + p] = s;
  }
  if (N == 0) return;

  // Each wave on its own (no block barrier per round): N rounds of a wave argmax over the lanes' best
  // entries; the winner's lane knocks its entry out and rescans its registers. Lane r keeps round r.
  float bv = -INFINITY;
  int bi = kLpNone;
#pragma unroll
  for (int k = 0; k < kLpPerThread; ++k) lp_merge(bv, bi, e[k], lo + tid + 256 * k);
  float myv = -INFINITY;
  int myi = -1;
  for (int r = 0; r < N; ++r) {
    float v = bv;
    int i = bi;
    lp_wave_argmax(v, i, lane);
    if (lane == r) {
      myv = v;
      myi = i == kLpNone ? -1 : i;
    }
    if (i != kLpNone && i == bi) {  // ids are unique: one lane
      const int kk = (i - lo - tid) >> 8;
      bv = -INFINITY;
      bi = kLpNone;
#pragma unroll
      for (int k = 0; k < kLpPerThread; ++k) {
        if (k < kmax) {  // block-uniform: a 128k vocabulary walks 8 of the 16
          if (k == kk) e[k] = __builtin_nanf("");
          lp_merge(bv, bi, e[k], lo + tid + 256 * k);
        }
      }
    }
  }
  if (lane < N) {
    lv[w * N + lane] = myv;
    li[w * N + lane] = myi;
  }
  __syncthreads();
  // The four ordered lists hold <= 80 entries with distinct ids: an entry's place in the part's list
  // is the number of entries better than it (no rounds). Places past the T valid entries get (-inf, -1).
  const int total = 4 * N;
  const int64_t cbase = (static_cast<int64_t>(b) * kLpParts + p) * N;
  if (tid >= total) return;
  const float v = lv[tid];
  const int i = li[tid];
  int better = 0, valid = 0;
  for (int j = 0; j < total; ++j) {
    const float ov = lv[j];
    const int oi = li[j];
    valid += oi >= 0;
    better += oi >= 0 && (ov > v || (ov == v && oi < i));
  }
  if (i >= 0 && better < N) {
    cand_v[cbase + better] = v;
    cand_i[cbase + better] = i;
  }
  if (tid < N && tid >= valid) {
    cand_v[cbase + tid] = -INFINITY;
    cand_i[cbase + tid] = -1;
  }
}

struct LogprobOut {
  const int32_t* out_count;  // [B] tokens counted so far, or null: column 0
  int cap;                   // columns of the rings
  float* lp_tok;             // [B, cap]
  float* lp_top_v;           // [B, cap, top_stride]
  int32_t* lp_top_i;         // [B, cap, top_stride]
  int top_stride;
};

// grid B, 64 threads
__global__ __launch_bounds__(64) void logprobs_stage2_kernel(const float* __restrict__ raw, int64_t row_stride, int V,
                                                             int N, const int32_t* __restrict__ tokens,
                                                             const float* __restrict__ part_m,
                                                             const float* __restrict__ part_s,
                                                             const float* __restrict__ cand_v,
                                                             const int* __restrict__ cand_i, LogprobOut o) {
  const int b = blockIdx.x, lane = threadIdx.x;
  __shared__ float term[kLpParts];
  __shared__ float cv[kLpParts * kLpMaxTop];
  __shared__ int ci[kLpParts * kLpMaxTop];

  const int c = o.out_count != nullptr ? o.out_count[b] - 1 : 0;
  if (c < 0 || c >= o.cap) return;  // uniform over the block

  const float mp = part_m[b * kLpParts + lane];
  const float M = wave_max(mp);
  term[lane] = mp > -INFINITY ? part_s[b * kLpParts + lane] * __expf(mp - M) : 0.f;
  const int64_t cbase = static_cast<int64_t>(b) * kLpParts * N;
  for (int j = lane; j < kLpParts * N; j += 64) {
    cv[j] = cand_v[cbase + j];
    ci[j] = cand_i[cbase + j];
  }
  __syncthreads();
  float sum = 0.f;
#pragma unroll 16
  for (int p = 0; p < kLpParts; ++p) sum += term[p];  // index order, the same in every lane
  const float lse = M + logf(sum);

  float myv;
  int myi;
  lp_merge_lists(cv, ci, kLpParts, N, lane, myv, myi);
  const int64_t col = static_cast<int64_t>(b) * o.cap + c;
  if (lane < N) {
    o.lp_top_v[col * o.top_stride + lane] = myi < 0 ? -INFINITY : myv - lse;
    o.lp_top_i[col * o.top_stride + lane] = myi;
  }
  if (lane == 0) {
    const int tok = tokens[b];
    const float l = (tok >= 0 && tok < V) ? raw[b * row_stride + tok] : __builtin_nanf("");
    o.lp_tok[col] = l - lse;
  }
}

}  // namespace llmc

using namespace llmc;

extern "C" int llmc_logprobs_stage1(const void* logits, int64_t row_stride, int B, int V, int N, void* part_m,
                                    void* part_s, void* cand_v, void* cand_i, hipStream_t s) {
  if (B <= 0 || V <= 0) return 0;
  if (N < 0 || N > kLpMaxTop || (V + kLpParts - 1) / kLpParts > kLpMaxPer) return static_cast<int>(hipErrorInvalidValue);
  logprobs_stage1_kernel<<<dim3(kLpParts, B), 256, 0, s>>>((const float*)logits, row_stride, V, N, (float*)part_m,
                                                           (float*)part_s, (float*)cand_v, (int*)cand_i);
  return static_cast<int>(hipGetLastError());
}

extern "C" int llmc_logprobs_stage2(const void* raw, int64_t row_stride, int B, int V, int N, const void* tokens,
                                    const void* part_m, const void* part_s, const void* cand_v, const void* cand_i,
                                    const void* out_count, int cap, void* lp_tok, void* lp_top_v, void* lp_top_i,
                                    int top_stride, hipStream_t s) {
  if (B <= 0 || V <= 0) return 0;
  if (N < 0 || N > kLpMaxTop || top_stride < N || cap <= 0) return static_cast<int>(hipErrorInvalidValue);
  LogprobOut o;
  o.out_count = (const int32_t*)out_count;
  o.cap = cap;
  o.lp_tok = (float*)lp_tok;
  o.lp_top_v = (float*)lp_top_v;
  o.lp_top_i = (int32_t*)lp_top_i;
  o.top_stride = top_stride;
  logprobs_stage2_kernel<<<B, 64, 0, s>>>((const float*)raw, row_stride, V, N, (const int32_t*)tokens,
                                          (const float*)part_m, (const float*)part_s, (const float*)cand_v,
                                          (const int*)cand_i, o);
  return static_cast<int>(hipGetLastError());
}
