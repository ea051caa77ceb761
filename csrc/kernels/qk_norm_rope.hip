// K3n: per-head q/k RMSNorm + RoPE + paged-KV write (Qwen3): rope.hip's rope_kv_write with an RMSNorm
// over the head dimension in front of the rotation of every Q and every K head.
//
// Input: bf16 qkv rows [T, (nh + 2 nkv) * D] as the projection wrote them (Q and K heads
// PAIR-INTERLEAVED, rope.hip), q_norm / k_norm bf16 [D] in CANONICAL dimension order (one vector for
// all Q heads, one for all K heads of the layer), eps; the rest and the outputs are rope_kv_write's:
// rotated q, canonical order, to q_out; rotated k and raw v (bit for bit) into the paged cache at
// slots[t]; slot < 0 writes no cache. Prefill runs it after the qkv GEMM, decode after the qkv GEMV
// (EPI_BF16): the GEMV's RoPE epilogue owns 1-2 rows per wave and 4-32 per block, so a head's 128
// rows never meet in one block there and the head's sum of squares cannot be formed in it.
//
// Geometry: one wave per (token, Q-or-K head). Lane i holds rotation pair i as ONE 4-byte load: the
// row's [2i, 2i + 1] are (x_i, x_{i + D/2}), and its norm weights are (g[i], g[i + D/2]). The head's
// sum of squares is wave_sum (common.h: a fixed butterfly in the VALU, no atomics, no LDS), so a
// row's output is a function of that row's bits only. D = 128 fills the wave, D = 64 leaves lanes
// 32-63 idle (they add zeros). V is copied by further waves, 64 16-byte chunks each. Blocks are 4
// waves and the grid is (token, group of 4 waves): a one-token launch spreads its nh + nkv heads
// over (nh + nkv + v waves) / 4 blocks. No block waits on another.
//
// Numerics (ops/oracle.py rope_kv_write with norms), all f32:
//   inv = rsqrt(sum_d x_d^2 / D + eps);  y_d = x_d * inv * g_d  (no bf16 rounding of y)
//   o1 = y_i c - y_{i+D/2} s;  o2 = y_{i+D/2} c + y_i s;  both rounded once to bf16.
#include "common.h"

namespace llmc {

constexpr int kQnWaves = 4;  // waves per block

__global__ __launch_bounds__(kQnWaves* kWave) void qk_norm_rope_kv_write_kernel(
    const bf16_t* __restrict__ qkv, int qkv_stride, bf16_t* __restrict__ q_out, int q_stride,
    const int32_t* __restrict__ positions, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    bf16_t* __restrict__ k_cache, bf16_t* __restrict__ v_cache, const int32_t* __restrict__ slots, int nh, int nkv,
    int D, int bs, const bf16_t* __restrict__ q_norm, const bf16_t* __restrict__ k_norm, float eps, int groups) {
  const int t = blockIdx.x / groups;
  const int u = (blockIdx.x % groups) * kQnWaves + static_cast<int>(threadIdx.x) / kWave;  // wave-uniform
  const int lane = static_cast<int>(threadIdx.x) % kWave;
  const int half = D / 2;
  const int slot = slots != nullptr ? slots[t] : -1;
  const bf16_t* row = qkv + static_cast<int64_t>(t) * qkv_stride;
  const int64_t page = slot >= 0 ? slot / bs : 0;
  const int off = slot >= 0 ? slot % bs : 0;

  if (u < nh + nkv) {  // a Q or K head: norm, rotate, write
    const bool live = lane < half;  // D = 64: lanes 32-63 carry zeros through the reduction
    const int i = live ? lane : 0;
    const uint32_t pr = *reinterpret_cast<const uint32_t*>(row + u * D + 2 * i);
    const float x1 = live ? bf16_lo(pr) : 0.f;
    const float x2 = live ? bf16_hi(pr) : 0.f;
    const float ss = wave_sum(x1 * x1 + x2 * x2);
    const float inv = rsqrtf(ss / static_cast<float>(D) + eps);
    const bf16_t* g = u < nh ? q_norm : k_norm;
    const float y1 = x1 * inv * bf16_to_f32(g[i]);
    const float y2 = x2 * inv * bf16_to_f32(g[i + half]);
    const int64_t cs = static_cast<int64_t>(positions[t]) * half + i;
    const float c = cos_t[cs], s = sin_t[cs];
    const float o1 = y1 * c - y2 * s;
    const float o2 = y2 * c + y1 * s;
    // lanes (2j, 2j + 1) trade halves, so each lane stores one 4-byte pair: the even lane
    // (o1[2j], o1[2j + 1]) at dim 2j, the odd lane (o2[2j], o2[2j + 1]) at dim D/2 + 2j
    const float p1 = xor_shfl<1>(o1, lane);
    const float p2 = xor_shfl<1>(o2, lane);
    const bool odd = (lane & 1) != 0;
    const uint32_t w = odd ? pack_bf16x2(p2, o2) : pack_bf16x2(o1, p1);
    const int col = odd ? half + i - 1 : i;
    bf16_t* dst = nullptr;
    if (u < nh) {
      dst = q_out + static_cast<int64_t>(t) * q_stride + u * D;
    } else if (slot >= 0) {
      dst = k_cache + ((page * nkv + (u - nh)) * bs + off) * D;
    }
    if (live && dst != nullptr) *reinterpret_cast<uint32_t*>(dst + col) = w;
    return;
  }
  // V: 64 16-byte chunks per wave, copied unchanged
  const int per = D / 8;
  const int ci = (u - (nh + nkv)) * kWave + lane;
  if (slot >= 0 && ci < nkv * per) {
    const int kh = ci / per;
    const int i = (ci % per) * 8;
    bf16_t* dst = v_cache + ((page * nkv + kh) * bs + off) * D;
    *reinterpret_cast<u32x4*>(dst + i) = *reinterpret_cast<const u32x4*>(row + (nh + nkv + kh) * D + i);
  }
}

}  // namespace llmc

using namespace llmc;

extern "C" int llmc_qk_norm_rope_kv_write(const void* qkv, int qkv_stride, void* q_out, int q_stride,
                                          const void* positions, const void* cos_t, const void* sin_t, void* k_cache,
                                          void* v_cache, const void* slots, int T, int nh, int nkv, int D, int bs,
                                          const void* q_norm, const void* k_norm, float eps, hipStream_t s) {
  if (D != 64 && D != 128) return -1;
  if (T < 0 || nh < 1 || nkv < 1 || bs < 1 || q_norm == nullptr || k_norm == nullptr) return -1;
  // 16-byte V chunks and 4-byte pairs: row starts and strides aligned for them
  if (qkv_stride % 8 != 0 || q_stride % 2 != 0 || reinterpret_cast<uintptr_t>(qkv) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(q_out) % 4 != 0 || reinterpret_cast<uintptr_t>(k_cache) % 4 != 0 ||
      reinterpret_cast<uintptr_t>(v_cache) % 16 != 0)
    return -1;
  if (T == 0) return 0;
  const int v_waves = (nkv * (D / 8) + kWave - 1) / kWave;
  const int groups = (nh + nkv + v_waves + kQnWaves - 1) / kQnWaves;
  if (static_cast<int64_t>(T) * groups > 0x7fffffff) return -1;
  qk_norm_rope_kv_write_kernel<<<T * groups, kQnWaves * kWave, 0, s>>>(
      (const bf16_t*)qkv, qkv_stride, (bf16_t*)q_out, q_stride, (const int32_t*)positions, (const float*)cos_t,
      (const float*)sin_t, (bf16_t*)k_cache, (bf16_t*)v_cache, (const int32_t*)slots, nh, nkv, D, bs,
      (const bf16_t*)q_norm, (const bf16_t*)k_norm, eps, groups);
  return static_cast<int>(hipGetLastError());
}
