// Packers of the lossless decode weight formats: 13 bits per weight (the reader: gemv_core.h, WF_P13),
// described first, and 12 bits per weight with patched exceptions (WF_P12), further down.
//
// A bf16 weight is s | e7..e0 | m6..m0. Per weight row the packer keeps
//  * the low byte (e0 m6..m0) as it is,
//  * a 4-bit code k = (e7..e1) - base, base = max(0, the row's largest e7..e1 - 15): one header
//    byte per row, a window of 32 exponents below the row's largest,
//  * the sign bit.
// A row with a weight below the window (a zero or denormal beside normal weights, an inf / NaN
// beside them) is RAW: header kP13Raw, and the GEMV reads that row from the bf16 tensor. Its
// planes are still written (codes against base 0, masked to 4 bits) so the buffer has no undefined
// bytes.
//
// Layout. Lane l of the wave that owns a row streams the 16-B chunks l + 64 i of it. A wave unit is
// 4 chunks per lane = 2048 weights = 3328 B, its three planes contiguous:
//   [L0: 64 x 16 B][L1: 64 x 16 B][N: 64 x 16 B][S: 64 x 4 B]
// For lane l, weight t = 8 c + e is element e of the lane's chunk c of the unit (k index
// 8 (l + 64 (4 u + c)) + e); group g = t / 4, j = t % 4:
//   L0 / L1 byte t (t < 16 / t - 16)   low byte of weight t
//   N dword c, byte j                  k(8 c + j) | k(8 c + 4 + j) << 4   (groups 2c | 2c + 1)
//   S bit 8 j + g                      sign of weight 4 g + j
// so the four high bytes of group g are ((S << (7 - g)) & 0x80808080) | (nibbles + base * 0x01010101).
#include "gemv_core.h"

namespace llmc {

// one wave per row: header = base, or kP13Raw; raw rows counted in *raw_count
__global__ __launch_bounds__(256) void wpack_header_kernel(const bf16_t* __restrict__ W, uint8_t* __restrict__ hdr,
                                                           int32_t* __restrict__ raw_count, int N, int K) {
  const int lane = threadIdx.x % kWave;
  const int row = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
  if (row >= N) return;  // wave-uniform
  const u32x4* w = reinterpret_cast<const u32x4*>(W + static_cast<int64_t>(row) * K);
  int hi = 0, lo = 127;
  for (int c = lane; c < K / 8; c += kWave) {
    const u32x4 v = w[c];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a = (v[i] >> 8) & 0x7f, b = (v[i] >> 24) & 0x7f;
      hi = max(hi, max(a, b));
      lo = min(lo, min(a, b));
    }
  }
  for (int o = 32; o; o >>= 1) {
    hi = max(hi, __shfl_xor(hi, o, kWave));
    lo = min(lo, __shfl_xor(lo, o, kWave));
  }
  if (lane == 0) {
    const int base = max(hi - 15, 0);
    const bool raw = lo < base;
    hdr[row] = raw ? kP13Raw : static_cast<uint8_t>(base);
    if (raw) atomicAdd(raw_count, 1);
  }
}

// one thread per (row, unit, lane): 4 chunks in, 52 B out
__global__ __launch_bounds__(256) void wpack_planes_kernel(const bf16_t* __restrict__ W,
                                                           const uint8_t* __restrict__ hdr, uint8_t* __restrict__ P,
                                                           int N, int K) {
  const int units = K / kP13UnitElems;
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gid >= static_cast<int64_t>(N) * units * kWave) return;
  const int lane = static_cast<int>(gid % kWave);
  const int u = static_cast<int>((gid / kWave) % units);
  const int64_t row = gid / kWave / units;
  const u32x4* w = reinterpret_cast<const u32x4*>(W + row * K);
  // the header kernel ran before on the same stream; a raw row's codes are taken against base 0
  const uint32_t hb = hdr[row];
  const uint32_t base = hb == kP13Raw ? 0u : hb;
  uint32_t lowb[8], nib[4], S = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const u32x4 v = w[lane + kWave * (4 * u + c)];
    uint32_t code[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // group g = 2 c + h: weights (v[2h] lo, hi, v[2h+1] lo, hi)
      const int g = 2 * c + h;
      uint32_t lb = 0, cd = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t b = (v[2 * h + j / 2] >> (16 * (j & 1))) & 0xffffu;
        lb |= (b & 0xffu) << (8 * j);
        cd |= ((((b >> 8) & 0x7fu) - base) & 0xfu) << (8 * j);
        S |= (b >> 15) << (8 * j + g);
      }
      lowb[g] = lb;
      code[h] = cd;
    }
    nib[c] = code[0] | (code[1] << 4);
  }
  uint8_t* p = P + (row * units + u) * kP13UnitBytes;
  u32x4 o;
  o = u32x4{lowb[0], lowb[1], lowb[2], lowb[3]};
  *reinterpret_cast<u32x4*>(p + lane * 16) = o;
  o = u32x4{lowb[4], lowb[5], lowb[6], lowb[7]};
  *reinterpret_cast<u32x4*>(p + 1024 + lane * 16) = o;
  o = u32x4{nib[0], nib[1], nib[2], nib[3]};
  *reinterpret_cast<u32x4*>(p + 2048 + lane * 16) = o;
  *reinterpret_cast<uint32_t*>(p + 3072 + lane * 4) = S;
}

// ---- P12: 12 bits per weight (the reader: gemv_core.h, WF_P12) ----
// Per weight the low byte and one nibble s << 3 | k, k = (e7..e1) - base in 3 bits: a window of 16
// exponents. The unit is P13's without the sign plane, [L0][L1][N] = 3072 B, same lane / chunk /
// element order; the four high bytes of a group are
//   ((n & 0x07070707) + base * 0x01010101) | ((n << 4) & 0x80808080).
// A weight outside the window is an exception: its code is written masked to 3 bits and its true
// bits go to the row's record, kP12RecDwords dwords:
//   [0]        base | count << 8, or kP12Raw (count 0) for a row with more than kP12MaxExc exceptions
//   [1 + i]    bf16 bits << 16 | k, i < count, sorted by k (k = q << 9 | lane << 3 | element: the
//              wave chunk, lane and element that the reader patches); the unused slots are zero
// The window: base = max(0, the row's largest e7..e1 - 7), or up to kP12WindowSteps - 1 below it
// where that leaves fewer exceptions (ties stay with the higher base). Exact zeros, denormals and
// tiny weights are exceptions; a raw row's codes are taken against base 0.
//
// P12 with a tail: K a multiple of 512 (a wave chunk: 64 lanes x 8 weights) off the 2048-weight unit,
// K > 2048. With U = K / 2048 and Q = (K / 512) % 4 (1..3), a row's planes are its U units as above and then
// Q * 768 tail bytes (row stride U * 3072 + Q * 768, a multiple of 256). Tail chunk c < Q holds the
// weights k = 2048 U + 512 c + 8 lane + e. The tail is the unit cut short, a lane's share of each plane
// contiguous so that it fetches the tail with the widest loads (the layout with one 512-B and one 256-B
// block per chunk cost two narrow loads per chunk and measured slower than bf16 on the Phi-3 shapes:
// profiles/r11_packed_tail.md section 1):
//   [A: 64 x 8 B (Q = 1) | 64 x 16 B]   lane's low bytes of chunk 0 (and of chunk 1), element e at + e
//   [B: 64 x 8 B, Q = 3 only]           lane's low bytes of chunk 2
//   [N: 64 x 4 Q B, at Q * 512]         lane's nibble dwords of chunks 0 .. Q-1, byte j of dword c =
//                                       code(e = j) | code(e = j + 4) << 4, the unit's convention
// i.e. the registers l0, l1[0..1], n[0..Q-1] of the unit's reader, in 2 (Q = 1, 2) or 3 (Q = 3) loads per
// lane. The record is the same: the base is chosen over the whole row, and a tail weight outside the
// window is an entry with q = k / 512 >= 4 U.
constexpr int kP12WindowSteps = 4;

// one wave per row, scanning the row in k order, so the record's bytes do not depend on timing
__global__ __launch_bounds__(256) void wpack12_record_kernel(const bf16_t* __restrict__ W, uint32_t* __restrict__ recs,
                                                             int32_t* __restrict__ counts, int N, int K) {
  __shared__ uint32_t slots[4][kP12MaxExc];
  const int lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
  const int row = blockIdx.x * 4 + wv;
  const bool live = row < N;  // wave-uniform; no early return: the block meets at the barrier below
  const u32x4* w = reinterpret_cast<const u32x4*>(W + static_cast<int64_t>(live ? row : 0) * K);
  const int nchunk = live ? K / 8 : 0;
  int hi = 0;
  for (int c = lane; c < nchunk; c += kWave) {
    const u32x4 v = w[c];
#pragma unroll
    for (int i = 0; i < 4; ++i) hi = max(hi, max(static_cast<int>((v[i] >> 8) & 0x7f), static_cast<int>((v[i] >> 24) & 0x7f)));
  }
  for (int o = 32; o; o >>= 1) hi = max(hi, __shfl_xor(hi, o, kWave));
  int cand[kP12WindowSteps], cnt[kP12WindowSteps];
#pragma unroll
  for (int d = 0; d < kP12WindowSteps; ++d) {
    cand[d] = max(hi - 7 - d, 0);
    cnt[d] = 0;
  }
  for (int c = lane; c < nchunk; c += kWave) {
    const u32x4 v = w[c];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int h = (v[i / 2] >> (16 * (i & 1) + 8)) & 0x7f;
#pragma unroll
      for (int d = 0; d < kP12WindowSteps; ++d) cnt[d] += (h < cand[d] || h > cand[d] + 7) ? 1 : 0;
    }
  }
#pragma unroll
  for (int d = 0; d < kP12WindowSteps; ++d)
    for (int o = 32; o; o >>= 1) cnt[d] += __shfl_xor(cnt[d], o, kWave);
  int base = cand[0], best = cnt[0];
#pragma unroll
  for (int d = 1; d < kP12WindowSteps; ++d)
    if (cnt[d] < best) {
      best = cnt[d];
      base = cand[d];
    }
  if (lane < kP12MaxExc) slots[wv][lane] = 0;
  __syncthreads();
  if (live && best <= kP12MaxExc) {  // wave-uniform
    int done = 0;
    for (int c0 = 0; c0 < nchunk; c0 += kWave) {  // chunk c0 + lane: k = 8 (c0 + lane) + e, ascending in (c0, lane, e)
      const u32x4 v = w[c0 + lane];                // K is a multiple of 512: every lane has a chunk
      uint32_t m = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int h = (v[i / 2] >> (16 * (i & 1) + 8)) & 0x7f;
        m |= (h < base || h > base + 7) ? 1u << i : 0u;
      }
      const uint64_t any = __ballot(m != 0);
      if (any == 0) continue;  // wave-uniform
      int mine = __popc(m), pre = mine;
      for (int o = 1; o < kWave; o <<= 1) {  // inclusive scan over the lanes
        const int t = __shfl_up(pre, o, kWave);
        if (lane >= o) pre += t;
      }
      int at = done + pre - mine;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (m >> i & 1u) {
          const uint32_t b = (v[i / 2] >> (16 * (i & 1))) & 0xffffu;
          if (at < kP12MaxExc) slots[wv][at] = b << 16 | static_cast<uint32_t>(8 * (c0 + lane) + i);
          ++at;
        }
      }
      done += __shfl(pre, kWave - 1, kWave);
    }
  }
  __syncthreads();
  if (!live) return;
  const bool raw = best > kP12MaxExc;
  uint32_t* rec = recs + static_cast<int64_t>(row) * kP12RecDwords;
  if (lane == 0) {
    rec[0] = raw ? static_cast<uint32_t>(kP12Raw) : static_cast<uint32_t>(base) | static_cast<uint32_t>(best) << 8;
    atomicAdd(counts + (raw ? 0 : 1), raw ? 1 : best);  // statistics only: no byte of the output depends on them
  }
  if (lane < kP12MaxExc) rec[1 + lane] = slots[wv][lane];
}

// one thread per (row, unit, lane): 4 chunks in, 48 B out; with a tail, one more "unit" per row whose
// threads write the lane's 8 + 4 bytes of each tail chunk
__global__ __launch_bounds__(256) void wpack12_planes_kernel(const bf16_t* __restrict__ W,
                                                             const uint32_t* __restrict__ recs, uint8_t* __restrict__ P,
                                                             int N, int K) {
  const int units = K / kP13UnitElems, tailq = (K / kP12ChunkElems) % 4;
  const int slots = units + (tailq ? 1 : 0);
  const int64_t row_bytes = static_cast<int64_t>(units) * kP12UnitBytes + tailq * kP12TailChunkBytes;
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gid >= static_cast<int64_t>(N) * slots * kWave) return;
  const int lane = static_cast<int>(gid % kWave);
  const int u = static_cast<int>((gid / kWave) % slots);
  const int64_t row = gid / kWave / slots;
  const u32x4* w = reinterpret_cast<const u32x4*>(W + row * K);
  const uint32_t hb = recs[row * kP12RecDwords] & 0xffu;  // the record kernel ran before on the same stream
  const uint32_t base = hb == kP12Raw ? 0u : hb;
  if (u == units) {  // the tail: chunk c of the lane is the row's chunk lane + 64 (4 units + c)
    uint8_t* t = P + row * row_bytes + static_cast<int64_t>(units) * kP12UnitBytes;
    for (int c = 0; c < tailq; ++c) {
      const u32x4 v = w[lane + kWave * (4 * units + c)];
      uint32_t lb[2], cd[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        lb[h] = cd[h] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t b = (v[2 * h + j / 2] >> (16 * (j & 1))) & 0xffffu;
          lb[h] |= (b & 0xffu) << (8 * j);
          cd[h] |= (((((b >> 8) & 0x7fu) - base) & 0x7u) | (b >> 15) << 3) << (8 * j);
        }
      }
      // low bytes: chunks 0, 1 in A (8 B per lane with one chunk, else 16), chunk 2 in B
      uint8_t* lo = c == 2 ? t + 1024 + lane * 8 : t + lane * (tailq == 1 ? 8 : 16) + c * 8;
      *reinterpret_cast<u32x2*>(lo) = u32x2{lb[0], lb[1]};
      *reinterpret_cast<uint32_t*>(t + tailq * 512 + (lane * tailq + c) * 4) = cd[0] | (cd[1] << 4);
    }
    return;
  }
  uint32_t lowb[8], nib[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const u32x4 v = w[lane + kWave * (4 * u + c)];
    uint32_t code[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint32_t lb = 0, cd = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t b = (v[2 * h + j / 2] >> (16 * (j & 1))) & 0xffffu;
        lb |= (b & 0xffu) << (8 * j);
        cd |= (((((b >> 8) & 0x7fu) - base) & 0x7u) | (b >> 15) << 3) << (8 * j);
      }
      lowb[2 * c + h] = lb;
      code[h] = cd;
    }
    nib[c] = code[0] | (code[1] << 4);
  }
  uint8_t* p = P + row * row_bytes + static_cast<int64_t>(u) * kP12UnitBytes;
  *reinterpret_cast<u32x4*>(p + lane * 16) = u32x4{lowb[0], lowb[1], lowb[2], lowb[3]};
  *reinterpret_cast<u32x4*>(p + 1024 + lane * 16) = u32x4{lowb[4], lowb[5], lowb[6], lowb[7]};
  *reinterpret_cast<u32x4*>(p + 2048 + lane * 16) = u32x4{nib[0], nib[1], nib[2], nib[3]};
}

}  // namespace llmc

using namespace llmc;

// W bf16 [N, K] (K a multiple of 512 from 2048 up, at most kP12MaxK) -> planes [N, K / 2048 * 3072 +
// (K / 512) % 4 * 768] bytes, recs [N, 17] dwords, counts int32 [2] += (raw rows, exceptions of the packed rows).
extern "C" int llmc_wpack12(const void* W, void* planes, void* recs, void* counts, int N, int K, hipStream_t s) {
  if (N <= 0 || K < kP13UnitElems || K % kP12ChunkElems != 0 || K > kP12MaxK) return -1;
  wpack12_record_kernel<<<(N + 3) / 4, 256, 0, s>>>((const bf16_t*)W, (uint32_t*)recs, (int32_t*)counts, N, K);
  const int64_t threads = static_cast<int64_t>(N) * ((K + kP13UnitElems - 1) / kP13UnitElems) * kWave;
  wpack12_planes_kernel<<<static_cast<unsigned>((threads + 255) / 256), 256, 0, s>>>(
      (const bf16_t*)W, (const uint32_t*)recs, (uint8_t*)planes, N, K);
  return static_cast<int>(hipGetLastError());
}

// W bf16 [N, K] (K a multiple of 2048) -> planes [N, K / 2048, 3328] bytes, hdr [N] bytes (the
// buffer may be longer), raw_count int32 [1] += the number of raw rows.
extern "C" int llmc_wpack13(const void* W, void* planes, void* hdr, void* raw_count, int N, int K, hipStream_t s) {
  if (N <= 0 || K <= 0 || K % kP13UnitElems != 0) return -1;
  wpack_header_kernel<<<(N + 3) / 4, 256, 0, s>>>((const bf16_t*)W, (uint8_t*)hdr, (int32_t*)raw_count, N, K);
  const int64_t threads = static_cast<int64_t>(N) * (K / kP13UnitElems) * kWave;
  wpack_planes_kernel<<<static_cast<unsigned>((threads + 255) / 256), 256, 0, s>>>(
      (const bf16_t*)W, (const uint8_t*)hdr, (uint8_t*)planes, N, K);
  return static_cast<int>(hipGetLastError());
}
