// Packer of the lossless 13-bit decode weight format (the reader: gemv_core.h, WF_P13).
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

}  // namespace llmc

using namespace llmc;

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
