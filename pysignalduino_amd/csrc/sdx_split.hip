// sdx_split.hip -- raw transport bytes -> line offsets (sdx_split_lines), hand-written HIP for gfx950.
//
// What StreamReader.readline() does in the reference (signalduino/transport.py:113-123), for a whole
// read buffer at once: every '\n' ends a line and the line keeps it (k_parse_lines strips it with the
// rest of the white space); the bytes after the last '\n' are the unterminated tail, which becomes one
// more line only at EOF (`final`).  The output is the offsets_dev[n + 1] array sdx_parse_lines reads.
//
// Two kernels on the caller's stream, no look-back and no spinning (as k_sel_count / k_sel_write of
// sdx_lines.hip): k_split_count leaves each workgroup's '\n' count in scratch, k_split_write sums the
// counts in front of its own span, ranks its own '\n's and stores one offset per line.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sdx.h"

namespace sdx {
int set_error(int code, const std::string& msg);  // sdx_kernels.hip
}

namespace sdxs {

constexpr int THREADS = 256;                      // 4 waves
constexpr int LANE_BYTES = 16;                    // one load per lane and round
constexpr int ROUND_BYTES = THREADS * LANE_BYTES;  // 4 KB: the workgroup's loads of one round are contiguous
constexpr int ROUNDS = 4;
constexpr int SPAN = ROUNDS * ROUND_BYTES;        // 16 KB per workgroup: 4096 workgroups for a 64 MB chunk
constexpr int WAVES = THREADS / 64;
static_assert(SPAN == SDX_SPLIT_SPAN, "include/sdx.h states the span (sdx_split_work_bytes)");

__host__ __device__ inline int64_t nblocks(int64_t nbytes) { return nbytes > 0 ? (nbytes + SPAN - 1) / SPAN : 1; }

// bit j set <=> byte j of w is '\n'.  The exact zero-byte test (no borrow runs into the byte above, as
// the (v - 0x01..) & ~v form has), then the eight 0x80 marks gathered into one byte by a multiply whose
// partial products 2^(8i + 7k) never meet
__host__ __device__ inline uint32_t nl_mask8(uint64_t w) {
  const uint64_t v = w ^ 0x0A0A0A0A0A0A0A0Aull, lo7 = 0x7F7F7F7F7F7F7F7Full;
  const uint64_t z = ~(((v & lo7) + lo7) | v | lo7);  // 0x80 in every byte that was '\n'
  return (uint32_t)(((z >> 7) * 0x0102040810204080ull) >> 56);
}

// the '\n's among the 16 bytes at q (bit j = byte q + j), bytes at or after nbytes masked out; lanes
// whose 16 bytes start at or after nbytes load nothing (the last load reads < 16 bytes past nbytes)
__device__ __forceinline__ uint32_t lane_mask(const uint8_t* bytes, int64_t q, int64_t nbytes) {
  if (q >= nbytes) return 0;
  const uint64_t* p = reinterpret_cast<const uint64_t*>(bytes + q);
  const uint64_t a = p[0], b = p[1];
  const uint32_t m = nl_mask8(a) | (nl_mask8(b) << 8);
  const int64_t left = nbytes - q;
  return left >= LANE_BYTES ? m : m & ((1u << (int)left) - 1u);
}

__global__ __launch_bounds__(THREADS) void k_split_count(const uint8_t* __restrict__ bytes, int64_t nbytes,
                                                         int32_t* __restrict__ scratch) {
  __shared__ int32_t wsum[WAVES];
  const int64_t base = (int64_t)blockIdx.x * SPAN + (int64_t)threadIdx.x * LANE_BYTES;
  uint32_t m[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) m[r] = lane_mask(bytes, base + (int64_t)r * ROUND_BYTES, nbytes);
  int c = 0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) c += __popc(m[r]);
  for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += wsum[w];
    scratch[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(THREADS) void k_split_write(const uint8_t* __restrict__ bytes, int64_t nbytes, int final_,
                                                         int nblk, const int32_t* __restrict__ scratch,
                                                         int64_t* __restrict__ offsets, int cap,
                                                         int64_t* __restrict__ count) {
  __shared__ int32_t red[2][WAVES];
  __shared__ uint32_t wcnt[ROUNDS][WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // the loads first: their latency runs beside the prefix sum over scratch
  const int64_t base = (int64_t)blockIdx.x * SPAN + (int64_t)threadIdx.x * LANE_BYTES;
  uint32_t m[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) m[r] = lane_mask(bytes, base + (int64_t)r * ROUND_BYTES, nbytes);
  // total = every workgroup's count, pre = the counts in front of this workgroup (both < 2^31: nbytes is)
  int t = 0, p = 0;
  for (int b = threadIdx.x; b < nblk; b += THREADS) {
    const int v = scratch[b];
    t += v;
    if (b < (int)blockIdx.x) p += v;
  }
  for (int d = 32; d; d >>= 1) {
    t += __shfl_xor(t, d);
    p += __shfl_xor(p, d);
  }
  // the lanes' counts of two rounds per register (each < 2^16: a wave's 64 x 16 bytes), scanned over the wave
  uint32_t s01 = __popc(m[0]) | (__popc(m[1]) << 16), s23 = __popc(m[2]) | (__popc(m[3]) << 16);
  const uint32_t own01 = s01, own23 = s23;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t a = __shfl_up(s01, d), b = __shfl_up(s23, d);
    if (lane >= d) {
      s01 += a;
      s23 += b;
    }
  }
  if (lane == 63) {
    wcnt[0][wave] = s01 & 0xFFFF;
    wcnt[1][wave] = s01 >> 16;
    wcnt[2][wave] = s23 & 0xFFFF;
    wcnt[3][wave] = s23 >> 16;
  }
  if (lane == 0) {
    red[0][wave] = t;
    red[1][wave] = p;
  }
  __syncthreads();
  int total = 0, rank = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    total += red[0][w];
    rank += red[1][w];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    offsets[0] = 0;
    if (total == 0) {  // no '\n' at all: everything is tail (a line only at EOF)
      const bool line = final_ && nbytes > 0;
      if (line && cap > 0) offsets[1] = nbytes;
      count[0] = line ? 1 : 0;
      count[1] = line ? nbytes : 0;
    }
  }
  const uint32_t ex01 = s01 - own01, ex23 = s23 - own23;  // the lanes before this one, same wave and round
  const uint32_t excl[ROUNDS] = {ex01 & 0xFFFF, ex01 >> 16, ex23 & 0xFFFF, ex23 >> 16};
  // rank order = byte order: round, then wave, then lane
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    int k = rank + (int)excl[r];
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) k += (int)wcnt[r][w];
      rank += (int)wcnt[r][w];
    }
    const int64_t q = base + (int64_t)r * ROUND_BYTES;
    for (uint32_t mm = m[r]; mm; mm &= mm - 1, ++k) {
      const int64_t end = q + __builtin_ctz(mm) + 1;  // one past this '\n'
      if (k < cap) offsets[k + 1] = end;
      if (k == total - 1) {  // the last '\n' of the buffer: its lane knows the tail
        const bool line = final_ && end < nbytes;
        if (line && total < cap) offsets[total + 1] = nbytes;
        count[0] = total + (line ? 1 : 0);
        count[1] = final_ ? nbytes : end;
      }
    }
  }
}

}  // namespace sdxs

// host side: how many of host[0, n) equal `value` -- the count of a chunk's lines before its bytes leave
// the host (LineStream.submit_bytes).  Byte sums of at most 255 compares, so the loop vectorises
extern "C" uint64_t sdx_host_count_byte(const uint8_t* host, uint64_t n, int value) {
  const uint8_t v = (uint8_t)value;
  uint64_t total = 0;
  for (uint64_t i = 0; i < n;) {
    const uint64_t e = n - i < 255 * 64 ? n : i + 255 * 64;
    uint8_t acc[64] = {};
    for (; i + 64 <= e; i += 64)
      for (int j = 0; j < 64; ++j) acc[j] += host[i + j] == v;
    for (; i < e; ++i) total += host[i] == v;   // only at the very end: fewer than 64 bytes
    for (int j = 0; j < 64; ++j) total += acc[j];
  }
  return total;
}

extern "C" size_t sdx_split_work_bytes(int64_t nbytes) {
  return (size_t)sdxs::nblocks(nbytes < 0 ? 0 : nbytes) * sizeof(int32_t);
}

extern "C" int sdx_split_lines(const uint8_t* bytes_dev, int64_t nbytes, int32_t final, int64_t* offsets_dev,
                               int32_t cap, int64_t* count_dev, int32_t* scratch_dev, void* hip_stream) {
  if (!bytes_dev || !offsets_dev || !count_dev || !scratch_dev)
    return sdx::set_error(SDX_EINVAL, "sdx_split_lines: null buffer");
  if (nbytes < 0 || nbytes >= ((int64_t)1 << 31))
    return sdx::set_error(SDX_EINVAL, "sdx_split_lines: nbytes must be in [0, 2^31)");
  if (cap < 0) return sdx::set_error(SDX_EINVAL, "sdx_split_lines: cap must be >= 0");
  if (((uintptr_t)bytes_dev & 7) != 0 || ((uintptr_t)offsets_dev & 7) != 0 || ((uintptr_t)count_dev & 7) != 0)
    return sdx::set_error(SDX_EINVAL, "sdx_split_lines: bytes_dev, offsets_dev and count_dev must be 8-byte aligned");
  const int nblk = (int)sdxs::nblocks(nbytes);
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(sdxs::k_split_count, dim3(nblk), dim3(sdxs::THREADS), 0, st, bytes_dev, nbytes, scratch_dev);
  hipLaunchKernelGGL(sdxs::k_split_write, dim3(nblk), dim3(sdxs::THREADS), 0, st, bytes_dev, nbytes, (int)final, nblk,
                     (const int32_t*)scratch_dev, offsets_dev, (int)cap, count_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return sdx::set_error(SDX_EHIP, std::string("sdx_split_lines: ") + hipGetErrorString(e));
  return SDX_OK;
}
