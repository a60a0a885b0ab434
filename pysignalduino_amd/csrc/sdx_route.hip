// sdx_route.hip -- payload routes (sdx_route_lines), hand-written HIP for gfx950.
//
// An ordered client list of (name, regex) pairs, compiled on the host into one search DFA per route over
// a shared byte-class alphabet (pysignalduino_amd/routes.py, regex_dfa.py), decides on the device which
// consumer a decoded telegram concerns: mask bit r = re.search(pattern_r, payload) over
// the payload of the line's first record, route = the lowest set bit, -1 = none.
//
// The file in the order it is written:
//   kernel   k_route: lane = line.  The workgroup stages cls_of, the DFA records and the tables of the
//            table's first routes into LDS (the blob's bytes behind its header, unchanged, so that a blob
//            offset o is LDS offset o - 32); routes behind the budget walk their tables in global memory.
//            The loop over routes is wave-uniform; every lane walks its own payload and stops at ACC_NOW
//            or DEAD.  The payload's first four bytes are kept in a register, the rest is read one byte
//            at a time, [off, off + len) only: nothing past a payload's end.
//   host     sdx_route_table_create / _destroy / _lds_routes, sdx_route_lines
// Table contents are never range-checked here: sdx_route_validate (sdx_route_layout.h) passed the whole
// blob before it was uploaded.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sdx.h"
#include "sdx_route_layout.h"

namespace sdx {
int set_error(int code, const std::string& msg);  // sdx_kernels.hip
}

struct sdx_route_table {
  int device;
  uint8_t* dev;  // the blob
  uint32_t nbytes, n_routes, n_class, width, lds_routes, lds_bytes;
};

namespace sdxq {

constexpr int T = SDX_ROUTE_TILE;
constexpr uint32_t HDR = sizeof(sdx_route_hdr);

struct KindIn {
  const sdx_desc* desc;  // nullptr: no launch of this kind
  const sdx_result* rec;
  const uint8_t* heap;
};
struct Kinds {
  KindIn k[4];  // by enum sdx_kind
};

// One route's walk over one payload -> does a match exist.  TR: the transition type; flags / trans: the
// route's tables, in LDS or in global memory (the caller's branch is wave-uniform).
template <class TR>
__device__ __forceinline__ bool walk(const uint8_t* cls, const uint8_t* flags, const TR* trans, uint32_t n_class,
                                     uint32_t start, const uint8_t* p, uint32_t len, uint32_t head4) {
  uint32_t st = start, f = flags[st], i = 0;
  while (!(f & (SDX_ROUTE_ACC_NOW | SDX_ROUTE_DEAD)) && i < len) {
    const uint32_t b = i < 4 ? (head4 >> (8 * i)) & 255u : p[i];
    st = trans[st * n_class + cls[b]];
    f = flags[st];
    ++i;
  }
  return (f & SDX_ROUTE_ACC_NOW) || (i == len && (f & SDX_ROUTE_ACC_END));
}

template <class TR>
__global__ __launch_bounds__(T) void k_route(Kinds in, int n, const uint8_t* __restrict__ blob, uint32_t n_routes,
                                             uint32_t n_class, uint32_t lds_routes, uint32_t lds_words,
                                             const uint8_t* __restrict__ repeat, int drop_unrouted,
                                             int16_t* __restrict__ route_out, uint64_t* __restrict__ mask_out,
                                             uint8_t* __restrict__ skip_out) {
  __shared__ uint32_t lds[SDX_ROUTE_LDS_BYTES / 4];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(blob + HDR);  // the blob is 16-byte aligned
  for (uint32_t w = threadIdx.x; w < lds_words; w += T) lds[w] = src[w];
  __syncthreads();
  const int g = blockIdx.x * T + threadIdx.x;
  if (g >= n) return;
  const uint8_t* S = reinterpret_cast<const uint8_t*>(lds);  // S + (a blob offset - HDR) = its staged copy
  const uint8_t* cls = S + (SDX_ROUTE_CLS_OFF - HDR);
  const sdx_route_dfa* dfa = reinterpret_cast<const sdx_route_dfa*>(S + (SDX_ROUTE_DFA_OFF - HDR));

  bool have = false;
  const uint8_t* p = nullptr;
  uint32_t len = 0;
#pragma unroll
  for (int kd = 3; kd >= 0; --kd) {  // a line belongs to one kind; the lowest kind wins otherwise (k_rep_keys)
    if (!in.k[kd].desc) continue;
    const sdx_desc d = in.k[kd].desc[g];
    if (d.status == SDX_ST_OK && d.n_rec > 0) {
      const sdx_result r = in.k[kd].rec[d.rec_begin];
      have = true;
      p = in.k[kd].heap + r.payload_off;
      len = r.payload_len;
    }
  }
  uint32_t head4 = 0;
  for (uint32_t i = 0; i < 4 && i < len; ++i) head4 |= (uint32_t)p[i] << (8 * i);

  uint64_t mask = 0;
  int route = -1;
  for (uint32_t r = 0; r < n_routes; ++r) {  // wave-uniform
    const sdx_route_dfa d = dfa[r];
    if (!have || (!mask_out && route >= 0)) continue;  // without a mask a lane stops at its first match
    bool hit;
    if (r < lds_routes)  // two calls, so that each walk's loads keep their address space
      hit = walk<TR>(cls, S + (d.flags_off - HDR), reinterpret_cast<const TR*>(S + (d.trans_off - HDR)), n_class, d.start,
                     p, len, head4);
    else
      hit = walk<TR>(cls, blob + d.flags_off, reinterpret_cast<const TR*>(blob + d.trans_off), n_class, d.start, p, len,
                     head4);
    if (hit) {
      mask |= 1ull << r;
      if (route < 0) route = (int)r;
    }
  }
  route_out[g] = (int16_t)route;
  if (mask_out) mask_out[g] = mask;
  if (skip_out) skip_out[g] = ((repeat && repeat[g]) || (drop_unrouted && have && route < 0)) ? 1 : 0;
}

static int bad_arg(const char* fn, const char* what) { return sdx::set_error(SDX_EINVAL, std::string(fn) + ": " + what); }

}  // namespace sdxq

extern "C" int sdx_route_table_create(const void* blob, size_t nbytes, int device, sdx_route_table** out) {
  using namespace sdxq;
  static const char FN[] = "sdx_route_table_create";
  if (!blob || !out) return bad_arg(FN, "null argument");
  const uint8_t* b = static_cast<const uint8_t*>(blob);
  if (const char* why = sdx_route_validate(b, nbytes)) return bad_arg(FN, why);  // nothing is uploaded
  sdx_route_hdr h;
  memcpy(&h, b, sizeof h);
  uint32_t lds_bytes = 0;
  const uint32_t lds_routes = sdx_route_lds_routes(b, SDX_ROUTE_LDS_BYTES, &lds_bytes);
  hipError_t e = hipSetDevice(device);
  void* d = nullptr;
  if (e == hipSuccess) e = hipMalloc(&d, nbytes);
  if (e == hipSuccess) e = hipMemcpy(d, blob, nbytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    return sdx::set_error(SDX_EHIP, std::string(FN) + ": " + hipGetErrorString(e));
  }
  *out = new sdx_route_table{device, static_cast<uint8_t*>(d), (uint32_t)nbytes, h.n_routes, h.n_class, h.trans_width,
                             lds_routes, lds_bytes};
  return SDX_OK;
}

extern "C" int sdx_route_table_destroy(sdx_route_table* table) {
  if (!table) return SDX_OK;
  if (table->dev) (void)hipFree(table->dev);
  delete table;
  return SDX_OK;
}

extern "C" int sdx_route_table_lds_routes(const sdx_route_table* table) { return table ? (int)table->lds_routes : -1; }

extern "C" int sdx_route_lines(const sdx_bank* bank, const sdx_route_table* table, const sdx_json_in* kinds, int k,
                               int32_t n, const uint8_t* repeat_dev, int drop_unrouted, int16_t* route_dev,
                               uint64_t* mask_dev, uint8_t* skip_dev, void* hip_stream) {
  using namespace sdxq;
  static const char FN[] = "sdx_route_lines";
  (void)bank;  // a payload is matched as bytes: no bank record is read
  if (!table || !table->dev) return bad_arg(FN, "null table");
  if (!kinds || k < 1 || k > 4) return bad_arg(FN, "1 to 4 kinds");
  if (n < 0) return bad_arg(FN, "n < 0");
  if (!route_dev) return bad_arg(FN, "null route_dev");
  if (((uintptr_t)route_dev & 1) || ((uintptr_t)mask_dev & 7))
    return bad_arg(FN, "route_dev must be 2-byte, mask_dev 8-byte aligned");
  Kinds in{};
  for (int i = 0; i < k; ++i) {
    const sdx_json_in& j = kinds[i];
    if (j.kind < SDX_KIND_MU || j.kind > SDX_KIND_MN) return bad_arg(FN, "bad kind");
    if (in.k[j.kind].desc) return bad_arg(FN, "a kind given twice");
    if (!j.desc_dev || !j.rec_dev || !j.heap_dev) return bad_arg(FN, "null buffer");
    if (j.n != n) return bad_arg(FN, "every kind's n must be the chunk's n");
    in.k[j.kind] = KindIn{j.desc_dev, j.rec_dev, j.heap_dev};
  }
  if (n == 0) return SDX_OK;
  const dim3 grid((n + T - 1) / T), blk(T);
  hipStream_t st = (hipStream_t)hip_stream;
  const uint8_t* blob = table->dev;
  if (table->width == 1)
    hipLaunchKernelGGL(k_route<uint8_t>, grid, blk, 0, st, in, (int)n, blob, table->n_routes, table->n_class,
                       table->lds_routes, table->lds_bytes / 4, repeat_dev, drop_unrouted, route_dev, mask_dev, skip_dev);
  else
    hipLaunchKernelGGL(k_route<uint16_t>, grid, blk, 0, st, in, (int)n, blob, table->n_routes, table->n_class,
                       table->lds_routes, table->lds_bytes / 4, repeat_dev, drop_unrouted, route_dev, mask_dev, skip_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SDX_OK : sdx::set_error(SDX_EHIP, std::string(FN) + ": " + hipGetErrorString(e));
}
