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
//   kernel   k_route_rec: k_route's staging and walks over every record of a line, in order,
//            up to the first one some route matches (pick): record 0 lane = line, the other records of the
//            lines still unrouted lane = record, numbered through the wave.  It also writes the picked
//            view, one descriptor array per kind in which a result-bearing line owns exactly its picked
//            record, so that every first_only consumer acts on that record unchanged.
//   kernel   k_route_skip: lane = line, skip = repeat or (drop_unrouted and result-bearing and unrouted).
//   host     sdx_route_table_create / _destroy / _lds_routes, sdx_route_lines, sdx_route_records,
//            sdx_route_skip
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

struct Views {
  sdx_desc* v[4];  // by enum sdx_kind; nullptr where the kind is not given
};

// One record against every route -> its route and mask (k_route's loop; wave-uniform over the lanes that call it).
template <class TR>
__device__ __forceinline__ void match_record(const uint8_t* S, const uint8_t* __restrict__ blob, uint32_t n_routes,
                                             uint32_t n_class, uint32_t lds_routes, bool want_mask, const sdx_result* rp,
                                             const uint8_t* heap, int& route, uint64_t& mask) {
  const uint8_t* cls = S + (SDX_ROUTE_CLS_OFF - HDR);
  const sdx_route_dfa* dfa = reinterpret_cast<const sdx_route_dfa*>(S + (SDX_ROUTE_DFA_OFF - HDR));
  const sdx_result r0 = *rp;
  const uint8_t* p = heap + r0.payload_off;
  const uint32_t len = r0.payload_len;
  uint32_t head4 = 0;
  for (uint32_t j = 0; j < 4 && j < len; ++j) head4 |= (uint32_t)p[j] << (8 * j);
  for (uint32_t r = 0; r < n_routes; ++r) {
    const sdx_route_dfa d = dfa[r];
    if (!want_mask && route >= 0) continue;  // without a mask a lane stops at its first match
    bool hit;
    if (r < lds_routes)
      hit = walk<TR>(cls, S + (d.flags_off - HDR), reinterpret_cast<const TR*>(S + (d.trans_off - HDR)), n_class, d.start, p,
                     len, head4);
    else
      hit = walk<TR>(cls, blob + d.flags_off, reinterpret_cast<const TR*>(blob + d.trans_off), n_class, d.start, p, len,
                     head4);
    if (hit) {
      mask |= 1ull << r;
      if (route < 0) route = (int)r;
    }
  }
}

// k_route over every record of the line, in the launch's order, until one matches: pick = its index, route and
// mask are its.  No record matches (or no result): pick 0, route -1, mask 0.
// Phase 1, lane = line: record 0, exactly k_route's walks; most routed lines end here.
// Phase 2, lane = record: the records 1 .. n_rec - 1 of the wave's lines that are still unrouted are numbered
// through (a wave prefix sum of their counts, in registers) and taken 64 at a time, so that one line of hundreds
// of records does not hold its wave for hundreds of rounds.  A worker lane finds its record's line by a binary
// search over the lanes' prefix sums (shuffles); the line's own lane takes the lowest hit inside its range of
// the round's ballot -- records are numbered in list order, so that is the first match -- and that worker's
// route and mask.  Lines routed in an earlier round are not walked again.  No LDS beside the tables.
template <class TR>
__global__ __launch_bounds__(T) void k_route_rec(Kinds in, Views views, int n, const uint8_t* __restrict__ blob,
                                                 uint32_t n_routes, uint32_t n_class, uint32_t lds_routes,
                                                 uint32_t lds_words, int16_t* __restrict__ route_out,
                                                 uint64_t* __restrict__ mask_out, uint16_t* __restrict__ pick_out) {
  __shared__ uint32_t lds[SDX_ROUTE_LDS_BYTES / 4];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(blob + HDR);  // the blob is 16-byte aligned
  for (uint32_t w = threadIdx.x; w < lds_words; w += T) lds[w] = src[w];
  __syncthreads();
  const int g = blockIdx.x * T + threadIdx.x;
  const bool valid = g < n;  // lanes past the chunk stay: the shuffles below need the whole wave
  const int lane = threadIdx.x & 63;
  const uint8_t* S = reinterpret_cast<const uint8_t*>(lds);  // S + (a blob offset - HDR) = its staged copy
  const bool want_mask = mask_out != nullptr;
  auto recs = [&](int kd) { return kd == 0 ? in.k[0].rec : kd == 1 ? in.k[1].rec : kd == 2 ? in.k[2].rec : in.k[3].rec; };
  auto heaps = [&](int kd) { return kd == 0 ? in.k[0].heap : kd == 1 ? in.k[1].heap : kd == 2 ? in.k[2].heap : in.k[3].heap; };

  int own = -1;  // the kind whose records are the line's result: the lowest one (k_route)
  sdx_desc dk[4] = {};
#pragma unroll
  for (int kd = 3; kd >= 0; --kd) {
    if (!in.k[kd].desc || !valid) continue;
    dk[kd] = in.k[kd].desc[g];
    if (dk[kd].status == SDX_ST_OK && dk[kd].n_rec > 0) own = kd;
  }
  uint32_t rec_begin = 0, n_rec = 0;
#pragma unroll
  for (int kd = 0; kd < 4; ++kd)  // selects, so that dk stays in registers
    if (own == kd) {
      rec_begin = dk[kd].rec_begin;
      n_rec = dk[kd].n_rec;
    }

  uint64_t mask = 0;
  int route = -1;
  uint32_t pick = 0;
  if (own >= 0)
    match_record<TR>(S, blob, n_routes, n_class, lds_routes, want_mask, recs(own) + rec_begin, heaps(own), route, mask);

  const uint32_t cnt = (own >= 0 && route < 0) ? n_rec - 1 : 0;  // records still to look at; n_rec <= 65,535
  uint32_t incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(incl, d);
    if (lane >= d) incl += v;
  }
  const uint32_t total = __shfl(incl, 63);
  const uint32_t start = incl - cnt;
  for (uint32_t base = 0; base < total; base += 64) {  // wave-uniform
    const bool work = base + lane < total;
    const uint32_t it = work ? base + lane : 0;
    uint32_t lo = 0, hi = 63;  // the first lane whose inclusive sum exceeds it: that line has a record numbered it
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      const uint32_t mid = (lo + hi) >> 1;
      if (__shfl(incl, (int)mid) <= it) lo = mid + 1; else hi = mid;
    }
    const int o = (int)lo;
    const uint32_t o_start = __shfl(start, o), o_begin = __shfl(rec_begin, o);
    const int o_own = __shfl(own, o);
    const bool o_open = __shfl(route, o) < 0;
    int w_route = -1;
    uint64_t w_mask = 0;
    if (work && o_open)
      match_record<TR>(S, blob, n_routes, n_class, lds_routes, want_mask, recs(o_own) + o_begin + 1 + (it - o_start),
                       heaps(o_own), w_route, w_mask);
    const uint64_t hits = __ballot(w_route >= 0);
    const uint32_t a = start > base ? start : base, b = incl < base + 64 ? incl : base + 64;
    uint64_t mine = 0;
    if (cnt && route < 0 && a < b) mine = ((b - a >= 64 ? ~0ull : (1ull << (b - a)) - 1) << (a - base)) & hits;
    const int from = mine ? __ffsll((unsigned long long)mine) - 1 : lane;
    const int r2 = __shfl(w_route, from);
    const uint32_t m_lo = __shfl((uint32_t)w_mask, from), m_hi = __shfl((uint32_t)(w_mask >> 32), from);
    if (mine) {
      route = r2;
      mask = ((uint64_t)m_hi << 32) | m_lo;
      pick = 1 + (base + (uint32_t)from - start);
    }
  }
  if (!valid) return;
  route_out[g] = (int16_t)route;
  if (mask_out) mask_out[g] = mask;
  pick_out[g] = (uint16_t)pick;
#pragma unroll
  for (int kd = 0; kd < 4; ++kd) {
    if (!views.v[kd]) continue;
    sdx_desc d = dk[kd];  // another kind's slot, raised, overflowed, absent: the input's bytes
    if (own == kd) d = sdx_desc{d.rec_begin + pick, 1, SDX_ST_OK, 0};
    views.v[kd][g] = d;
  }
}

__global__ __launch_bounds__(T) void k_route_skip(Kinds in, int n, const int16_t* __restrict__ route,
                                                  const uint8_t* __restrict__ repeat, int drop_unrouted,
                                                  uint8_t* __restrict__ skip_out) {
  const int g = blockIdx.x * T + threadIdx.x;
  if (g >= n) return;
  bool have = false;
#pragma unroll
  for (int kd = 0; kd < 4; ++kd) {
    if (!in.k[kd].desc) continue;
    const sdx_desc d = in.k[kd].desc[g];
    have = have || (d.status == SDX_ST_OK && d.n_rec > 0);
  }
  skip_out[g] = ((repeat && repeat[g]) || (drop_unrouted && have && route[g] < 0)) ? 1 : 0;
}

static int bad_arg(const char* fn, const char* what) { return sdx::set_error(SDX_EINVAL, std::string(fn) + ": " + what); }

// kinds[0..k) by enum sdx_kind, as every entry here takes them; heaps: the records and heaps are read
static int take_kinds(const char* FN, const sdx_json_in* kinds, int k, int32_t n, bool heaps, Kinds* in, int* slot) {
  if (!kinds || k < 1 || k > 4) return bad_arg(FN, "1 to 4 kinds");
  if (n < 0) return bad_arg(FN, "n < 0");
  for (int i = 0; i < k; ++i) {
    const sdx_json_in& j = kinds[i];
    if (j.kind < SDX_KIND_MU || j.kind > SDX_KIND_MN) return bad_arg(FN, "bad kind");
    if (in->k[j.kind].desc) return bad_arg(FN, "a kind given twice");
    if (!j.desc_dev || (heaps && (!j.rec_dev || !j.heap_dev))) return bad_arg(FN, "null buffer");
    if (j.n != n) return bad_arg(FN, "every kind's n must be the chunk's n");
    in->k[j.kind] = KindIn{j.desc_dev, j.rec_dev, j.heap_dev};
    if (slot) slot[i] = j.kind;
  }
  return SDX_OK;
}

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
  if (!route_dev) return bad_arg(FN, "null route_dev");
  if (((uintptr_t)route_dev & 1) || ((uintptr_t)mask_dev & 7))
    return bad_arg(FN, "route_dev must be 2-byte, mask_dev 8-byte aligned");
  Kinds in{};
  if (const int rc = take_kinds(FN, kinds, k, n, true, &in, nullptr)) return rc;
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

extern "C" int sdx_route_records(const sdx_bank* bank, const sdx_route_table* table, const sdx_json_in* kinds, int k,
                                 int32_t n, int16_t* route_dev, uint64_t* mask_dev, uint16_t* pick_dev,
                                 sdx_desc* const* view_dev, void* hip_stream) {
  using namespace sdxq;
  static const char FN[] = "sdx_route_records";
  (void)bank;  // a payload is matched as bytes: no bank record is read
  if (!table || !table->dev) return bad_arg(FN, "null table");
  if (!route_dev || !pick_dev || !view_dev) return bad_arg(FN, "null route_dev, pick_dev or view_dev");
  if (((uintptr_t)route_dev & 1) || ((uintptr_t)pick_dev & 1) || ((uintptr_t)mask_dev & 7))
    return bad_arg(FN, "route_dev and pick_dev must be 2-byte, mask_dev 8-byte aligned");
  Kinds in{};
  int slot[4];
  if (const int rc = take_kinds(FN, kinds, k, n, true, &in, slot)) return rc;
  Views views{};
  for (int i = 0; i < k; ++i) {
    if (!view_dev[i]) return bad_arg(FN, "a null view");
    if ((uintptr_t)view_dev[i] & 3) return bad_arg(FN, "a view must be 4-byte aligned");
    views.v[slot[i]] = view_dev[i];
  }
  if (n == 0) return SDX_OK;
  const dim3 grid((n + T - 1) / T), blk(T);
  hipStream_t st = (hipStream_t)hip_stream;
  const uint8_t* blob = table->dev;
  if (table->width == 1)
    hipLaunchKernelGGL(k_route_rec<uint8_t>, grid, blk, 0, st, in, views, (int)n, blob, table->n_routes, table->n_class,
                       table->lds_routes, table->lds_bytes / 4, route_dev, mask_dev, pick_dev);
  else
    hipLaunchKernelGGL(k_route_rec<uint16_t>, grid, blk, 0, st, in, views, (int)n, blob, table->n_routes, table->n_class,
                       table->lds_routes, table->lds_bytes / 4, route_dev, mask_dev, pick_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SDX_OK : sdx::set_error(SDX_EHIP, std::string(FN) + ": " + hipGetErrorString(e));
}

extern "C" int sdx_route_skip(const sdx_json_in* kinds, int k, int32_t n, const int16_t* route_dev,
                              const uint8_t* repeat_dev, int drop_unrouted, uint8_t* skip_dev, void* hip_stream) {
  using namespace sdxq;
  static const char FN[] = "sdx_route_skip";
  if (!route_dev || !skip_dev) return bad_arg(FN, "null route_dev or skip_dev");
  if ((uintptr_t)route_dev & 1) return bad_arg(FN, "route_dev must be 2-byte aligned");
  Kinds in{};
  if (const int rc = take_kinds(FN, kinds, k, n, false, &in, nullptr)) return rc;
  if (n == 0) return SDX_OK;
  hipLaunchKernelGGL(k_route_skip, dim3((n + T - 1) / T), dim3(T), 0, (hipStream_t)hip_stream, in, (int)n, route_dev,
                     repeat_dev, drop_unrouted, skip_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SDX_OK : sdx::set_error(SDX_EHIP, std::string(FN) + ": " + hipGetErrorString(e));
}
