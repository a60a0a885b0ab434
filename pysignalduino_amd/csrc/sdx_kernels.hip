// sdx_kernels.hip -- MI355X (gfx950) kernels of the batched SIGNALduino demodulator and their C ABI.
//
// The engines are headers of this one translation unit:
//   sdx_tile.h      : the MU / MS tile engine (pulses_tile: stage, filter, decode, flush of one tile).
//                     Short messages (<= 256 pulses): one 512-thread workgroup (8 waves) per tile of 64
//                     messages, or of 128 for MS tiles without a message of more than 128 pulses; long
//                     messages (<= 4096): one 256-thread workgroup (4 waves) per tile of 4.
//   sdx_mc_blocks.h : the MC blocks of 256 frames (lane = frame for the gates, then whole protocols
//                     per wave over the block's compacted frames).
// Here: the kernels -- k_pulses (one tile per workgroup), k_ms_classes (each MS tile on its length
// class's instantiation), k_mc, k_step (a mixed step's MU, MS and MC ranges as one grid),
// k_copy_narrow -- and the C ABI that launches them (include/sdx.h).
#include "sdx_device.h"
#include "sdx_lane.h"
#include "sdx_mc.h"
#include "sdx_mc_blocks.h"
#include "sdx_tile.h"

#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

namespace sdx {

// one tile per workgroup: the short MU tiles (MR = 1: header fields from the message records) and the
// long MU / MS tiles
template <int KIND, int NW, int TM, int MR = 0>
__global__ __launch_bounds__((pulses_threads<KIND, NW>())) __attribute__((amdgpu_waves_per_eu(
    (NW <= 4 ? 4 : 1)))) void k_pulses(
    const void* __restrict__ bank, sdx_pulse_batch b, sdx_out out) {
  __shared__ PulsesLds<KIND, NW, TM> L;
  __shared__ int msg_of[TM];
  pulses_tile<KIND, NW, TM, MR>(bank, b, out, (int)blockIdx.x, L, msg_of);
}

// A copy on a few workgroups (sdx_copy_async_narrow): the streaming front end's device -> pinned-host
// result copies.  hipMemcpyAsync ran them as a blit kernel of 256 workgroups that held a slot on every CU
// for the whole PCIe transfer (0.4 ms per 500k-line chunk), beside the next chunks' demodulation
// tiles; this one holds nwg slots.  16-byte pieces when both ends are 16-byte aligned, bytes otherwise.
__global__ __launch_bounds__(256) void k_copy_narrow(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t n) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
  size_t done = 0;
  if ((((uintptr_t)dst | (uintptr_t)src) & 15u) == 0) {
    const size_t n16 = n >> 4;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (size_t i = t; i < n16; i += 4 * nt) {  // four 16-byte pieces in flight per thread
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i + u * nt < n16) v[u] = s4[i + u * nt];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i + u * nt < n16) d4[i + u * nt] = v[u];
    }
    done = n16 << 4;
  }
  for (size_t i = done + t; i < n; i += nt) dst[i] = src[i];
}

// MC, 256 frames per workgroup: k_mc<4, false> the frames of <= 64 characters (mc_block_c), k_mc<8, true>
// the longer ones (mc_block); sdx_demod_mc launches the second only when the batch may hold such frames
template <int MW, bool LONG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LONG ? 1 : MC_WPE))) void k_mc(const void* __restrict__ bank, sdx_mc_batch b, sdx_out out) {
  if constexpr (LONG) {
    __shared__ McLds<MW> L;
    mc_block<MW>(bank, b, out, (int)blockIdx.x, (int)threadIdx.x, L);
  } else {
    __shared__ McLdsC<MW> L;
    mc_block_c<MW>(bank, b, out, (int)blockIdx.x, (int)threadIdx.x, L);
  }
}

// ---------------------------------------------------------------------------------------------
// k_step: a mixed step's MU, MS and MC launches as one grid (sdx_demod_step).  Workgroups are
// dispatched in index order, so MU's tiles go first, then MS's (each tile on the instantiation of its
// length class, NW = 2 when no message has more than 128 pulses), then MC's frames, two 256-frame
// blocks per workgroup.  A kind's tiles start on the CU slots the previous kind's last tiles
// free: with one launch per kind, each launch's tail (its last round of tiles finishing unevenly)
// idled the CUs until the whole launch had ended.  One LDS union serves every kind (the MU tile is the
// largest at 80.7 KB; two MC blocks 80.9 KB) and every body fits the MU tile's 128 VGPRs, so each kind
// keeps its own occupancy (2 tiles per CU).
// ---------------------------------------------------------------------------------------------
// one MS tile on the instantiation of its length class: NW = 2 (2 bitmap words per id, 118 VGPRs)
// when none of its messages has more than 128 pulses, NW = 4 otherwise -- decided per tile, so no
// workgroup exists only to find that the tile is another launch's.  MR = 1: the header fields (and the
// length deciding the class) from the message records the grouping wrote (one 128-byte line per
// message instead of a sector of each SoA field)
// tm = 128 (large batches): workgroup w owns messages [128 w, 128 w + 128) of the order.  When none has
// more than 128 pulses they run as one 128-message NW = 2 tile, so the per-tile phases that keep
// one or two of the eight waves busy (survivor decode, flush scan) come half as often per message;
// otherwise as the 64-message NW = 4 tiles 2 w and 2 w + 1, one after the other in the same LDS.
// tm = 64: workgroup w is tile w, as before.  tm is block-uniform (a kernel argument)
union MsLds {
  PulsesLds<SDX_KIND_MS, 2, 64> n2;
  PulsesLds<SDX_KIND_MS, 4, 64> n4;
  PulsesLds<SDX_KIND_MS, 2, 128> w2;
};
constexpr int MS_TM_MAX = 128;  // msg_of[] of the kernels that run MS tiles
template <int MR>
SDX_DEV void ms_tile_by_class(const void* __restrict__ bank, const sdx_pulse_batch& b, const sdx_out& out, const int w,
                              const int tm, MsLds& L, int* msg_of) {
  const int ntot = b.sel_dev ? b.n_sel : b.n;
  const int m = w * tm + (int)threadIdx.x;
  int len = 0;
  if ((int)threadIdx.x < tm && m < ntot) {
    const int msg = b.sel_dev ? b.sel_dev[m] : m;
    if (MR)
      len = b.mrec_dev[msg].len;
    else
      len = b.len_dev ? b.len_dev[msg] : (int)(b.offsets_dev[msg + 1] - b.offsets_dev[msg]);
  }
  const bool wide = __syncthreads_or(len > 128) != 0;
  int t0 = w, nt = 1;
  if (tm > 64) {
    if (!wide) {
      pulses_tile<SDX_KIND_MS, 2, 128, MR>(bank, b, out, w, L.w2, msg_of);
      return;
    }
    t0 = 2 * w;
    nt = (t0 + 1) * 64 < ntot ? 2 : 1;
  }
  if (!wide) {
    pulses_tile<SDX_KIND_MS, 2, 64, MR>(bank, b, out, w, L.n2, msg_of);
  } else {
    // (two calls, not a loop over the tile: values hoisted out of such a loop stayed live across the
    // whole tile and spilled ~130 VGPRs)
    pulses_tile<SDX_KIND_MS, 4, 64, MR>(bank, b, out, t0, L.n4, msg_of);
    if (nt > 1) {
      __syncthreads();  // the first tile's flush still reads the LDS the next one initialises
      pulses_tile<SDX_KIND_MS, 4, 64, MR>(bank, b, out, t0 + 1, L.n4, msg_of);
    }
  }
}

// sdx_demod_pulses(MS): every tile on its length class's instantiation
template <int MR>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void k_ms_classes(
    const void* __restrict__ bank, sdx_pulse_batch b, sdx_out out, int tm) {
  __shared__ MsLds U;
  __shared__ int msg_of[MS_TM_MAX];
  ms_tile_by_class<MR>(bank, b, out, (int)blockIdx.x, tm, U, msg_of);
}

struct StepArgs {
  sdx_pulse_batch mu, ms;
  sdx_mc_batch mc;
  sdx_out mu_out, ms_out, mc_out;
  int t_mu, t_ms, b_mc;  // workgroups of each range (b_mc: pairs of 256-frame blocks)
  int ms_tm;             // messages per MS workgroup: 64 or 128 (ms_tile_by_class)
};
union StepLds {
  PulsesLds<SDX_KIND_MU, 4, 64> mu;
  MsLds ms;
  McLdsC<MC_SHORTW> mc[2];
};
static_assert(sizeof(StepLds) <= 81920, "two k_step workgroups per CU (160 KB of LDS)");
static_assert(sizeof(StepLds) + MS_TM_MAX * sizeof(int) <= 81920, "... with the kernel's msg_of[]");

template <int MRU, int MRS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void k_step(const void* __restrict__ bank,
                                                                                      StepArgs a) {
  static_assert(pulses_threads<SDX_KIND_MU, 4>() == 512 && pulses_threads<SDX_KIND_MS, 2>() == 512, "512-thread tiles");
  __shared__ StepLds U;
  __shared__ int msg_of[MS_TM_MAX];
  // the ranges in dispatch order: MU's tiles, MS's, then MC's block pairs
  int w = (int)blockIdx.x, r = 2;
  if (w < a.t_mu) {
    r = 0;
  } else {
    w -= a.t_mu;
    if (w < a.t_ms) r = 1;
    else w -= a.t_ms;
  }
  if (r == 0) {
    pulses_tile<SDX_KIND_MU, 4, 64, MRU>(bank, a.mu, a.mu_out, w, U.mu, msg_of);
  } else if (r == 1) {
    ms_tile_by_class<MRS>(bank, a.ms, a.ms_out, w, a.ms_tm, U.ms, msg_of);
  } else {
    const int half = (int)threadIdx.x >> 8;
    mc_block_c<MC_SHORTW>(bank, a.mc, a.mc_out, 2 * w + half, (int)threadIdx.x & 255, U.mc[half]);
  }
}

}  // namespace sdx

// =============================================================================================
// C-ABI
// =============================================================================================
struct sdx_bank {
  int device;
  void* dev;
  size_t nbytes;
  sdx_bank_hdr hdr;
};

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
namespace sdx {
size_t group_bytes(int n);  // sdx_group.hip
bool group_messages(const void* bank_dev, int kind, const sdx_pulse_batch& b, int32_t* order, sdx_msg_rec* mrec, uint8_t* work,
                    size_t bytes, hipStream_t st);
bool group_messages2(const void* bank_dev, const sdx_pulse_batch& bmu, int32_t* omu, sdx_msg_rec* rmu, uint8_t* wmu,
                     size_t cmu, const sdx_pulse_batch& bms, int32_t* oms, sdx_msg_rec* rms, uint8_t* wms, size_t cms,
                     hipStream_t st);
// for the other translation units (sdx_lines.hip, sdx_mn.hip): the error text of sdx_last_error()
// and the bank handle's fields
int set_error(int code, const std::string& msg) { return fail(code, msg); }
const void* bank_dev_ptr(const sdx_bank* b) { return b->dev; }
const sdx_bank_hdr* bank_hdr(const sdx_bank* b) { return &b->hdr; }
}  // namespace sdx
#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) return fail(SDX_EHIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

extern "C" {

int sdx_abi_version(void) { return SDX_ABI_VERSION; }

#ifdef SDX_PROF
int sdx_gprof_read(unsigned long long* out256, int reset) {
  HIPCHK(hipMemcpyFromSymbol(out256, HIP_SYMBOL(g_gprof), sizeof(unsigned long long) * 256));
  if (reset) {
    unsigned long long z[256] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_gprof), z, sizeof z));
  }
  return SDX_OK;
}
int sdx_prof_read(unsigned long long* out34, int reset) {
  HIPCHK(hipMemcpyFromSymbol(out34, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * 34));
  if (reset) {
    unsigned long long z[34] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof z));
  }
  return SDX_OK;
}
#endif
#ifdef SDX_WGTIME
int sdx_wgtime_read(unsigned long long* out, int n) {
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wgt), sizeof(unsigned long long) * 2 * (n < 65536 ? n : 65536)));
  return SDX_OK;
}
#endif
const char* sdx_last_error(void) { return g_err.c_str(); }

// sdx_source_hash(): defined in the build's generated translation unit (build.py, _lib/obj/sdx_hash.cpp),
// so a change of one source recompiles only that source

int sdx_layout_size(int which) {
  switch (which) {
    case 0: return (int)sizeof(sdx_bank_hdr);
    case 1: return (int)sizeof(sdx_patspec);
    case 2: return (int)sizeof(sdx_mu_proto);
    case 3: return (int)sizeof(sdx_ms_proto);
    case 4: return (int)sizeof(sdx_mc_proto);
    case 5: return (int)sizeof(sdx_result);
    case 6: return (int)sizeof(sdx_desc);
    case 7: return (int)sizeof(sdx_mu_desc);
    case 8: return (int)sizeof(sdx_mn_proto);
    case 9: return (int)sizeof(sdx_json_rec);
    case 10: return (int)sizeof(sdx_mu_filt);
    case 11: return (int)sizeof(sdx_ms_filt);
    case 12: return (int)sizeof(sdx_xchg_part);
    case 13: return (int)sizeof(sdx_xchg_wire);
    case 14: return (int)sizeof(sdx_wire_rec);
    case 15: static_assert(sizeof(sdx_msg_rec) == 128, "sdx_msg_rec is one 128-byte line"); return (int)sizeof(sdx_msg_rec);
    case 16: return (int)sizeof(sdx_pulse_batch);
    case 17: return (int)sizeof(sdx_out);
  }
  return -1;
}

int sdx_bank_create(const void* blob, size_t nbytes, int device, sdx_bank** out) {
  if (!blob || !out || nbytes < sizeof(sdx_bank_hdr)) return fail(SDX_EINVAL, "bad bank arguments");
  sdx_bank_hdr h;
  std::memcpy(&h, blob, sizeof h);
  if (h.magic != SDX_BANK_MAGIC || h.version != SDX_BANK_VERSION || h.total_bytes != nbytes)
    return fail(SDX_EBANK, "bank blob magic/version/size mismatch (rebuild the bank and the library)");
  if ((size_t)h.off_order + 2u * ((size_t)h.n_mu + h.n_ms + h.n_mu_groups + 1) > nbytes || h.off_rank > nbytes || h.n_mu > 65535u ||
      h.n_ms > 65535u || (size_t)h.off_mudesc + sizeof(sdx_mu_desc) * h.n_mu > nbytes ||
      (size_t)h.off_mmtab + h.mmtab_bytes > nbytes || h.mmtab_bytes > SDX_MMTAB_LDS || (h.mmtab_bytes & 15u) ||
      (h.off_mudesc & 15u) || (h.off_mmtab & 15u) || 17u * h.mm_states > h.mmtab_bytes || h.n_mn > SDX_MN_MAX ||
      (size_t)h.off_mn + sizeof(sdx_mn_proto) * h.n_mn > nbytes || (h.off_mn & 15u) ||
      (size_t)h.off_json + sizeof(sdx_json_rec) * ((size_t)h.n_mu + h.n_ms + h.n_mc + h.n_mn) > nbytes ||
      (size_t)h.off_mufilt + sizeof(sdx_mu_filt) * h.n_mu > nbytes || (h.off_mufilt & 127u) ||
      (size_t)h.off_msfilt + sizeof(sdx_ms_filt) * h.n_ms > nbytes || (h.off_msfilt & 127u) ||
      (size_t)h.off_mntab + SDX_MNTAB_BYTES > nbytes || (h.off_mntab & 15u))
    return fail(SDX_EBANK, "bank blob: processing-order section out of range");
  HIPCHK(hipSetDevice(device));
  void* d = nullptr;
  HIPCHK(hipMalloc(&d, nbytes));
  hipError_t e = hipMemcpy(d, blob, nbytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return fail(SDX_EHIP, std::string("bank upload: ") + hipGetErrorString(e));
  }
  sdx_bank* b = new sdx_bank{device, d, nbytes, h};
  *out = b;
  return SDX_OK;
}

int sdx_bank_destroy(sdx_bank* bank) {
  if (!bank) return SDX_OK;
  if (bank->dev) (void)hipFree(bank->dev);
  delete bank;
  return SDX_OK;
}

const void* sdx_bank_device_ptr(const sdx_bank* bank) { return bank ? bank->dev : nullptr; }

int sdx_copy_async(void* dst, const void* src, size_t nbytes, void* hip_stream) {
  if (!nbytes) return SDX_OK;
  if (!dst || !src) return fail(SDX_EINVAL, "sdx_copy_async: null pointer");
  HIPCHK(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDefault, (hipStream_t)hip_stream));
  return SDX_OK;
}

int sdx_copy_async_kind(void* dst, const void* src, size_t nbytes, int kind, void* hip_stream) {
  if (!nbytes) return SDX_OK;
  if (!dst || !src) return fail(SDX_EINVAL, "sdx_copy_async_kind: null pointer");
  if (kind < 0 || kind > 4) return fail(SDX_EINVAL, "sdx_copy_async_kind: kind must be a hipMemcpyKind (0-4)");
  HIPCHK(hipMemcpyAsync(dst, src, nbytes, (hipMemcpyKind)kind, (hipStream_t)hip_stream));
  return SDX_OK;
}

int sdx_copy_async_narrow(void* dst, const void* src, size_t nbytes, int nwg, void* hip_stream) {
  if (!nbytes) return SDX_OK;
  if (!dst || !src) return fail(SDX_EINVAL, "sdx_copy_async_narrow: null pointer");
  if (nwg < 1 || nwg > 1024) return fail(SDX_EINVAL, "sdx_copy_async_narrow: 1..1024 workgroups");
  hipLaunchKernelGGL(sdx::k_copy_narrow, dim3(nwg), dim3(256), 0, (hipStream_t)hip_stream, (uint8_t*)dst,
                     (const uint8_t*)src, nbytes);
  HIPCHK(hipGetLastError());
  return SDX_OK;
}

int sdx_fill_async(void* dst, int value, size_t nbytes, void* hip_stream) {
  if (!nbytes) return SDX_OK;
  if (!dst) return fail(SDX_EINVAL, "sdx_fill_async: null pointer");
  HIPCHK(hipMemsetAsync(dst, value, nbytes, (hipStream_t)hip_stream));
  return SDX_OK;
}

// Messages per MS workgroup (ms_tile_by_class).  128-message tiles halve the workgroup count, which pays
// only where the range still fills the device's tile slots several times over (256 CUs x 2 tiles):
// below MS_TILE128_MIN messages (stream chunks, small Engine.run batches) the 64-message tiles stay.
// Measured (k_ms_classes alone, 64 vs 128, DESIGN.md section 4 "128-message MS tiles"): 32k messages 0.075 vs
// 0.130 ms, 64k 0.124 vs 0.141, 128k 0.207 vs 0.217, 256k 0.374 vs 0.336, 333k 0.467 vs 0.411.
// SDX_MS_TILE=64|128 overrides the choice; read per call, so a test compares both in one process
constexpr int MS_TILE128_MIN = 262144;
static int ms_tile_msgs(int n) {
  const char* e = getenv("SDX_MS_TILE");
  if (e && e[0] == '6' && e[1] == '4' && !e[2]) return 64;
  if (e && e[0] == '1' && e[1] == '2' && e[2] == '8' && !e[3]) return 128;
  return n >= MS_TILE128_MIN ? 128 : 64;
}

int sdx_demod_pulses(const sdx_bank* bank, int kind, const sdx_pulse_batch* batch, const sdx_out* out,
                     void* hip_stream) {
  if (!bank || !batch || !out) return fail(SDX_EINVAL, "null argument");
  if (kind != SDX_KIND_MU && kind != SDX_KIND_MS) return fail(SDX_EINVAL, "kind must be MU or MS");
  if (kind == SDX_KIND_MS && (!batch->cp_slot_dev || !batch->ms_ok_dev)) return fail(SDX_EINVAL, "MS needs cp_slot/ms_ok");
  if ((uintptr_t)batch->mrec_dev & 127) return fail(SDX_EINVAL, "mrec_dev must be 128-byte aligned");
  // spill regions are addressed with 32-bit offsets (region index cursor_dev[3] x SPILL_BYTES)
  if (out->work_dev && out->work_cap > 0xFFFFFFFFull - sdx::SPILL_BYTES)
    return fail(SDX_EINVAL, "work_cap above 4 GiB - 112 KB: spill offsets are 32-bit");
  const int ntot = batch->sel_dev ? batch->n_sel : batch->n;
  if (ntot <= 0) return SDX_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  // short variant (<= 256 pulses, 64 messages per tile); the caller routes longer messages (<= 4096)
  // through sel_dev to sdx_demod_pulses_long
  const sdx_pulse_batch& b = *batch;
  const sdx_out& o = *out;
  constexpr int TM = 64;
  const int grid = (ntot + TM - 1) / TM;
  const int ms_tm = kind == SDX_KIND_MS ? ms_tile_msgs(ntot) : TM;  // k_ms_classes: 64 or 128 per workgroup
  const dim3 blk(sdx::pulses_threads<SDX_KIND_MU, 4>());
  static_assert(sdx::pulses_threads<SDX_KIND_MU, 4>() == sdx::pulses_threads<SDX_KIND_MS, 4>(), "one block shape");
  if (kind == SDX_KIND_MU && b.mrec_dev)
    hipLaunchKernelGGL((sdx::k_pulses<SDX_KIND_MU, 4, 64, 1>), dim3(grid), blk, 0, st, bank->dev, b, o);
  else if (kind == SDX_KIND_MU)
    hipLaunchKernelGGL((sdx::k_pulses<SDX_KIND_MU, 4, 64>), dim3(grid), blk, 0, st, bank->dev, b, o);
  else {
    // MS messages are mostly short (87 % of the bench corpus have <= 128 pulses): tiles whose
    // messages all fit 2 words per id run the NW = 2 instantiation (half the bitmap words and mask
    // arithmetic), the others the NW = 4 one; the grouping puts the long messages last (k_sig).
    // (An NW = 1 class for <= 64 pulses spilled thousands of VGPRs: not used.)  One launch decides
    // per tile (k_ms_classes)
    static_assert(sdx::pulses_threads<SDX_KIND_MS, 2>() == sdx::pulses_threads<SDX_KIND_MS, 4>(), "block shape");
    const dim3 ms_grid((ntot + ms_tm - 1) / ms_tm);
    if (b.mrec_dev)
      hipLaunchKernelGGL(sdx::k_ms_classes<1>, ms_grid, blk, 0, st, bank->dev, b, o, ms_tm);
    else
      hipLaunchKernelGGL(sdx::k_ms_classes<0>, ms_grid, blk, 0, st, bank->dev, b, o, ms_tm);
  }
  HIPCHK(hipGetLastError());
  return SDX_OK;
}

size_t sdx_pulses_work_bytes(int spill_tiles) { return (size_t)(spill_tiles > 0 ? spill_tiles : 0) * sdx::SPILL_BYTES; }

size_t sdx_group_work_bytes(int n) { return sdx::group_bytes(n); }

int sdx_group_pulses(const sdx_bank* bank, int kind, const sdx_pulse_batch* batch, int32_t* order_dev,
                     sdx_msg_rec* mrec_dev, void* work_dev, size_t work_cap, void* hip_stream) {
  if (!bank || !batch || !order_dev || !work_dev) return fail(SDX_EINVAL, "null argument");
  if (kind != SDX_KIND_MU && kind != SDX_KIND_MS) return fail(SDX_EINVAL, "kind must be MU or MS");
  if (kind == SDX_KIND_MS && (!batch->cp_slot_dev || !batch->ms_ok_dev)) return fail(SDX_EINVAL, "MS needs cp_slot/ms_ok");
  const int ntot = batch->sel_dev ? batch->n_sel : batch->n;
  if (ntot <= 0) return SDX_OK;
  if (work_cap < sdx::group_bytes(ntot)) return fail(SDX_EINVAL, "grouping workspace smaller than sdx_group_work_bytes(n)");
  if ((uintptr_t)mrec_dev & 127) return fail(SDX_EINVAL, "mrec_dev must be 128-byte aligned");
  if (!sdx::group_messages(bank->dev, kind, *batch, order_dev, mrec_dev, (uint8_t*)work_dev, work_cap,
                           (hipStream_t)hip_stream))
    return fail(SDX_EHIP, "message grouping (k_sig / radix sort) launch failed");
  return SDX_OK;
}

int sdx_group_step(const sdx_bank* bank, const sdx_group_job* mu, const sdx_group_job* ms, void* hip_stream) {
  if (!bank || !mu || !ms || !mu->batch || !ms->batch) return fail(SDX_EINVAL, "null argument");
  const sdx_group_job* job[2] = {mu, ms};
  for (int k = 0; k < 2; ++k) {
    const sdx_group_job& j = *job[k];
    if (!j.order_dev || !j.work_dev) return fail(SDX_EINVAL, "sdx_group_step: null order / work");
    if ((uintptr_t)j.mrec_dev & 127) return fail(SDX_EINVAL, "mrec_dev must be 128-byte aligned");
    const int n = j.batch->sel_dev ? j.batch->n_sel : j.batch->n;
    if (n > 0 && j.work_cap < sdx::group_bytes(n))
      return fail(SDX_EINVAL, "grouping workspace smaller than sdx_group_work_bytes(n)");
  }
  const int nmu = mu->batch->sel_dev ? mu->batch->n_sel : mu->batch->n;
  const int nms = ms->batch->sel_dev ? ms->batch->n_sel : ms->batch->n;
  if (nms > 0 && (!ms->batch->cp_slot_dev || !ms->batch->ms_ok_dev)) return fail(SDX_EINVAL, "MS needs cp_slot/ms_ok");
  if (nmu <= 0 || nms <= 0) {  // one side empty: the single grouping of the other
    const sdx_group_job& j = nmu > 0 ? *mu : *ms;
    if ((nmu > 0 ? nmu : nms) <= 0) return SDX_OK;
    return sdx_group_pulses(bank, nmu > 0 ? SDX_KIND_MU : SDX_KIND_MS, j.batch, j.order_dev, j.mrec_dev, j.work_dev,
                            j.work_cap, hip_stream);
  }
  if (!sdx::group_messages2(bank->dev, *mu->batch, mu->order_dev, mu->mrec_dev, (uint8_t*)mu->work_dev, mu->work_cap,
                            *ms->batch, ms->order_dev, ms->mrec_dev, (uint8_t*)ms->work_dev, ms->work_cap,
                            (hipStream_t)hip_stream))
    return fail(SDX_EHIP, "message grouping (k_sig2 / radix sort) launch failed");
  return SDX_OK;
}

int sdx_demod_pulses_long(const sdx_bank* bank, int kind, const sdx_pulse_batch* batch, const sdx_out* out,
                          void* hip_stream) {
  if (!bank || !batch || !out) return fail(SDX_EINVAL, "null argument");
  const int ntot = batch->sel_dev ? batch->n_sel : batch->n;
  if (ntot <= 0) return SDX_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  constexpr int TM = 4;
  const int grid = (ntot + TM - 1) / TM;
  if (kind == SDX_KIND_MU)
    hipLaunchKernelGGL((sdx::k_pulses<SDX_KIND_MU, 64, 4>), dim3(grid), dim3(256), 0, st, bank->dev, *batch, *out);
  else if (kind == SDX_KIND_MS)
    hipLaunchKernelGGL((sdx::k_pulses<SDX_KIND_MS, 64, 4>), dim3(grid), dim3(256), 0, st, bank->dev, *batch, *out);
  else
    return fail(SDX_EINVAL, "kind must be MU or MS");
  HIPCHK(hipGetLastError());
  return SDX_OK;
}

static_assert(sdx::MC_SHORTW * 16 == SDX_MC_SHORT_HEX, "k_mc<MC_SHORTW> holds SDX_MC_SHORT_HEX characters");

int sdx_demod_step(const sdx_bank* bank, const sdx_step* step, void* hip_stream) {
  if (!bank || !step) return fail(SDX_EINVAL, "null argument");
  if ((step->mu && !step->mu_out) || (step->ms && !step->ms_out) || (step->mc && !step->mc_out))
    return fail(SDX_EINVAL, "sdx_demod_step: a batch without its sdx_out");
  hipStream_t st = (hipStream_t)hip_stream;
  sdx::StepArgs a{};
  auto count = [](int n, int n_sel, const void* sel) { return sel ? n_sel : n; };
  // the fused kernel's forms: MU short and MS short (the two length classes), each with or without
  // message records, MC frames of <= SDX_MC_SHORT_HEX characters; longer MC frames keep their own
  // launches, after the fused kernel on the same stream
  const bool mc_fused = step->mc && step->mc->max_hex > 0 && step->mc->max_hex <= SDX_MC_SHORT_HEX;
  if (step->mc && (int)bank->hdr.n_mc > sdx::MC_CMAXP) return fail(SDX_EINVAL, "the MC kernel's gate mask holds 16 MC protocols");
  if (step->mu) {
    const sdx_pulse_batch& b = *step->mu;
    if ((uintptr_t)b.mrec_dev & 127) return fail(SDX_EINVAL, "mrec_dev must be 128-byte aligned");
    if (step->mu_out->work_dev && step->mu_out->work_cap > 0xFFFFFFFFull - sdx::SPILL_BYTES)
      return fail(SDX_EINVAL, "work_cap above 4 GiB - 112 KB: spill offsets are 32-bit");
    a.mu = b;
    a.mu_out = *step->mu_out;
    a.t_mu = (count(b.n, b.n_sel, b.sel_dev) + 63) / 64;
  }
  if (step->ms) {
    const sdx_pulse_batch& b = *step->ms;
    if (!b.cp_slot_dev || !b.ms_ok_dev) return fail(SDX_EINVAL, "MS needs cp_slot/ms_ok");
    if ((uintptr_t)b.mrec_dev & 127) return fail(SDX_EINVAL, "mrec_dev must be 128-byte aligned");
    if (step->ms_out->work_dev && step->ms_out->work_cap > 0xFFFFFFFFull - sdx::SPILL_BYTES)
      return fail(SDX_EINVAL, "work_cap above 4 GiB - 112 KB: spill offsets are 32-bit");
    a.ms = b;
    a.ms_out = *step->ms_out;
    const int nms = count(b.n, b.n_sel, b.sel_dev);
    a.ms_tm = ms_tile_msgs(nms);
    a.t_ms = (nms + a.ms_tm - 1) / a.ms_tm;
  }
  if (mc_fused) {
    a.mc = *step->mc;
    a.mc_out = *step->mc_out;
    a.b_mc = (count(a.mc.n, a.mc.n_sel, a.mc.sel_dev) + 511) / 512;
  }
  const long long grid = (long long)a.t_mu + a.t_ms + a.b_mc;
  if (grid > 0x7FFFFFFFll) return fail(SDX_EINVAL, "sdx_demod_step: grid too large");
  if (grid > 0) {
    const bool mru = a.mu.mrec_dev != nullptr, mrs = a.ms.mrec_dev != nullptr;
    if (mru && mrs)
      hipLaunchKernelGGL((sdx::k_step<1, 1>), dim3((unsigned)grid), dim3(512), 0, st, bank->dev, a);
    else if (mru)
      hipLaunchKernelGGL((sdx::k_step<1, 0>), dim3((unsigned)grid), dim3(512), 0, st, bank->dev, a);
    else if (mrs)
      hipLaunchKernelGGL((sdx::k_step<0, 1>), dim3((unsigned)grid), dim3(512), 0, st, bank->dev, a);
    else
      hipLaunchKernelGGL((sdx::k_step<0, 0>), dim3((unsigned)grid), dim3(512), 0, st, bank->dev, a);
    HIPCHK(hipGetLastError());
  }
  if (step->mc && !mc_fused) return sdx_demod_mc(bank, step->mc, step->mc_out, hip_stream);
  return SDX_OK;
}

int sdx_demod_mc(const sdx_bank* bank, const sdx_mc_batch* batch, const sdx_out* out, void* hip_stream) {
  if (!bank || !batch || !out) return fail(SDX_EINVAL, "null argument");
  if ((int)bank->hdr.n_mc > sdx::MC_CMAXP) return fail(SDX_EINVAL, "the MC kernel's gate mask holds 16 MC protocols");
  const int ntot = batch->sel_dev ? batch->n_sel : batch->n;
  if (ntot <= 0) return SDX_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  const int grid = (ntot + 255) / 256;
  hipLaunchKernelGGL((sdx::k_mc<sdx::MC_SHORTW, false>), dim3(grid), dim3(256), 0, st, bank->dev, *batch, *out);
  // the 65..128-character variant only when the caller cannot rule such frames out (VERDICT r04 #4:
  // over a batch without one, its grid of early-exiting waves still held CU slots beside MS)
  if (batch->max_hex <= 0 || batch->max_hex > SDX_MC_SHORT_HEX)
    hipLaunchKernelGGL((sdx::k_mc<sdx::MC_MAXW, true>), dim3(grid), dim3(256), 0, st, bank->dev, *batch, *out);
  HIPCHK(hipGetLastError());
  return SDX_OK;
}

}  // extern "C"
