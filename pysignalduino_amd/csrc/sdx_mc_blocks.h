// sdx_mc_blocks.h -- the MC engine's blocks of 256 frames (manchester.py "fixed" chain, gfx950):
// mc_stage (hex -> bits in LDS), mc_block_c (frames of <= 64 characters: k_mc<4, false> and k_step's
// MC range) and mc_block (65..128 characters: k_mc<8, true>), with their LDS structs.  The protocol
// methods are sdx_mc.h's.  Included by sdx_kernels.hip only; the result records (StageRec), wire_class
// and the wave helpers are sdx_tile.h's.
#pragma once
#include "sdx_mc.h"
#include "sdx_tile.h"

namespace sdx {

// =============================================================================================
// MC engine (manchester.py "fixed" chain), lane = frame, 12 clockrange protocols uniform
// =============================================================================================
// staged records / payload bytes per wave of mc_block.  (Sized when the short frames ran here too, so
// that k_mc<4> fit 4 workgroups per CU; 5 waves/SIMD with 96 / 2560 measured no faster:
// profiles/r05/dropped/time_mc5_*.log)
constexpr int MC_REC_CAP = 152, MC_HEAP_CAP = 3584;
constexpr int MC_WPE = 4;  // waves per EU asked of the compiler for k_mc<4> (k_mc<8>: 1)

// mc_block's LDS: the block of 65..128-character frames only (the short frames' is McLdsC)
template <int MW>
struct McLds {
  uint64_t bn[MW * 256];   // bits, polarity as given
  uint64_t bi[MW * 256];   // bits, polarity inverted
  StageRec rec[4][MC_REC_CAP];
  alignas(16) uint8_t heap[4][MC_HEAP_CAP];
};

// a[w] <<= S bits across the MW-word bitstring (MSB-first words, 0 <= S < 64 * MW), no dynamic
// register indexing
template <int MW>
SDX_DEV void shl_words(uint64_t* a, int S) {
  const int q = S >> 6, r = S & 63;
  uint64_t o[MW];
#pragma unroll
  for (int w = 0; w < MW; ++w) {
    uint64_t hi = 0, lo = 0;
#pragma unroll
    for (int k = 0; k < MW; ++k) {
      hi |= a[k] & (0ull - (uint64_t)(k == w + q));
      lo |= a[k] & (0ull - (uint64_t)(k == w + q + 1));
    }
    o[w] = r ? ((hi << r) | (lo >> (64 - r))) : hi;
  }
#pragma unroll
  for (int w = 0; w < MW; ++w) a[w] = o[w];
}

// hex -> MSB-first bits of a frame of 1..16 MW characters, both polarities, into the LDS words
// dn[w * 256] / di[w * 256] (helpers.py:168-188, manchester.py:36; leading zero nibbles dropped as
// bin(int(h, 16)) does, the last nibble always kept).  The characters come in with 2 MW + 1 aligned
// 8-byte loads issued together (hex_dev is readable 8 bytes past every frame's end) and are
// decoded in registers; the LDS words are written once.
template <int MW>
SDX_DEV void mc_stage(const uint8_t* src, int hl, uint64_t* dn, uint64_t* di, int* nN, int* nI, bool* ok) {
  constexpr int NR = 2 * MW + 1;
  const int s = (int)((uintptr_t)src & 7);
  const uint64_t* wp = reinterpret_cast<const uint64_t*>(src - s);
  uint64_t raw[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) raw[k] = (8 * k < s + hl) ? wp[k] : 0ull;
  uint64_t wn[MW], wi[MW];
#pragma unroll
  for (int w = 0; w < MW; ++w) wn[w] = wi[w] = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 2 * MW; ++k) {
    const uint64_t x = s ? ((raw[k] >> (8 * s)) | (raw[k + 1] << (64 - 8 * s))) : raw[k];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = 8 * k + j;
      const uint32_t c = (uint32_t)(x >> (8 * j)) & 0xFFu;
      const bool in = i < hl;
      const bool dig = c - '0' < 10u, up = c - 'A' < 6u, lo = c - 'a' < 6u;
      bad |= in && !(dig || up || lo);
      const uint32_t v = dig ? c - '0' : (c & 7u) + 9u;  // 'A'/'a' -> 10 ... 'F'/'f' -> 15
      const uint32_t vi = (dig || up) ? 15u - v : v;      // str.translate: uppercase only
      const int sh = 60 - 4 * (i & 15);
      wn[i >> 4] |= (uint64_t)(in ? v & 15u : 0u) << sh;
      wi[i >> 4] |= (uint64_t)(in ? vi & 15u : 0u) << sh;
    }
  }
  *ok = !bad;
  // leading zero nibbles (at most hl - 1 of them)
  auto lead = [&](const uint64_t* a) -> int {
    int f = 64 * MW;
#pragma unroll
    for (int w = MW - 1; w >= 0; --w)
      if (a[w]) f = 64 * w + __clzll((long long)a[w]);
    const int lz = f >> 2;
    return lz < hl - 1 ? lz : hl - 1;
  };
  const int lzn = lead(wn), lzi = lead(wi);
  shl_words<MW>(wn, 4 * lzn);
  shl_words<MW>(wi, 4 * lzi);
  *nN = 4 * (hl - lzn);
  *nI = 4 * (hl - lzi);
#pragma unroll
  for (int w = 0; w < MW; ++w) {
    dn[w * 256] = wn[w];
    di[w * 256] = wi[w];
  }
}

// The block of the long frames: 65..16 MW hex characters (MW = MC_MAXW = 8: up to 128).  Frames of
// <= 64 characters belong to mc_block_c (below) and are skipped here; sdx_demod_mc launches both, and
// a wave without long frames exits at once.  256 frames (blk = the block's index in the launch,
// tid = 0..255 the frame's thread) of a k_mc<MW, true> launch, which provides the LDS
template <int MW>
SDX_DEV void mc_block(const void* __restrict__ bank, const sdx_mc_batch& b, const sdx_out& out, const int blk,
                      const int tid, McLds<MW>& L) {
  const BankView bv = bank_view(bank);
  const int wave = tid >> 6, lane = tid & 63;
  const int ntot = b.sel_dev ? b.n_sel : b.n;
  const int gi = blk * 256 + tid;
  bool valid = gi < ntot;
  const int msg = valid ? (b.sel_dev ? b.sel_dev[gi] : gi) : 0;
  bool toolong = false;  // > MC_MAXW * 16 characters: left to sdx_demod_mc_general (status OVF_TILE)
  if (valid) {  // this launch's share: the long frames
    const int hl0 = b.len_dev ? b.len_dev[msg] : (int)(b.offsets_dev[msg + 1] - b.offsets_dev[msg]);
    valid = hl0 > MC_SHORTW * 16;
    if (valid && hl0 > MW * 16) {
      toolong = true;
      valid = false;
    }
  }
  if (toolong) {
    sdx_desc d;
    d.rec_begin = 0;
    d.n_rec = 0;
    d.status = SDX_ST_OVF_TILE;
    d.raise_kind = 0;
    out.desc_dev[msg] = d;
    atomicOr(&out.cursor_dev[2], 2u);
  }
  if (!__ballot(valid)) return;  // whole wave without long frames (nothing staged yet)
#ifdef SDX_PROF  // per-wave cycles of k_mc's phases (g_prof slots 27-31, tools/prof_phases.py), summed
  // in registers
  unsigned long long mcacc[5] = {0, 0, 0, 0, 0};
#define MCPROF_T(v) unsigned long long v = __builtin_amdgcn_s_memtime()
#define MCPROF_ADD(slot, v) mcacc[(slot) - 27] += __builtin_amdgcn_s_memtime() - (v)
#else
#define MCPROF_T(v)
#define MCPROF_ADD(slot, v)
#endif
  MCPROF_T(t_all);
  MCPROF_T(t_st);
  int w_heap = 0, w_rec = 0;  // the wave's staged payload bytes and records (wave-uniform)
  bool w_ovf = false;
  const LaneBits BN{&L.bn[tid], MW, false}, BI{&L.bi[tid], MW, false};
  // hex -> bits for both polarities (helpers.py:168-188: leading zero nibbles are dropped)
  int nN = 0, nI = 0;
  bool hex_ok = false;
  int clock = 0, mcbit = 0, flags = 0, only = -1;
  if (valid) {
    const int64_t off = b.offsets_dev[msg];
    const int hl = b.len_dev ? b.len_dev[msg] : (int)(b.offsets_dev[msg + 1] - off);
    clock = b.clock_dev[msg];
    mcbit = b.mcbitnum_dev[msg];
    flags = b.flags_dev[msg];
    if (b.only_dev) only = b.only_dev[msg];
    hex_ok = hl > 0 && hl <= MW * 16;
    if (hex_ok) mc_stage<MW>(b.hex_dev + off, hl, &L.bn[tid], &L.bi[tid], &nN, &nI, &hex_ok);
  }
  MCPROF_ADD(27, t_st);
  const int nmc = (int)bv.hdr->n_mc;
  int raise = 0, mycnt = 0;
  for (int p = 0; p < nmc; ++p) {
    MCPROF_T(t_m);
    const sdx_mc_proto* r = uniform_ptr(bv.mc + p);
    bool go = valid && !raise && (only < 0 || only == p);
    // gates of _demodulate_mc_data (manchester.py:70-89; clockrange fixed to [0] / [1])
    if (go && mcbit < (cld(&r->has_lmin) ? cld(&r->lmin) : -1)) go = false;
    if (go && mcbit > (cld(&r->has_lmax) ? cld(&r->lmax) : 9999)) go = false;
    if (go && cld(&r->has_cr) && !((double)clock > cld(&r->cr_lo) && (double)clock < cld(&r->cr_hi))) go = false;
    McOut o{0, 0, 0, 0, 0, 0, 0, 0};
    const bool inv = (cld(&r->invert) != 0) ^ ((flags & 3) != 0);  // (:91-96)
    const LaneBits& B = inv ? BI : BN;
    const int nb = inv ? nI : nN;
    if (go && !hex_ok) { raise = SDX_RAISE_TYPE; go = false; }  // len(None) -> TypeError
    if (go) {
      const LaneBits DM{B.base, MW, true};  // mc2dmc(lh/hl) view for Funkbus
      o = mc_method(r, cld(&r->method), B, nb, nb, DM);
      if (o.rc == -1) { raise = SDX_RAISE_TYPE; o.rc = 0; }
      if (o.rc == -2) { raise = SDX_RAISE_VALUE; o.rc = 0; }
    }
    // stage results of the wave in lane (= frame) order for this protocol
    const bool has = o.rc == 1;
    MCPROF_ADD(28, t_m);
    if (!ballot(has)) continue;  // no result in this wave: nothing to stage (wave-uniform)
    MCPROF_T(t_r);
    const int plen = has ? cld(&r->pre_len) + o.len : 0;
    int incl = plen;  // inclusive scan over lanes
    for (int d = 1; d < WAVE; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    const int wtot = __shfl(incl, WAVE - 1);
    const uint64_t hm = ballot(has);
    const int nnew = popc64(hm);
    const int hb = w_heap, rb = w_rec;
    const bool fits = hb + wtot <= MC_HEAP_CAP && rb + nnew <= MC_REC_CAP;
    if (has && fits) {
      uint8_t* dst = &L.heap[wave][hb + incl - plen];
      const int pl = cld(&r->pre_len), po = cld(&r->pre_off);
      for (int i = 0; i < pl; i += 8) {  // 8 independent loads per step
        uint8_t c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = (i + j < pl) ? bv.str[po + i + j] : (uint8_t)0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (i + j < pl) dst[i + j] = c[j];
      }
      mc_write(r, o, B, nb, nb, dst + cld(&r->pre_len));
      StageRec sr;
      sr.off = (uint32_t)(hb + incl - plen);
      sr.len = (uint16_t)plen;
      sr.proto = (uint16_t)p;
      sr.bitlen = 0;
      sr.msg = (uint16_t)lane;
      sr.rank = (uint16_t)mycnt;  // this frame's records so far (protocol order)
      L.rec[wave][rb + lanes_below(hm)] = sr;
      ++mycnt;
    }
    if (fits) {  // the wave's staging cursors are wave-uniform registers (every lane computes them)
      w_heap = hb + wtot;
      w_rec = rb + nnew;
    } else if (nnew) {
      w_ovf = true;
    }
    MCPROF_ADD(29, t_r);
  }
  wave_sync();  // the staged records and payloads of all lanes, for the flush
  MCPROF_T(t_f);
  // flush this wave's frames: records are staged in protocol-major order, each carrying its rank
  // among its frame's records; the wave writes them 64 at a time to (frame, protocol) order
  const int nr = w_rec;
  const int nh = (w_heap + 15) & ~15;  // 16-B pieces: every reservation keeps hbase aligned
  const bool bad = w_ovf;
  if (raise) mycnt = 0;
  int incl = mycnt;
  for (int d = 1; d < WAVE; d <<= 1) {
    const int t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  const int wrec = __shfl(incl, WAVE - 1);
  uint32_t rbase = 0, hbase = 0;
  int st = bad ? 2 : 0;
  if (lane == 0 && !bad) {
    rbase = atomicAdd(&out.cursor_dev[0], (uint32_t)wrec);
    hbase = atomicAdd(&out.cursor_dev[1], (uint32_t)nh);
    if (rbase + wrec > out.rec_cap || hbase + nh > out.heap_cap) { st = 3; atomicOr(&out.cursor_dev[2], 1u); }
  }
  if (lane == 0 && bad) atomicOr(&out.cursor_dev[2], 2u);
  rbase = (uint32_t)__shfl((int)rbase, 0);
  hbase = (uint32_t)__shfl((int)hbase, 0);
  st = __shfl(st, 0);
  // the exchange's counts (ABI 12): per frame payload << 32 | wire bytes, in this wave's slice of
  // the (now dead) bit rows
  const bool wx = out.wire_dev != nullptr;
  unsigned long long* wsum = reinterpret_cast<unsigned long long*>(&L.bn[64 * wave]);
  if (wx) {
    wsum[lane] = 0ull;
    wave_sync();
  }
  if (st == 0) {
    const int excl = incl - mycnt;
    for (int i0 = 0; i0 < nr; i0 += WAVE) {  // wave-uniform trip count (the shuffles below)
      const int i = i0 + lane;
      StageRec sr{};
      if (i < nr) sr = L.rec[wave][i];
      const int fl = i < nr ? (int)sr.msg : 0;
      const int fbase = __shfl(excl, fl), fmsg = __shfl(msg, fl), fraise = __shfl(raise, fl);
      if (i < nr && !fraise) {
        sdx_result o;
        o.payload_off = hbase + sr.off;
        o.payload_len = sr.len;
        o.proto = sr.proto;
        o.bit_length = 0;
        o.msg = (uint32_t)fmsg;
        out.rec_dev[rbase + fbase + sr.rank] = o;
        if (wx) {
          const uint32_t xr = wire_class(bv, SDX_KIND_MC, sr.proto, &L.heap[wave][sr.off], sr.len);
          if (out.xrec_dev) out.xrec_dev[rbase + fbase + sr.rank] = xr;
          atomicAdd(&wsum[fl], (unsigned long long)(((uint64_t)sr.len << 32) | wire_bytes_x(xr, sr.len)));
        }
      }
    }
    uint4* hd = reinterpret_cast<uint4*>(out.heap_dev + hbase);
    const uint4* hs = reinterpret_cast<const uint4*>(L.heap[wave]);
    if ((((uintptr_t)hd) & 15u) == 0) {
      for (int i = lane; i < (nh >> 4); i += WAVE) hd[i] = hs[i];
    } else {
      for (int i = lane; i < nh; i += WAVE) out.heap_dev[hbase + i] = L.heap[wave][i];
    }
  }
  if (valid) {
    sdx_desc d;
    d.rec_begin = rbase + (uint32_t)(incl - mycnt);
    if (raise) { d.status = SDX_ST_RAISED; d.raise_kind = (uint8_t)raise; d.n_rec = 0; }
    else if (st) { d.status = st == 2 ? SDX_ST_OVF_TILE : SDX_ST_OVF_OUT; d.raise_kind = 0; d.n_rec = 0; }
    else { d.status = SDX_ST_OK; d.raise_kind = 0; d.n_rec = (uint16_t)mycnt; }
    out.desc_dev[msg] = d;
  }
  if (wx) {
    wave_sync();
    if (valid) out.wire_dev[msg] = (!raise && st == 0) ? (uint64_t)wsum[lane] : 0ull;
  }
  MCPROF_ADD(30, t_f);
  MCPROF_ADD(31, t_all);
#ifdef SDX_PROF
  if (lane == 0)
    for (int i = 0; i < 5; ++i) atomicAdd(&g_prof[27 + i], mcacc[i]);
#endif
#undef MCPROF_T
#undef MCPROF_ADD
}

// ---------------------------------------------------------------------------------------------
// compacted MC block (frames of <= 64 characters).  mc_block runs every protocol on
// every wave: per (wave, protocol) the method and the result staging execute for the ~4 of 64 lanes
// whose frame passed the protocol's gates, i.e. 4 waves x 12 protocols of mostly idle method passes
// (measured: the methods + staging are 0.15 of k_mc's 0.18 ms; gates alone 0.03 ms).  Here the gates
// run lane = frame and leave a 12-bit mask per frame; then each wave takes whole protocols (an LDS
// counter) and runs the method over the frames of the WHOLE block that passed that protocol's gates,
// compacted 64 to a pass -- the protocol stays wave-uniform (scalar record loads, mc_method as is) --
// staging into block-wide pools; a block-level flush places the records in (frame, protocol) order.
// Results, statuses and raise kinds are the per-frame sequential loop's: a frame raises with the kind
// of the FIRST protocol (bank order) that raises for it, and then publishes nothing.
// ---------------------------------------------------------------------------------------------
constexpr int MC_BREC = 512, MC_BHEAP = 11264;  // block-wide staging pools (bench mean ~97 records,
                                                 // ~2.9 KB of payload per 256 frames)
constexpr int MC_CMAXP = 16;                      // protocols of the gate mask (the bank has 12)
constexpr uint32_t MC_NORAISE = 0xFFFFFFFFu;
template <int MW>
struct McLdsC {
  uint64_t bn[MW * 256];   // bits, polarity as given
  uint64_t bi[MW * 256];   // bits, polarity inverted
  StageRec rec[MC_BREC];
  alignas(16) uint8_t heap[MC_BHEAP];
  uint16_t gm[256];        // bit p: the frame passed protocol p's gates (and is valid hex)
  uint16_t nbits[2][256];  // len(bits) as given / inverted (leading zero nibbles dropped)
  uint8_t fl[256];         // the frame's flags (bits 0-1: message type / version)
  uint8_t list[4][256];    // per wave: the frames of the protocol it runs
  uint32_t fraise[256];    // p << 4 | kind of the first raising protocol (bank order), MC_NORAISE: none
  uint32_t rcur, hcur, pnext, ovf;
};

template <int MW>
SDX_DEV void mc_block_c(const void* __restrict__ bank, const sdx_mc_batch& b, const sdx_out& out, const int blk,
                        const int tid, McLdsC<MW>& L) {
  const BankView bv = bank_view(bank);
  const int wave = tid >> 6, lane = tid & 63;
  const int ntot = b.sel_dev ? b.n_sel : b.n;
  const int gi = blk * 256 + tid;
  bool valid = gi < ntot;
  const int msg = valid ? (b.sel_dev ? b.sel_dev[gi] : gi) : 0;
  const int nmc = (int)bv.hdr->n_mc;
  if (tid == 0) {
    L.rcur = 0;
    L.hcur = 0;
    L.pnext = 0;
    L.ovf = 0;
  }
  // ---- lane = frame: this launch's share, hex -> bits (both polarities), the gates of every protocol
  bool toolong = false;
  if (valid) {
    const int hl0 = b.len_dev ? b.len_dev[msg] : (int)(b.offsets_dev[msg + 1] - b.offsets_dev[msg]);
    valid = hl0 <= MC_SHORTW * 16;
    // a frame longer than the batch's promised bound (0 < max_hex <= 64: no long launch follows) is
    // marked for a re-run instead of being left without a descriptor
    if (!valid && b.max_hex > 0 && b.max_hex <= MC_SHORTW * 16) toolong = true;
  }
  if (toolong) {
    sdx_desc d;
    d.rec_begin = 0;
    d.n_rec = 0;
    d.status = SDX_ST_OVF_TILE;
    d.raise_kind = 0;
    out.desc_dev[msg] = d;
    atomicOr(&out.cursor_dev[2], 2u);
  }
  int nN = 0, nI = 0;
  bool hex_ok = false;
  int clock = 0, mcbit = 0, flags = 0, only = -1;
  if (valid) {
    const int64_t off = b.offsets_dev[msg];
    const int hl = b.len_dev ? b.len_dev[msg] : (int)(b.offsets_dev[msg + 1] - off);
    clock = b.clock_dev[msg];
    mcbit = b.mcbitnum_dev[msg];
    flags = b.flags_dev[msg];
    if (b.only_dev) only = b.only_dev[msg];
    hex_ok = hl > 0 && hl <= MW * 16;
    if (hex_ok) mc_stage<MW>(b.hex_dev + off, hl, &L.bn[tid], &L.bi[tid], &nN, &nI, &hex_ok);
  }
  // gates of _demodulate_mc_data (manchester.py:70-89; clockrange fixed to [0] / [1])
  uint32_t gm = 0;
  for (int p = 0; p < nmc; ++p) {
    const sdx_mc_proto* r = uniform_ptr(bv.mc + p);
    bool go = valid && (only < 0 || only == p);
    if (go && mcbit < (cld(&r->has_lmin) ? cld(&r->lmin) : -1)) go = false;
    if (go && mcbit > (cld(&r->has_lmax) ? cld(&r->lmax) : 9999)) go = false;
    if (go && cld(&r->has_cr) && !((double)clock > cld(&r->cr_lo) && (double)clock < cld(&r->cr_hi))) go = false;
    gm |= (uint32_t)go << p;
  }
  // a frame that is not valid hex raises at its first protocol past the gates (len(None) -> TypeError)
  // and runs no method
  const uint32_t r0 = (gm && !hex_ok) ? (((uint32_t)(__ffs(gm) - 1) << 4) | SDX_RAISE_TYPE) : MC_NORAISE;
  L.gm[tid] = hex_ok ? (uint16_t)gm : (uint16_t)0;
  L.nbits[0][tid] = (uint16_t)nN;
  L.nbits[1][tid] = (uint16_t)nI;
  L.fl[tid] = (uint8_t)(flags & 3);
  L.fraise[tid] = r0;
  __syncthreads();
  // ---- per wave: whole protocols, each over the block's frames that passed its gates, 64 per pass
  for (;;) {
    int p = 0;
    if (lane == 0) p = (int)atomicAdd(&L.pnext, 1u);
    p = __shfl(p, 0);
    if (p >= nmc) break;
    const sdx_mc_proto* r = uniform_ptr(bv.mc + p);
    int cnt = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int f = g * 64 + lane;
      const bool on = (L.gm[f] >> p) & 1u;
      const uint64_t m = ballot(on);
      if (on) L.list[wave][cnt + lanes_below(m)] = (uint8_t)f;
      cnt += popc64(m);
    }
    wave_sync();
    const bool pinv = cld(&r->invert) != 0;
    const int method = cld(&r->method);
    const int pl = cld(&r->pre_len), po = cld(&r->pre_off);
    for (int i0 = 0; i0 < cnt; i0 += WAVE) {
      const int i = i0 + lane;
      const bool act = i < cnt;
      const int f = act ? (int)L.list[wave][i] : 0;
      const bool inv = pinv ^ (L.fl[f] != 0);  // (:91-96)
      const LaneBits BN{&L.bn[f], MW, false}, BI{&L.bi[f], MW, false};
      const LaneBits& B = inv ? BI : BN;
      const int nb = L.nbits[inv ? 1 : 0][f];
      McOut o{0, 0, 0, 0, 0, 0, 0, 0};
      if (act) {
        const LaneBits DM{B.base, MW, true};  // mc2dmc(lh/hl) view for Funkbus
        o = mc_method(r, method, B, nb, nb, DM);
        int rk = 0;
        if (o.rc == -1) { rk = SDX_RAISE_TYPE; o.rc = 0; }
        if (o.rc == -2) { rk = SDX_RAISE_VALUE; o.rc = 0; }
        if (rk) atomicMin(&L.fraise[f], ((uint32_t)p << 4) | (uint32_t)rk);  // the first raising protocol
      }
      const bool has = o.rc == 1;
      const uint64_t hm = ballot(has);
      if (!hm) continue;
      const int plen = has ? pl + o.len : 0;
      int incl = plen;  // inclusive scan over lanes
      for (int d = 1; d < WAVE; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
      }
      const int wtot = __shfl(incl, WAVE - 1);
      const int nnew = popc64(hm);
      uint32_t hb = 0, rb = 0;
      if (lane == 0) {
        hb = atomicAdd(&L.hcur, (uint32_t)wtot);
        rb = atomicAdd(&L.rcur, (uint32_t)nnew);
      }
      hb = (uint32_t)__shfl((int)hb, 0);
      rb = (uint32_t)__shfl((int)rb, 0);
      const bool fits = hb + (uint32_t)wtot <= (uint32_t)MC_BHEAP && rb + (uint32_t)nnew <= (uint32_t)MC_BREC;
      if (!fits) {
        if (lane == 0) L.ovf = 1u;
        continue;
      }
      if (has) {
        uint8_t* dst = &L.heap[hb + incl - plen];
        for (int k = 0; k < pl; k += 8) {  // 8 independent loads per step
          uint8_t c[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) c[j] = (k + j < pl) ? bv.str[po + k + j] : (uint8_t)0;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (k + j < pl) dst[k + j] = c[j];
        }
        mc_write(r, o, B, nb, nb, dst + pl);
        StageRec sr;
        sr.off = hb + (uint32_t)(incl - plen);
        sr.len = (uint16_t)plen;
        sr.proto = (uint16_t)p;
        sr.bitlen = 0;
        sr.msg = (uint8_t)f;
        sr.wave = 0;
        sr.rank = 0;
        L.rec[rb + lanes_below(hm)] = sr;
      }
    }
  }
  __syncthreads();
  // ---- block flush: records bucketed by frame, each frame's in protocol order (flush_tile's scheme)
  const int nr = (int)(L.rcur < (uint32_t)MC_BREC ? L.rcur : (uint32_t)MC_BREC);
  const int nh = (int)(((L.hcur < (uint32_t)MC_BHEAP ? L.hcur : (uint32_t)MC_BHEAP) + 15u) & ~15u);
  const bool bad = L.ovf != 0;
  // scratch in the (dead) bit rows: per frame the record count, bucket fill, base, wire sums; the
  // bucketed record indices
  uint32_t* cntm = reinterpret_cast<uint32_t*>(L.bn);
  uint32_t* fill = cntm + 256;
  uint32_t* mbase = fill + 256;
  uint32_t* wtot = mbase + 256;      // [4] per wave totals of the scan, [4..5] rbase / hbase, [6] st
  unsigned long long* wsum = reinterpret_cast<unsigned long long*>(L.bi);
  uint16_t* bidx = reinterpret_cast<uint16_t*>(wsum + 256);
  static_assert(4 * (3 * 256 + 8) <= (int)sizeof(L.bn) && 8 * 256 + 2 * MC_BREC <= (int)sizeof(L.bi), "flush scratch");
  const bool raised = L.fraise[tid] != MC_NORAISE;
  cntm[tid] = 0;
  fill[tid] = 0;
  wsum[tid] = 0ull;
  __syncthreads();
  if (!bad)
    for (int k = tid; k < nr; k += 256) {
      const int f = L.rec[k].msg;
      if (L.fraise[f] == MC_NORAISE) atomicAdd(&cntm[f], 1u);
    }
  __syncthreads();
  // exclusive scan of the 256 counts (lane = frame): wave scans + the waves' totals
  const uint32_t c = (valid && !raised && !bad) ? cntm[tid] : 0u;
  uint32_t x = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) wtot[wave] = x;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; ++w) before += wtot[w];
  mbase[tid] = before + x - c;
  if (tid == 0) {
    const uint32_t nrec = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    uint32_t st = bad ? 2u : 0u, rbase = 0, hbase = 0;
    if (!bad) {
      rbase = atomicAdd(&out.cursor_dev[0], nrec);
      hbase = atomicAdd(&out.cursor_dev[1], (uint32_t)nh);
      if (rbase + nrec > out.rec_cap || hbase + (uint32_t)nh > out.heap_cap) {
        st = 3u;
        atomicOr(&out.cursor_dev[2], 1u);
      }
    } else {
      atomicOr(&out.cursor_dev[2], 2u);
    }
    wtot[4] = rbase;
    wtot[5] = hbase;
    wtot[6] = st;
    wtot[7] = nrec;
  }
  __syncthreads();
  const uint32_t rbase = wtot[4], hbase = wtot[5], st = wtot[6], nrec = wtot[7];
  const bool wx = out.wire_dev != nullptr;
  if (st == 0) {
    for (int k = tid; k < nr; k += 256) {
      const int f = L.rec[k].msg;
      if (L.fraise[f] != MC_NORAISE) continue;
      const uint32_t q = atomicAdd(&fill[f], 1u);
      bidx[mbase[f] + q] = (uint16_t)k;
    }
    __syncthreads();
    for (int j = tid; j < (int)nrec; j += 256) {
      const StageRec sr = L.rec[bidx[j]];
      const uint32_t b0 = mbase[sr.msg], b1 = b0 + cntm[sr.msg];
      uint32_t rk = 0;  // one record per (frame, protocol): its rank = the frame's records of lower protocols
      for (uint32_t q = b0; q < b1; ++q) rk += L.rec[bidx[q]].proto < sr.proto ? 1u : 0u;
      const int gf = blk * 256 + sr.msg;
      sdx_result o;
      o.payload_off = hbase + sr.off;
      o.payload_len = sr.len;
      o.proto = sr.proto;
      o.bit_length = 0;
      o.msg = (uint32_t)(b.sel_dev ? b.sel_dev[gf] : gf);
      out.rec_dev[rbase + b0 + rk] = o;
      if (wx) {
        const uint32_t xr = wire_class(bv, SDX_KIND_MC, sr.proto, &L.heap[sr.off], sr.len);
        if (out.xrec_dev) out.xrec_dev[rbase + b0 + rk] = xr;
        atomicAdd(&wsum[sr.msg], (unsigned long long)(((uint64_t)sr.len << 32) | wire_bytes_x(xr, sr.len)));
      }
    }
    uint4* hd = reinterpret_cast<uint4*>(out.heap_dev + hbase);
    const uint4* hs = reinterpret_cast<const uint4*>(L.heap);
    if ((((uintptr_t)hd) & 15u) == 0) {
      for (int k = tid; k < (nh >> 4); k += 256) hd[k] = hs[k];
    } else {
      for (int k = tid; k < nh; k += 256) out.heap_dev[hbase + k] = L.heap[k];
    }
  }
  if (wx) __syncthreads();  // wsum complete
  if (valid) {
    sdx_desc d;
    d.rec_begin = rbase + mbase[tid];
    const uint32_t rw = L.fraise[tid];
    if (rw != MC_NORAISE) { d.status = SDX_ST_RAISED; d.raise_kind = (uint8_t)(rw & 15u); d.n_rec = 0; }
    else if (st) { d.status = st == 2 ? SDX_ST_OVF_TILE : SDX_ST_OVF_OUT; d.raise_kind = 0; d.n_rec = 0; }
    else { d.status = SDX_ST_OK; d.raise_kind = 0; d.n_rec = (uint16_t)cntm[tid]; }
    out.desc_dev[msg] = d;
    if (wx) out.wire_dev[msg] = (rw == MC_NORAISE && st == 0) ? (uint64_t)wsum[tid] : 0ull;
  }
}

}  // namespace sdx
