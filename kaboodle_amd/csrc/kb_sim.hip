// kb_sim.hip — MI355X (gfx950) implementation of the Kaboodle SWIM round as a bulk-synchronous
// simulator over HBM-resident structure-of-arrays tables.  Exposes the C ABI of include/kaboodle_sim.h.
//
// Round pipeline, one HIP stream; the host reads 8 bytes per round (+20 when the
// broadcasts produced Join responses, to size the wave-0 outbox):
//   k_rebase (every 64 rounds)      stamp window shift                             
//   k_events / k_churn_*            Kaboodle::start/stop, churn                    src/lib.rs:136-183
//   k_alive_bits, k_truefp_*        running set and its fingerprint
//   k_bfail_prep(_lds), k_lat_mark  per-list facts of the Failed broadcasts
//   k_rowpass  <- dominant kernel   handle_incoming_broadcasts (Failed, Join) + ping_random_peer's
//                                   oldest-5 candidates, one pass per row        :256-311, :655-703
//   k_lat_sweep                     latency entries of Failed removals (track_latency)  :789-817
//   k_resp_wave / k_resp_node       maybe_send_known_peers_to_peer                 :356-392
//   k_tick_scan, k_tick_pre         maybe_broadcast_join + handle_suspected_peers  :228-251, :558-653
//   k_fold                          stale fingerprint checkpoints refolded         :71-83
//   k_tick_post                     ping target, handle_incoming_ping_requests     :655-703, :550-556
//   k_bcast_write                   the round's Join/Failed lists
//   waves: k_route (k_route_x, k_pack, exchange, k_route_recv when sharded), k_scan_*, k_scatter,
//          k_kp_small, k_kp_group, k_sort_inbox (+ KPR oversize probe), k_proc_fast, k_proc
//                                   handle_incoming_messages                       src/kaboodle.rs:394-548
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <array>
#include <algorithm>
#include <atomic>
#include <thread>
#include "kb_common.h"
#include "kb_wire.h"
#include "kb_round.h"
#include "kb_tick.h"
#include "kb_waves.h"
#include "kb_xfer.h"
#include "kb_sparse.h"

using namespace kb;

// Every launch of a round is tagged with one of these ids; with profiling on (kb_sim_set_profiling) it
// carries start/stop events on its own dispatch packet and kb_sim_kernel_breakdown reports the sums.
enum KId : int {
  KI_REBASE, KI_EVENTS, KI_CHURN_LEAVE, KI_CHURN_JOIN, KI_ALIVE_BITS, KI_TRUEFP_PART, KI_TRUEFP_FIN, KI_LOG_MARK,
  KI_LAT_MARK, KI_BFAIL_PREP, KI_ROWPASS, KI_LAT_SWEEP, KI_SCAN_TILES, KI_SCAN_APPLY, KI_SET_CAP, KI_RESP_WAVE,
  KI_RESP_NODE, KI_TICK_SCAN, KI_TICK_PRE, KI_FOLD, KI_FP_ROWS, KI_TICK_POST, KI_BCAST_WRITE, KI_ROUTE, KI_ROUTE_X,
  KI_XBOUND, KI_PACK, KI_ROUTE_RECV, KI_SCATTER, KI_SCATTER_FLAT, KI_KP, KI_SORTFAST, KI_PROC, KI_ROUND_END,
  KI_PROBE, KI_A3_EXACT, NKI
};
static const char* const KNAME[NKI] = {
  "k_rebase", "k_events", "k_churn_leave", "k_churn_join", "k_alive_bits", "k_truefp_part", "k_truefp_fin",
  "k_log_mark", "k_lat_mark", "k_bfail_prep", "k_rowpass", "k_lat_sweep", "k_scan_tiles", "k_scan_apply",
  "k_set_cap", "k_resp_wave", "k_resp_node", "k_tick_scan", "k_tick_pre", "k_fold", "k_fp_rows", "k_tick_post",
  "k_bcast_write", "k_route", "k_route_x", "k_xbound", "k_pack", "k_route_recv", "k_scatter", "k_scatter_flat",
  "k_kp", "k_sortfast", "k_proc", "k_round_end", "k_probe", "k_a3_exact"};
// the in-kernel algorithmic byte counter of a kernel (StatIdx), or -1
static int kbytes_stat(int kid) {
  switch (kid) {
    case KI_ROWPASS: return S_ROWB;
    case KI_FOLD: return S_FOLDB;
    case KI_RESP_WAVE: return S_RESPB;
    case KI_PROC: return S_PROCB;
    default: return -1;
  }
}

// ================================================================================================
// Exclusive scan over up to 4 arrays of length n (+ optional compaction of indices j with in[0][j] != 0),
// two fully parallel passes over 1024-element tiles: per-tile sums, then per-tile offsets + local scan.
// ================================================================================================
struct ScanArgs {
  const uint32_t* in[4]; uint32_t* out[4]; int narr; uint32_t n;
  uint32_t* totals;   // device, narr values (+ list count at totals[4] when list != null)
  uint32_t* list; uint32_t* list_count; uint32_t list_base;   // list entries are j + list_base
  uint32_t list_or3;  // list flag: in[0][j] != 0, or also in[3][j] != 0 when set
  uint32_t addc[4];   // constant added to every element of array q before scanning
  uint32_t* tiles;    // workspace [5 * ntiles]
  uint32_t ntiles;
};
__device__ inline uint32_t scan_val(const ScanArgs& a, int q, uint32_t j) {
  if (q == 4) return a.in[0][j] != 0 || (a.list_or3 && a.in[3][j] != 0);
  return (a.in[q] ? a.in[q][j] : 0) + a.addc[q];
}
__global__ __launch_bounds__(1024) void k_scan_tiles(ScanArgs a) {
  __shared__ uint32_t red[5][16];
  const uint32_t j = blockIdx.x * 1024 + threadIdx.x;
  const int nq = a.list ? 5 : a.narr;
  for (int q = 0; q < 5; ++q) {
    if (q >= a.narr && !(q == 4 && a.list)) continue;
    uint32_t v = j < a.n ? scan_val(a, q, j) : 0;
    v = wave_sum(v);
    if (lane() == 0) red[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 5 && (threadIdx.x < (uint32_t)a.narr || (threadIdx.x == 4 && a.list))) {
    uint32_t t = 0;
    for (int w = 0; w < 16; ++w) t += red[threadIdx.x][w];
    a.tiles[threadIdx.x * a.ntiles + blockIdx.x] = t;
  }
  (void)nq;
}
__global__ __launch_bounds__(1024) void k_scan_apply(ScanArgs a) {
  __shared__ uint32_t base[5], red[5][16], wpre[5][16];
  const uint32_t tile = blockIdx.x, t = threadIdx.x;
  const uint32_t j = tile * 1024 + t;
  for (int q = 0; q < 5; ++q) {
    const bool on = q < a.narr || (q == 4 && a.list);
    uint32_t s = 0;
    if (on) for (uint32_t k = t; k < tile; k += 1024) s += a.tiles[q * a.ntiles + k];
    s = wave_sum(s);
    if (lane() == 0) red[q][t >> 6] = s;
  }
  __syncthreads();
  if (t < 5) { uint32_t s = 0; for (int w = 0; w < 16; ++w) s += red[t][w]; base[t] = s; }
  __syncthreads();
  uint32_t v[5], ex[5];
  for (int q = 0; q < 5; ++q) {
    const bool on = q < a.narr || (q == 4 && a.list);
    v[q] = (on && j < a.n) ? scan_val(a, q, j) : 0;
    ex[q] = wave_excl(v[q]);
    const uint32_t tot = wave_sum(v[q]);
    if (lane() == 0) wpre[q][t >> 6] = tot;
  }
  __syncthreads();
  if (t < 5) { uint32_t run = 0; for (int w = 0; w < 16; ++w) { uint32_t x = wpre[t][w]; wpre[t][w] = run; run += x; } }
  __syncthreads();
  for (int q = 0; q < a.narr; ++q) if (j < a.n) a.out[q][j] = base[q] + wpre[q][t >> 6] + ex[q];
  if (a.list && j < a.n && v[4]) a.list[base[4] + wpre[4][t >> 6] + ex[4]] = j + a.list_base;
  if (tile == gridDim.x - 1 && t == 1023) {
    for (int q = 0; q < a.narr; ++q) a.totals[q] = base[q] + wpre[q][15] + ex[q] + v[q];
    if (a.list) { const uint32_t c = base[4] + wpre[4][15] + ex[4] + v[4]; a.totals[4] = c; if (a.list_count) *a.list_count = c; }
  }
}


// crc0 fold of every member pattern of every 8-id half block (uniform identity length)
__global__ void k_build_htab(Dev d) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)(d.W / 8) * 256;
  if (k >= total) return;
  const uint32_t h = (uint32_t)(k >> 8), m = (uint32_t)(k & 255);
  uint32_t raw = 0;
  for (uint32_t t = 0; t < 8; ++t) {
    const uint32_t j = h * 8 + t;
    if (((m >> t) & 1u) && j < d.C) raw = multmodp(d.zpow[1], raw) ^ d.cseg[j];
  }
  d.htab[k] = raw;
}
// (also hands the wave-0 scan totals to the host: tot[0..4] -> host-mapped hpin[0..4], then the
// sequence number the host polls for)
__global__ void k_set_cap(Dev d, const uint32_t* nresp, uint32_t* cap, uint32_t* cnt, const uint32_t* tot, uint32_t* hpin,
                          uint32_t seq, uint32_t* rest2n) {
  const uint32_t i = d.lo + blockIdx.x * blockDim.x + threadIdx.x;
  if (i < d.hi) { cap[i] = nresp[i] + TICK_MAX; cnt[i] = nresp[i]; }
  if (blockIdx.x == 0 && threadIdx.x == 0) { d.ctr[C_RESTN] = 0; *rest2n = 0; pin_publish(hpin, tot, 5, seq); }
}
// device values -> the host's mapped pinned buffer, then the sequence number it polls for (sharded
// hand-offs of all-gathered counts)
__global__ void k_publish(const uint32_t* v, uint32_t n, uint32_t* hpin, uint32_t seq) {
  if (blockIdx.x == 0 && threadIdx.x == 0) pin_publish(hpin, v, n, seq);
}
__global__ void k_init_nodes(Dev d, uint32_t n0) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.C) return;
  if (local(d, i)) { d.last_bcast[i] = NONE_ROUND; d.a3cur[i] = i; }
  d.start_round[i] = NONE_ROUND;
  if (i < n0) node_start(d, i, 0);
}
// rows of the initial members (the local ones): every initial member known and "ancient", self now
__global__ void k_init_converged_rows(Dev d, uint32_t n0) {
  const uint32_t wpr = d.W / 16;
  const uint32_t r0 = d.lo, r1 = n0 < d.hi ? n0 : d.hi;
  const size_t words = r1 > r0 ? (size_t)(r1 - r0) * wpr : 0;
  uint4* p = reinterpret_cast<uint4*>(d.stamp);
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < words; k += (size_t)gridDim.x * blockDim.x) {
    const uint32_t i = r0 + (uint32_t)(k / wpr), c = (uint32_t)(k % wpr);
    uint32_t w4[4];
    for (int q = 0; q < 4; ++q) {
      uint32_t y = 0;
      for (int t = 0; t < 4; ++t) {
        const uint32_t j = c * 16 + q * 4 + t;
        uint32_t b = j < n0 ? ST_ANCIENT : 0;
        if (j == i) b = enc(0, 0);
        y |= b << (8 * t);
      }
      w4[q] = y;
    }
    p[(size_t)i * wpr + c] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
  }
  const size_t bw = r1 > r0 ? (size_t)(r1 - r0) * d.NWR : 0;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < bw; k += (size_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)(k % d.NWR);
    uint32_t x = 0;
    if (w * 32 + 32 <= n0) x = 0xFFFFFFFFu;
    else if (w * 32 < n0) x = (1u << (n0 - w * 32)) - 1u;
    d.bits[(size_t)r0 * d.NWR + k] = x;
  }
}
__global__ void k_init_converged_nodes(Dev d, uint32_t n0) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.C) return;
  const bool loc = local(d, i);
  if (loc) { d.last_bcast[i] = NONE_ROUND; d.a3cur[i] = i; }
  d.start_round[i] = NONE_ROUND;
  if (i >= n0) return;
  d.alive[i] = 1; d.start_round[i] = 0;
  if (loc) { d.dirty[i] = 1; d.n[i] = n0; d.last_bcast[i] = -1000; d.paq_n[i] = 0; d.sdirty[i] = ~0ull; }
}
__global__ void k_mark_all_dirty(Dev d) {
  const uint32_t i = d.lo + blockIdx.x * blockDim.x + threadIdx.x;
  if (i < d.hi) { d.dirty[i] = 1; d.sdirty[i] = ~0ull; }
}
__global__ __launch_bounds__(64) void k_fp_one(Dev d, uint32_t i) {
  __shared__ uint32_t ztab[ZT * 128];
  load_ztab(d, ztab);
  if (!d.dirty[i]) return;
  const uint32_t f = wave_fp(d, ztab, i, 0);
  if (lane() == 0) { d.fp[i] = f; d.dirty[i] = 0; }
}
__global__ __launch_bounds__(256) void k_fp_all(Dev d) {
  __shared__ uint32_t ztab[ZT * 128];
  load_ztab(d, ztab);
  const uint32_t i = d.lo + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= d.hi || !d.dirty[i]) return;
  const uint32_t f = wave_fp(d, ztab, i, 0);
  if (lane() == 0) { d.fp[i] = f; d.dirty[i] = 0; }
}

// ================================================================================================
// Host side
// ================================================================================================
static thread_local std::string g_err;
static void seterr(const std::string& s) { g_err = s; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { seterr(std::string(#x) + ": " + hipGetErrorString(e_)); return KB_IO_ERROR; } } while (0)

// zeroed device memory, the zeroing complete on return (hipMemset runs on the null stream, which does not order
// with the simulator's non-blocking stream: a buffer regrown mid-round could be zeroed after a kernel wrote it)
template <class T> static hipError_t dalloc(T** p, size_t n) {
  hipError_t e = hipMalloc((void**)p, sizeof(T) * (n ? n : 1));
  if (e == hipSuccess) e = hipMemset(*p, 0, sizeof(T) * (n ? n : 1));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}

// the Join broadcasts of external peers (kb_sim_inject) merged into the round's Join list in sender
// order, as the tick's Joins would be (one per sender, bseq 0; pad = the sender's partition group when the list
// carries it, pgroups > 1)
static int merge_ext_joins(hipStream_t st, BCast* list, uint32_t* n, std::vector<uint32_t>& joins, uint32_t pgroups, uint32_t C) {
  if (joins.empty()) return KB_OK;
  std::vector<BCast> v(*n);
  if (*n) HIPCHK(hipMemcpyAsync(v.data(), list, sizeof(BCast) * *n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (const uint32_t x : joins) {
    const uint32_t g = pgroups > 1 ? (uint32_t)((uint64_t)x * pgroups / C) : 0u;
    const auto at = std::upper_bound(v.begin(), v.end(), x, [](uint32_t a, const BCast& b) { return a < b.sender; });
    v.insert(at, BCast{x, x, 0, g});
  }
  HIPCHK(hipMemcpyAsync(list, v.data(), sizeof(BCast) * v.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  *n = (uint32_t)v.size();
  joins.clear();
  return KB_OK;
}

static uint32_t h_crc_table[256];
static void h_crc_init() {
  for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1; h_crc_table[i] = c; }
}
static uint32_t h_crc_update(uint32_t reg, const uint8_t* p, size_t n) {
  for (size_t k = 0; k < n; ++k) reg = h_crc_table[(reg ^ p[k]) & 0xFF] ^ (reg >> 8);
  return reg;
}
static uint32_t h_xpow8(uint64_t n) {
  uint32_t res = 0x80000000u, sq = 0x00800000u;
  while (n) { if (n & 1) res = multmodp(sq, res); sq = multmodp(sq, sq); n >>= 1; }
  return res;
}

// Event streams (src/events.rs:57-100): the net difference between `node`'s membership bitset and
// the observer's snapshot.  One workgroup walks the row 1024 words at a time; the ids of each pass
// are compacted in ascending order by a wave scan plus a scan over the 16 wave totals.
// out = [discovered: C][departed: C][n_discovered, n_departed, n_known]
__global__ __launch_bounds__(1024) void k_events_diff(const uint32_t* __restrict__ row,
                                                      const uint32_t* __restrict__ snap, uint32_t C,
                                                      uint32_t* __restrict__ out) {
  __shared__ uint32_t wa[16], wr[16], base[2], known;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6, nw = (C + 31) / 32;
  uint32_t* add = out;
  uint32_t* rem = out + C;
  if (t == 0) { base[0] = 0; base[1] = 0; known = 0; }
  __syncthreads();
  uint32_t kn = 0;
  for (uint32_t w0 = 0; w0 < nw; w0 += 1024) {
    const uint32_t w = w0 + t;
    uint32_t cur = 0, old = 0;
    if (w < nw) {
      const uint32_t valid = (C - w * 32 >= 32) ? ~0u : ((1u << (C - w * 32)) - 1u);
      cur = row[w] & valid;
      old = snap[w] & valid;
    }
    const uint32_t a = cur & ~old, r = old & ~cur;
    kn += __popc(cur);
    uint32_t pa = __popc(a), pr = __popc(r);
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t xa = __shfl_up(pa, o, 64), xr = __shfl_up(pr, o, 64);
      if (lane >= (uint32_t)o) { pa += xa; pr += xr; }
    }
    if (lane == 63) { wa[wv] = pa; wr[wv] = pr; }
    __syncthreads();
    uint32_t oa = base[0] + pa - __popc(a), orr = base[1] + pr - __popc(r);
    for (uint32_t k = 0; k < wv; ++k) { oa += wa[k]; orr += wr[k]; }
    for (uint32_t m = a; m; m &= m - 1) add[oa++] = w * 32 + __ffs(m) - 1;
    for (uint32_t m = r; m; m &= m - 1) rem[orr++] = w * 32 + __ffs(m) - 1;
    __syncthreads();
    if (t == 1023) { base[0] = oa; base[1] = orr; }
    __syncthreads();
  }
  for (int o = 32; o > 0; o >>= 1) kn += __shfl_down(kn, o, 64);
  if (lane == 0) atomicAdd(&known, kn);
  __syncthreads();
  if (t == 0) { out[2 * C] = base[0]; out[2 * C + 1] = base[1]; out[2 * C + 2] = known; }
}
// the drain: the snapshot becomes the current row
__global__ __launch_bounds__(256) void k_events_commit(const uint32_t* __restrict__ row, uint32_t* __restrict__ snap,
                                                       uint32_t nw) {
  const uint32_t w = blockIdx.x * 256 + threadIdx.x;
  if (w < nw) snap[w] = row[w];
}
// one node's latencies out of the peer-major table (peer_states)
__global__ __launch_bounds__(256) void k_lat_column(Dev d, uint32_t node, uint16_t* out) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j < d.C) out[j] = *lat_at(d, node, j);
}

namespace kb { struct SpSim; }
enum CensusMs { CM_VIEW, CM_RECIP, CM_CLASSES, CM_LAT, CM_AGE, CM_DELTA, CM_ISLANDS, CM_GAPS, CM_HOLDERS, CM_N };   // kb_sim::census_ms (kb_censusframe.h)

struct kb_sim {
  kb_config cfg;
  SpSim* sp = nullptr;                 // KB_VARIANT_SPARSE_ROWS: the sparse-row engine answers every call
  Dev d;
  int device;
  hipStream_t st;
  // side stream: kernels off the round's critical path (the running set's fingerprint, the latency sweep)
  // run beside it, forked from and joined back into st by events
  hipStream_t st2 = nullptr;
  // third stream: the Join responses of the responders A2 cannot touch, beside the tick (side work 4)
  hipStream_t st3 = nullptr;
  hipEvent_t ev_fork[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, ev_join[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // side work 0-4
  uint32_t C, W, S;                    // capacity, row stride, row-sweep column splits
  // row shard: this handle holds rows [lo, hi) of the mesh, R = hi - lo
  uint32_t lo, hi, R;
  int rank, world;
  Xfer* xf;                            // null: unsharded (no exchange at all)
  bool in_group;                       // a shard of a kb_sim_create_local group
  std::vector<void*> allocs;           // device memory owned by this handle
  int32_t round;
  bool probed = false;                 // kb_sim_debug_fold wrote rows of its own: the handle steps no more
  std::vector<uint8_t> h_ident, h_idlen;
  std::vector<uint8_t> h_pend; std::vector<int16_t> h_pendlen;   // identity set on a stopped instance that ran:
                                                                 // its next address takes it (-1: none)
  std::vector<uint8_t> h_moved;                                  // the instance bound here restarted elsewhere
  std::vector<uint8_t> h_idset;                                  // identity set on a never-bound address (d.idset)
  std::vector<uint8_t> h_ext;                                    // external peers (d.ext)
  // external peers: records injected for the next round's wave 0, records exported not drained
  size_t n_ext = 0;
  std::vector<XRec> inj; std::vector<uint32_t> inj_ids;
  std::vector<uint32_t> inj_join;                    // external peers' Join broadcasts for the next round
  XRec* d_inj = nullptr; uint32_t* d_inj_ids = nullptr; size_t d_inj_cap = 0, d_inj_ids_cap = 0;
  std::vector<kb_unicast> xq; std::vector<uint32_t> xq_ids;
  std::vector<Event> events;
  uint32_t* rpack = nullptr; uint32_t* rpack_in = nullptr;       // a restart's packed row (send / receive)
  // discovery: Probes queued for the next round, those delivered this round, responses not yet drained
  std::vector<kb_wire_addr> probe_q, probes;
  std::vector<kb_probe_response> presp;
  uint2* d_presp = nullptr; uint32_t* d_presp_n = nullptr; size_t presp_cap = 0;
  OutBuf ob[2];
  WaveCtl wc;
  uint32_t msg_cap, pay_cap;
  BCast* bfail; BCast* bjoin;          // the round's broadcast lists (whole mesh, sender order)
  BCast* bfail_loc; BCast* bjoin_loc;  // sharded: this shard's part, before the all-gather
  uint32_t nf, nj;
  uint32_t ucap = 0;                   // Join-response union slots (sharded meshes, kb_waves.h UCAP)
  uint32_t host_paths = 0;             // PATH_* bits of variants chosen at a launch (kb_sim_debug_paths ORs them in)
  uint64_t xbytes_cross = 0, xbytes_all = 0;   // bytes this shard's waves sent to other shards / to every shard
  BcastSlots bs;
  uint32_t* join_off; uint32_t* fail_off;
  uint32_t* scan_tot; uint32_t* scan_tiles;
  unsigned long long* newmask; unsigned long long* respmask; size_t mask_words;
  unsigned long long* newmask_base; unsigned long long* respmask_base;
  uint32_t* nresp; uint32_t* paysum; uint32_t* nbase; uint32_t* resp_off;
  uint32_t* resp_nodes; uint32_t* bf_gid; uint8_t* bf_dep;
  uint32_t* slow;                      // the nodes of a wave k_proc_fast leaves to k_proc; in the tick, A2's node list
  uint32_t* rest[2] = {nullptr, nullptr};   // the responders k_resp_wave leaves to k_resp_node: phases 0 and 1, phase 2
  uint32_t* rest2n = nullptr;          // phase 2's list counter (phases 0 and 1: d.ctr[C_RESTN])
  uint8_t* a2flag = nullptr;           // [R] k_tick_scan: 1 for the nodes it listed for A2
  uint32_t* defer = nullptr;           // split wave 0: the BIG KnownPeers groups' destinations, handled after the join
  uint32_t* w0ctr = nullptr;           // its counters (W0_*: deferred nodes, k_proc's tickets)
  uint16_t* lat_col;                   // [C] one node's latencies (peer_states), track_latency only
  uint32_t* fnamed;                    // [NWR] peers named by the round's Failed list (track_latency only)
  uint32_t* resp_scratch; size_t resp_scratch_words;   // k_resp_node's HBM scratch, grown on demand
  RowOut ro;
  Event* d_events; size_t events_cap;
  // sharded waves: send side (xs), all-gathered counts, receive buffers (grown on demand)
  XState xs;
  uint32_t* xall; unsigned long long* xstats;
  std::vector<uint32_t> h_xall;
  Msg* rmsg; uint32_t* rpay; uint8_t* rstatus; uint32_t* rinbox; uint32_t* rkp;
  size_t rmsg_cap, rpay_cap;
  double round_ms;                     // the whole round: markers on the stream, read back like the kernels'
  uint32_t* rr = nullptr;              // [3] the round's {Join, Failed, error} on the device (sharded gather)
  uint64_t round_launches, bj_total, bf_total;
  // per-kernel profile (kb_sim_kernel_breakdown): with prof_on every launch carries start/stop events
  // on its own dispatch packet; a round's records are read back during the next round's final wait
  // (the host is idle then), the last round's on query
  struct KRec { int16_t kid, wave; hipEvent_t a, b; };
  int prof_level = 1;                  // 0 none, 1 the kernels with byte counters, 2 every launch
  bool capturing = false;              // inside a HIP graph capture: launches carry no events
  int cur_wave = -1;                   // the delivery wave being launched (-1: outside the window)
  std::vector<hipEvent_t> ev_free;
  std::vector<KRec> krec;
  double k_ms[NKI] = {};
  double k_wms[NKI][KB_WAVE_SLOTS] = {};
  uint64_t k_n[NKI] = {};
  uint64_t k_bytes0[NSTAT] = {};
  uint64_t host_syncs = 0;             // host waits on the device (stream syncs, pinned hand-offs) since creation
  uint32_t ncu = 256;
  uint32_t* cs_buf = nullptr;          // the census's scratch (kb_census.h), allocated by the first census
  uint32_t* rc_buf = nullptr;          // the reciprocity census's scratch (kb_recip.h), allocated by its first call
  uint2* rc_pairs = nullptr; size_t rc_pairs_cap = 0;  // its pair list, grown on demand
  char* fc_buf = nullptr; size_t fc_cap = 0;   // the class census's scratch (kb_classes.h), bytes; grown on demand, held by
                                               // the engine whose stream runs the census (a group's first shard)
  double census_ms[CM_N] = {};         // device time of the last census of each kind, on the handle that was asked
  bool debug_waves = false;
  size_t lds_per_cu = 65536;
  // kb_sim_create_local: a façade over `world` in-process shards (one host thread each per step)
  std::vector<kb_sim*> shards;
  LocalHub* hub;
  // event observers (kb_sim_watch): a watched node and the device snapshot of its membership bitset
  // at the last drain, plus the fingerprint last reported for it
  std::vector<uint32_t> watch_node, watch_fp;
  std::vector<uint32_t*> watch_snap;
  uint32_t* ev_out = nullptr;          // [2*C + 4]: discovered ids, departed ids, counters
  uint32_t* h_pin = nullptr;           // [16] pinned host memory, mapped: per-round results written by kernels
  uint32_t* d_pin = nullptr;           //      its device address
  uint32_t pin_seq = 0;                // hand-off sequence number (h_pin[PIN_SEQ])
  uint64_t occ_key = ~0ull; int occ_val = 0;   // row-pass occupancy query, cached per launch shape
  // the unsharded receive window as a HIP graph (launch_waves), re-captured when buffers are regrown
  bool graph_on = false;               // env KB_WAVE_GRAPH=1
  hipGraph_t wave_graph = nullptr; hipGraphExec_t wave_exec = nullptr;
  uint64_t buf_gen = 0, wave_gen = ~0ull;
  uint32_t* lc_buf = nullptr;          // the latency census's scratch (kb_latcensus.h), allocated by its first call
  double sn_ms = 0;                    // device time of the last snapshot pack, or of the restore that made the handle
  // the view-delta census (kb_delta.h): this handle's baseline, taken by kb_sim_delta_mark, and the pass's scratch
  uint32_t* dl_base = nullptr;         // [R][W/32] the rows' member bits at the mark (null: no baseline)
  uint8_t* dl_run = nullptr;           // [C] the running set at the mark
  int32_t dl_round = 0;                // the round of the mark
  uint32_t* dl_buf = nullptr;          // the scratch, allocated by the first delta census
  uint32_t* is_buf = nullptr;          // the island census's scratch (kb_islands.h), allocated by its first call
  // the gap list and the holders query (kb_gaps.h), on the handle whose stream runs them (a group's first shard)
  uint32_t* gp_buf = nullptr;          // the gap list's scratch, allocated by its first call
  uint32_t* gp_list = nullptr; size_t gp_list_cap = 0;   // the listed elements of either call, grown on demand
  char* hd_buf = nullptr; size_t hd_cap = 0;   // the holders query's scratch, bytes; grown with the number of ids asked
};

// allocation of this handle's device memory; row tables hold the local rows only and their pointer
// is biased by -lo rows so kernels index them with global ids
template <class T> static hipError_t talloc(kb_sim* s, T** p, size_t n) {
  hipError_t e = dalloc(p, n);
  if (e == hipSuccess) s->allocs.push_back((void*)*p);
  return e;
}
template <class T> static hipError_t eng_alloc(kb_sim* s, T** p, size_t n) { return talloc(s, p, n); }   // kb_roundframe.h's hooks
static const char* eng_alloc_what(kb_sim*) { return "device allocation failed: "; }
template <class T> static T* bias(T* base, size_t per_row, uint32_t lo) {
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) - sizeof(T) * per_row * lo);
}
template <class T> static hipError_t ralloc(kb_sim* s, T** p, size_t per_row) {
  T* base = nullptr;
  hipError_t e = talloc(s, &base, per_row * s->R);
  *p = bias(base, per_row, s->lo);
  return e;
}
template <class T> static T* L(const kb_sim* s, T* p) { return p + s->lo; }   // biased row table -> local base

// ---- launches and their profile ------------------------------------------------------------------
static void prof_events(kb_sim* s, int kid, hipEvent_t* a, hipEvent_t* b) {
  *a = *b = nullptr;
  // level 1 times the once-per-round kernels with byte counters only: k_proc's eight launches a round
  // would add ≈ 0.05 ms of event dispatch overhead to the round (tools/ev_cost.py)
  if (s->capturing || s->prof_level <= 0 || (s->prof_level == 1 && (kbytes_stat(kid) < 0 || kid == KI_PROC))) return;
  hipEvent_t e[2];
  for (int k = 0; k < 2; ++k) {
    if (!s->ev_free.empty()) { e[k] = s->ev_free.back(); s->ev_free.pop_back(); }
    else if (hipEventCreate(&e[k]) != hipSuccess) { if (k) s->ev_free.push_back(e[0]); return; }
  }
  *a = e[0]; *b = e[1];
  const int w = s->cur_wave < 0 ? -1 : (s->cur_wave < KB_WAVE_SLOTS ? s->cur_wave : KB_WAVE_SLOTS - 1);
  s->krec.push_back(kb_sim::KRec{(int16_t)kid, (int16_t)w, e[0], e[1]});
}
// every kernel of the round is launched through here: the dispatch packet itself records the events
template <typename F, typename... Args>
static void klaunch_on(kb_sim* s, hipStream_t stream, int kid, F kern, dim3 grid, dim3 block, uint32_t lds, Args... args) {
  hipEvent_t a, b;
  prof_events(s, kid, &a, &b);
  hipExtLaunchKernelGGL(kern, grid, block, lds, stream, a, b, 0, args...);
}
template <typename F, typename... Args>
static void klaunch(kb_sim* s, int kid, F kern, dim3 grid, dim3 block, uint32_t lds, Args... args) {
  klaunch_on(s, s->st, kid, kern, grid, block, lds, args...);
}
// fork side work k onto st2 after everything st has queued so far / join it back into st
static hipStream_t side_stream(kb_sim* s, int k) { return k == 4 ? s->st3 : s->st2; }   // side work 4 has the third stream
static void side_fork(kb_sim* s, int k) { (void)hipEventRecord(s->ev_fork[k], s->st); (void)hipStreamWaitEvent(side_stream(s, k), s->ev_fork[k], 0); }
static void side_done(kb_sim* s, int k) { (void)hipEventRecord(s->ev_join[k], side_stream(s, k)); }
static void side_join(kb_sim* s, int k) { (void)hipStreamWaitEvent(s->st, s->ev_join[k], 0); }
// fold the first n records (complete: their round has ended) into the per-kernel sums
static void prof_resolve(kb_sim* s, size_t n) {
  n = std::min(n, s->krec.size());
  for (size_t k = 0; k < n; ++k) {
    const kb_sim::KRec& q = s->krec[k];
    float ms = 0;
    hipError_t e = hipEventElapsedTime(&ms, q.a, q.b);
    if (e == hipErrorNotReady) {                      // still pending (an earlier round's tail): wait for it
      (void)hipGetLastError();                        // rather than drop the record and recycle live events
      (void)hipEventSynchronize(q.b);
      e = hipEventElapsedTime(&ms, q.a, q.b);
    }
    if (e == hipSuccess) {
      if (q.kid == NKI) { s->round_ms += ms; s->round_launches++; }          // the whole round
      else {
        s->k_ms[q.kid] += ms; s->k_n[q.kid]++;
        if (q.wave >= 0) s->k_wms[q.kid][q.wave] += ms;
      }
    }
    s->ev_free.push_back(q.a); s->ev_free.push_back(q.b);
  }
  s->krec.erase(s->krec.begin(), s->krec.begin() + n);
}

static ScanArgs scan_args(kb_sim* s, uint32_t n, uint32_t* totals) {
  ScanArgs a; memset(&a, 0, sizeof a); a.n = n; a.totals = totals;
  a.tiles = s->scan_tiles; a.ntiles = (n + 1023) / 1024; return a;
}
static void launch_scan(kb_sim* s, const ScanArgs& a) {
  if (!a.n) return;
  klaunch(s, KI_SCAN_TILES, k_scan_tiles, dim3(a.ntiles), dim3(1024), 0, a);
  klaunch(s, KI_SCAN_APPLY, k_scan_apply, dim3(a.ntiles), dim3(1024), 0, a);
}

extern "C" void kb_config_default(kb_config* c) {
  memset(c, 0, sizeof *c);
  c->abi_version = KB_ABI_VERSION; c->capacity = 1024; c->initial_nodes = 1024; c->init_mode = KB_INIT_JOIN;
  c->seed = 1; c->fault_end_round = -1; c->max_waves = 8; c->failed_mode = KB_FAILED_SIM_SENDER; c->device = -1;
}
extern "C" const char* kb_last_error(void) { return g_err.c_str(); }
extern "C" int kb_format_addr(uint32_t id, char* buf, size_t cap) {
  char tmp[32];
  int len = snprintf(tmp, sizeof tmp, "10.100.100.%u:%u", 100u + id / 50000u, 10000u + id % 50000u);
  if (!buf || cap < (size_t)len + 1) return KB_INVALID_ARGUMENT;
  memcpy(buf, tmp, (size_t)len + 1);
  return KB_OK;
}
static void default_identity(uint32_t id, uint32_t len, uint8_t* out) {
  for (uint32_t k = 0; k < len; ++k) out[k] = (uint8_t)('a' + ((id * 31u + k * 7u) % 26u));
}

// (re)upload per-id segment CRCs, the Z tables and the half-block tables
static int upload_segments(kb_sim* s) {
  const uint32_t C = s->C;
  std::vector<uint32_t> cseg(C), segmul(C), seglen(C);
  bool uniform = true;
  uint32_t xp[ADDR_LEN + MAXID + 1];                 // x^(8 len) per segment length
  for (uint32_t l = 0; l <= ADDR_LEN + MAXID; ++l) xp[l] = h_xpow8(l);
  for (uint32_t j = 0; j < C; ++j) {
    char a[32]; kb_format_addr(j, a, sizeof a);
    uint32_t reg = h_crc_update(0, (const uint8_t*)a, ADDR_LEN);
    reg = h_crc_update(reg, &s->h_ident[(size_t)j * MAXID], s->h_idlen[j]);
    cseg[j] = reg; seglen[j] = ADDR_LEN + s->h_idlen[j]; segmul[j] = xp[seglen[j]];
    if (s->h_idlen[j] != s->cfg.id_len) uniform = false;
  }
  s->d.uniform = uniform ? 1 : 0;
  s->d.L = ADDR_LEN + s->cfg.id_len;
  const uint32_t Z = h_xpow8(s->d.L);
  std::vector<uint32_t> zpow(std::max<uint32_t>(C + 2, 17));     // the tables below need Z^0..Z^16
  zpow[0] = 0x80000000u;
  for (size_t k = 1; k < zpow.size(); ++k) zpow[k] = multmodp(Z, zpow[k - 1]);
  std::vector<uint32_t> ztab(17 * 128);
  for (uint32_t c = 0; c <= 16; ++c)
    for (uint32_t k = 0; k < 8; ++k)
      for (uint32_t v = 0; v < 16; ++v) ztab[c * 128 + k * 16 + v] = multmodp(zpow[c], v << (4 * k));
  HIPCHK(hipMemcpy(s->d.cseg, cseg.data(), 4ull * C, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(s->d.segmul, segmul.data(), 4ull * C, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(s->d.seglen, seglen.data(), 4ull * C, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(s->d.zpow, zpow.data(), 4ull * (C + 2), hipMemcpyHostToDevice));
  {
    std::vector<uint32_t> zf(C + 2);
    for (uint32_t k = 0; k < C + 2; ++k) zf[k] = multmodp(zpow[k], 0xFFFFFFFFu);
    HIPCHK(hipMemcpy(s->d.zfin, zf.data(), 4ull * (C + 2), hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemcpy(s->d.ztab, ztab.data(), 4ull * ztab.size(), hipMemcpyHostToDevice));
  std::vector<uint32_t> zb(ZB);
  for (uint32_t c = 0; c < 9; ++c)
    for (uint32_t k = 0; k < 4; ++k)
      for (uint32_t v = 0; v < 256; ++v) zb[c * 1024 + k * 256 + v] = multmodp(zpow[c], v << (8 * k));
  HIPCHK(hipMemcpy(s->d.zbtab, zb.data(), 4ull * zb.size(), hipMemcpyHostToDevice));
  const size_t hn = (size_t)(s->W / 8) * 256;
  k_build_htab<<<(unsigned)((hn + 255) / 256), 256>>>(s->d);
  HIPCHK(hipDeviceSynchronize());
  return KB_OK;
}

#include "kb_roundframe.h"
#include "kb_sparse_host.h"

// a handle answered by the sparse-row engine: the whole mesh (xf null) or one row shard of it (owns xf)
static int sp_wrap(const kb_config* cfg, int rank, int world, Xfer* xf, kb_sim** out) {
  if (cfg->capacity == 0 || cfg->capacity > 7800000u || cfg->initial_nodes > cfg->capacity || cfg->id_len > MAXID ||
      cfg->max_waves == 0 || cfg->max_waves > 64) { seterr("config out of range"); delete xf; return KB_INVALID_ARGUMENT; }
  SpSim* sp = nullptr;
  const int rc = sp_create(cfg, rank, world, xf, &sp);
  if (rc) return rc;
  kb_sim* s = new kb_sim();
  s->cfg = *cfg; s->C = cfg->capacity; s->sp = sp; s->device = sp->device; s->rank = rank; s->world = world;
  s->lo = sp->lo; s->hi = sp->hi; s->R = sp->R;
  *out = s;
  return KB_OK;
}

static void free_all(kb_sim* s) {
  for (void* p : s->allocs) (void)hipFree(p);
  s->allocs.clear();
}
static void destroy_shard(kb_sim* s) {
  (void)hipSetDevice(s->device);
  if (s->st) (void)hipStreamSynchronize(s->st);
  free_all(s);
  for (auto& q : s->krec) { (void)hipEventDestroy(q.a); (void)hipEventDestroy(q.b); }
  for (hipEvent_t e : s->ev_free) (void)hipEventDestroy(e);
  if (s->h_pin) (void)hipHostFree(s->h_pin);
  if (s->wave_exec) (void)hipGraphExecDestroy(s->wave_exec);
  if (s->wave_graph) (void)hipGraphDestroy(s->wave_graph);
  if (s->st) (void)hipStreamDestroy(s->st);
  if (s->st2) (void)hipStreamDestroy(s->st2);
  if (s->st3) (void)hipStreamDestroy(s->st3);
  for (int k = 0; k < 5; ++k) {
    if (s->ev_fork[k]) (void)hipEventDestroy(s->ev_fork[k]);
    if (s->ev_join[k]) (void)hipEventDestroy(s->ev_join[k]);
  }
  delete s->xf;
  delete s;
}

// One handle = rows [lo, hi) of a mesh; unsharded when xf is null (world 1, no exchange).
static int create_shard(const kb_config* cfg, int rank, int world, Xfer* xf, kb_sim** out) {
  h_crc_init();
  if (!cfg || !out || cfg->abi_version != KB_ABI_VERSION) { seterr("bad config"); delete xf; return KB_INVALID_ARGUMENT; }
  if (cfg->capacity == 0 || cfg->capacity > 7800000u || cfg->initial_nodes > cfg->capacity || cfg->id_len > MAXID ||
      cfg->max_waves == 0 || cfg->max_waves > 64) { seterr("config out of range"); delete xf; return KB_INVALID_ARGUMENT; }
  if (cfg->stat_flags) { seterr("kb_config.stat_flags: sparse rows and the oracle only"); delete xf; return KB_INVALID_ARGUMENT; }
  if (cfg->variant && cfg->variant != KB_VARIANT_EXACT_LRU) { seterr("semantic variants other than KB_VARIANT_SPARSE_ROWS are measurement-only (CPU oracle)"); delete xf; return KB_INVALID_ARGUMENT; }
  const uint32_t C = cfg->capacity;
  const uint32_t rows_per = (C + (uint32_t)world - 1) / (uint32_t)world;
  if (world < 1 || world > (int)XMAX || rank < 0 || rank >= world || (uint64_t)(world - 1) * rows_per >= C) {
    seterr("shard layout out of range (1..8 shards, each holding at least one row)"); delete xf; return KB_INVALID_ARGUMENT;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { seterr("no HIP device"); delete xf; return KB_NO_DEVICE; }
  kb_sim* s = new kb_sim();
  memset((void*)&s->d, 0, sizeof s->d);
  memset((void*)&s->xs, 0, sizeof s->xs);
  s->cfg = *cfg;
  s->xf = xf;
  s->rank = rank; s->world = world;
  s->device = cfg->device >= 0 ? cfg->device : 0;
  if (cfg->device < 0) (void)hipGetDevice(&s->device);
  if (hipSetDevice(s->device) != hipSuccess) { destroy_shard(s); seterr("hipSetDevice failed"); return KB_NO_DEVICE; }
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, s->device) != hipSuccess) { destroy_shard(s); seterr("hipGetDeviceProperties failed"); return KB_NO_DEVICE; }
    s->ncu = (uint32_t)prop.multiProcessorCount;
    s->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 65536;
  }
  const uint32_t W = (C + 8191) / 8192 * 8192;       // 64 segments of whole 128-id steps
  s->C = C; s->W = W; s->round = 0;
  s->lo = (uint32_t)rank * rows_per;
  s->hi = std::min<uint32_t>(C, s->lo + rows_per);
  s->R = s->hi - s->lo;
  const uint32_t R = s->R;
  const uint32_t groups = (R + 63) / 64;
  uint32_t S = 1;
constexpr uint32_t KB_FOLD_WAVES = 16384;                            // fold waves wanted: column splits double up to it (64K:
                                                       // 16 splits, 0.44 -> 0.42 ms against 8 and 32, profiles/r04fs_ab_fold_splits.txt)
  while (S < 64 && groups * S < KB_FOLD_WAVES) S <<= 1;   // enough sweep waves to fill the chip
  s->S = S;
  Dev& d = s->d;
  d.lo = s->lo; d.hi = s->hi;
  d.C = C; d.W = W; d.SEGW = W / NSEG; d.NWR = W / 32;
  d.segq = d.SEGW / 128;
  d.segm = d.segq > 1 ? (uint32_t)(((1ull << 32) + d.segq - 1) / d.segq) : 0u;
  d.k0 = (uint32_t)cfg->seed; d.k1 = (uint32_t)(cfg->seed >> 32);
  d.loss_thr = cfg->loss_threshold; d.churn_thr = cfg->churn_threshold; d.fault_end = cfg->fault_end_round;
  d.failed_mode = cfg->failed_mode; d.pgroups = cfg->partition_groups; d.pstart = cfg->partition_start;
  d.pend = cfg->partition_end;
  const uint32_t Lid = cfg->id_len;
  d.capk = (BUFSZ - 20 - Lid) / (18 + Lid);           // 20 + L + k(18+L) <= 10240
  d.capj = (BUFSZ - 20 - Lid - 1) / (18 + Lid);       // 20 + L + k(18+L) <  10240
  d.paybound = C < d.capk ? C : d.capk;
  d.dbg = cfg->debug_flags;
  if (const char* dv = getenv("KB_DEV")) d.dev = (uint32_t)atoi(dv);
  s->debug_waves = getenv("KB_DEBUG_WAVES") != nullptr;
  if (const char* gv = getenv("KB_WAVE_GRAPH")) s->graph_on = atoi(gv) != 0;
  if (cfg->debug_flags & KB_DBG_WAVE_GRAPH) s->graph_on = true;
  s->h_ident.assign((size_t)C * MAXID, 0); s->h_idlen.assign(C, (uint8_t)Lid);
  s->h_pend.assign((size_t)C * MAXID, 0); s->h_pendlen.assign(C, (int16_t)-1); s->h_moved.assign(C, 0);
  s->h_idset.assign(C, 0);
  for (uint32_t j = 0; j < C; ++j) default_identity(j, Lid, &s->h_ident[(size_t)j * MAXID]);
  hipError_t e = hipSuccess;
#define A(ptr, n) if (e == hipSuccess) e = talloc(s, &(ptr), (n))     // per-id / global tables
#define AR(ptr, n) if (e == hipSuccess) e = ralloc(s, &(ptr), (n))   // row tables: n entries per local row
  AR(d.stamp, W); AR(d.bits, d.NWR); AR(d.segp, NSEG); AR(d.sdirty, 1);
  AR(d.dirty, 1); A(d.alive, C); A(d.idset, C); A(d.ext, C); A(d.abits, d.NWR); A(d.start_round, C); AR(d.n, 1); AR(d.fp, 1);
  AR(d.last_bcast, 1); AR(d.a3cur, 1); AR(d.susp, SLOTS); AR(d.cur, CSLOTS); AR(d.paq, PAQ);
  AR(d.paq_n, 1); A(d.cseg, C); A(d.segmul, C); A(d.seglen, C); A(d.zpow, (size_t)C + 2); A(d.zfin, (size_t)C + 2);
  A(d.ztab, 17 * 128); A(d.zbtab, ZB);
  A(d.htab, (size_t)(W / 8) * 256); A(d.stats, NSTAT); A(d.sacc, (size_t)NACC * NSTAT); A(d.ctr, NCTR); A(d.truefp, 1); A(d.tfpart, TRUEFP_G);
  AR(d.flog, LOGCAP); AR(d.flog_n, 1); AR(d.fstart, 16); AR(d.kpr_big, 1);
  if (cfg->variant == KB_VARIANT_EXACT_LRU) { AR(d.tst, W); AR(d.tlb, W / 1024); }   // exact A3 instants
  if (cfg->track_latency) { A(d.lat, (size_t)W * lat_stride(R)); A(s->lat_col, C); A(s->fnamed, d.NWR); }   // peer-major
  s->msg_cap = std::max<uint32_t>(8u * R + (uint32_t)TICK_MAX * R, 1u << 16);
  s->pay_cap = std::max<uint32_t>((d.capk + 1) * R, 1u << 24);
  for (int b = 0; b < 2; ++b) {
    A(s->ob[b].msgs, s->msg_cap); A(s->ob[b].pay, s->pay_cap); AR(s->ob[b].off, 1); AR(s->ob[b].cap, 1);
    AR(s->ob[b].cnt, 1); AR(s->ob[b].poff, 1);
    s->ob[b].msg_cap = s->msg_cap; s->ob[b].pay_cap = s->pay_cap;
  }
  AR(s->wc.cnt1, 1); AR(s->wc.bnd, 1); AR(s->wc.bpay, 1); AR(s->wc.cursor, 1);
  AR(s->wc.in_off, 1); A(s->wc.active, R);
  AR(s->wc.kcnt, 1); AR(s->wc.kpay, 1); AR(s->wc.kcur, 1); AR(s->wc.koff, 1);
  if (!xf) { A(s->wc.status, s->msg_cap); A(s->wc.inbox, s->msg_cap); A(s->wc.kin, s->msg_cap); }
  A(s->bfail, (size_t)C * SLOTS); A(s->bjoin, C);
  AR(s->bs.join, 1); AR(s->bs.nfail, 1); AR(s->bs.fail, SLOTS); AR(s->join_off, 1); AR(s->fail_off, 1);
  A(s->scan_tot, 32); A(s->rr, 4); A(s->scan_tiles, 5 * ((std::max<size_t>(C, (size_t)world * R) + 1023) / 1024) + 5);
  AR(s->nresp, 1); AR(s->paysum, 1); AR(s->nbase, 1); AR(s->resp_off, 1);
  A(s->resp_nodes, R); A(s->bf_gid, (size_t)C * SLOTS); A(s->bf_dep, (size_t)C * SLOTS); A(s->slow, R); A(s->defer, R); A(s->w0ctr, W0_WORDS);
  A(s->rest[0], R); A(s->rest[1], R); A(s->rest2n, 1); AR(s->a2flag, 1);
  AR(s->ro.part, 10);
  if (xf) {
    XState& x = s->xs;
    x.world = (uint32_t)world; x.R = R; x.S = rows_per; x.RS = R + 1;
    x.NWW = d.NWR; x.nju = 0; x.nj = 0; x.uon = 0;
    s->ucap = std::min<uint32_t>(UCAP, C);             // Join-response unions (kb_waves.h): slots and their reserve
    A(x.ostatus, s->msg_cap); A(x.xcnt, (size_t)world * x.RS); A(x.xpay, (size_t)world * x.RS);
    A(x.xoff, (size_t)world * x.RS); A(x.xpoff, (size_t)world * x.RS); A(x.xb, 2 * world);
    A(x.smsg, (size_t)s->msg_cap + s->ucap); A(x.spay, (size_t)s->pay_cap + (size_t)s->ucap * x.NWW);
    A(x.jslot, C); A(x.ubits, (size_t)s->ucap * x.NWW); A(x.uany, s->ucap);
    A(s->xall, std::max(2 * world * world, 3 * world));   // wave counts (2W per rank), round results (3 per rank)
    A(s->xstats, NSTAT);
    A(s->bfail_loc, (size_t)R * SLOTS); A(s->bjoin_loc, R);
    s->h_xall.assign(2 * world * world, 0);
  }
#undef A
#undef AR
  if (e != hipSuccess) { seterr(std::string("device allocation failed: ") + hipGetErrorString(e)); destroy_shard(s); return KB_CAPACITY; }
  (void)hipMemset(L(s, d.kpr_big), 0xFF, 4ull * R);          // no round yet
  if (xf) { (void)hipMemset(s->xs.jslot, 0xFF, 4ull * C); (void)hipMemset(s->xs.ubits, 0, 4ull * s->ucap * s->xs.NWW); }
  if (d.lat) { (void)hipMemset(d.lat, 0xFF, 2ull * lat_stride(R) * W); (void)hipMemset(s->fnamed, 0, 4ull * d.NWR); }   // all None
  if (d.tst) {
    (void)hipMemsetD32(d.tst + (size_t)s->lo * W, INT32_MIN / 2, (size_t)R * W);   // a converged start: ancient, all tied
    (void)hipMemsetD32(d.tlb + (size_t)s->lo * (W / 1024), INT32_MIN, (size_t)R * (W / 1024));   // bounds: scan every block once
  }
  s->wc.msg_cap = s->msg_cap; s->wc.pay_cap = s->pay_cap;
  if (hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess) { destroy_shard(s); seterr("stream"); return KB_IO_ERROR; }
  if (hipStreamCreateWithFlags(&s->st2, hipStreamNonBlocking) != hipSuccess) { destroy_shard(s); seterr("stream"); return KB_IO_ERROR; }
  if (hipStreamCreateWithFlags(&s->st3, hipStreamNonBlocking) != hipSuccess) { destroy_shard(s); seterr("stream"); return KB_IO_ERROR; }
  for (int k = 0; k < 5; ++k)
    if (hipEventCreateWithFlags(&s->ev_fork[k], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_join[k], hipEventDisableTiming) != hipSuccess) { destroy_shard(s); seterr("events"); return KB_IO_ERROR; }
  if (hipHostMalloc((void**)&s->h_pin, 4 * PIN_WORDS, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
    s->h_pin = nullptr; destroy_shard(s); seterr("pinned buffer"); return KB_IO_ERROR;
  }
  if (hipHostGetDevicePointer((void**)&s->d_pin, s->h_pin, 0) != hipSuccess) { destroy_shard(s); seterr("pinned buffer mapping"); return KB_IO_ERROR; }
  if (const char* pv = getenv("KB_PROF")) s->prof_level = atoi(pv);
  int rc = upload_segments(s);
  if (rc) { destroy_shard(s); return rc; }
  uint32_t ctr0[NCTR] = {0};
  ctr0[C_NEXTFREE] = cfg->initial_nodes;
  ctr0[C_FIRSTCONV] = 0xFFFFFFFFu; ctr0[C_LASTCONV] = 0xFFFFFFFFu;
  if (hipMemcpy(d.ctr, ctr0, sizeof ctr0, hipMemcpyHostToDevice) != hipSuccess) { destroy_shard(s); seterr("ctr upload"); return KB_IO_ERROR; }
  const uint32_t tb = 256, gb = (C + tb - 1) / tb;
  if (cfg->init_mode == KB_INIT_CONVERGED) {
    k_init_converged_rows<<<4096, 256, 0, s->st>>>(d, cfg->initial_nodes);
    k_init_converged_nodes<<<gb, tb, 0, s->st>>>(d, cfg->initial_nodes);
  } else {
    k_init_nodes<<<gb, tb, 0, s->st>>>(d, cfg->initial_nodes);
  }
  if (hipStreamSynchronize(s->st) != hipSuccess) { destroy_shard(s); seterr("init failed"); return KB_IO_ERROR; }
  *out = s;
  return KB_OK;
}

// ---- the router: four kinds of handle behind one kb_sim* (DESIGN.md "Host control plane") ------------------
// A leaf is a dense shard or a wrapper of a sparse engine (sp); a kb_sim_create_local group holds leaves of one sort.
static bool is_group(const kb_sim* s) { return !s->shards.empty(); }
struct Kind { bool sparse, group, rank; };           // rank: one rank of a kb_sim_create_rank mesh (its own rows only)
static Kind kind_of(const kb_sim* s) {
  const kb_sim* f = is_group(s) ? s->shards[0] : s;
  const bool leaf_xf = f->sp ? f->sp->xf != nullptr : f->xf != nullptr;
  return Kind{f->sp != nullptr, is_group(s), !is_group(s) && leaf_xf && !s->in_group};
}
static kb_sim* owner(kb_sim* g, uint32_t node) {     // the shard holding node's row
  for (kb_sim* t : g->shards) if (node >= t->lo && node < t->hi) return t;
  return nullptr;
}
// f on a leaf's engine: a generic callable, f(kb_sim*) for a dense shard and f(SpSim*) for the sparse rows
template <class F> static int visit(kb_sim* leaf, F&& f) { return leaf->sp ? f(leaf->sp) : f(leaf); }
// R_ALL: every shard in rank order, the first error wins (mesh-changing calls; with a callable that accumulates,
// the fold of the merging calls); R_OWNER: the shard holding node's row; R_FIRST: the first shard (replicated facts).
// A leaf handle answers every policy itself.  The shard's device is current while f runs.
enum Route { R_ALL, R_OWNER, R_FIRST };
template <class F> static int route(kb_sim* s, Route how, uint32_t node, F&& f) {
  if (!is_group(s)) return visit(s, f);
  if (how != R_ALL) {
    kb_sim* t = how == R_OWNER ? owner(s, node) : s->shards[0];
    (void)hipSetDevice(t->device);
    return visit(t, f);
  }
  for (kb_sim* t : s->shards) {
    (void)hipSetDevice(t->device);
    const int rc = visit(t, f);
    if (rc) return rc;
  }
  return KB_OK;
}

static void destroy_one(kb_sim* s) {                 // a dense shard, or a sparse handle (its engine owns the exchange)
  if (s->sp) { sp_destroy(s->sp); delete s; return; }
  destroy_shard(s);
}

extern "C" int kb_sim_create(const kb_config* cfg, kb_sim** out) {
  if (cfg && out && cfg->abi_version == KB_ABI_VERSION && (cfg->variant & KB_VARIANT_SPARSE_ROWS)) {
    if (cfg->capacity == 0 || cfg->capacity > 7800000u || cfg->initial_nodes > cfg->capacity || cfg->id_len > MAXID ||
        cfg->max_waves == 0 || cfg->max_waves > 64) { seterr("config out of range"); return KB_INVALID_ARGUMENT; }
    return sp_wrap(cfg, 0, 1, nullptr, out);
  }
  return create_shard(cfg, 0, 1, nullptr, out);
}

extern "C" int kb_rccl_unique_id(uint8_t* out, size_t cap) {
  if (!out || cap < sizeof(ncclUniqueId)) { seterr("unique id buffer too small"); return KB_INVALID_ARGUMENT; }
  ncclUniqueId id;
  const ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) { seterr(std::string("ncclGetUniqueId: ") + ncclGetErrorString(r)); return KB_IO_ERROR; }
  memcpy(out, &id, sizeof id);
  return KB_OK;
}

// a unique id for ranks that share ONE device (the IpcXfer test transport, kb_xfer.h): the magic prefix, then the
// name of the shared-memory segment rank 0 creates
extern "C" int kb_ipc_unique_id(uint8_t* out, size_t cap) {
  if (!out || cap < KB_UNIQUE_ID_BYTES) { seterr("unique id buffer too small"); return KB_INVALID_ARGUMENT; }
  memset(out, 0, KB_UNIQUE_ID_BYTES);
  memcpy(out, IPC_MAGIC, sizeof IPC_MAGIC);
  uint64_t rnd = 0;
  FILE* f = fopen("/dev/urandom", "rb");
  if (f) { if (fread(&rnd, sizeof rnd, 1, f) != 1) rnd = 0; fclose(f); }
  snprintf(reinterpret_cast<char*>(out) + sizeof IPC_MAGIC, KB_UNIQUE_ID_BYTES - sizeof IPC_MAGIC, "/kbipc-%d-%016llx",
           (int)getpid(), (unsigned long long)rnd);
  return KB_OK;
}

extern "C" int kb_sim_create_rank(const kb_config* cfg, int32_t rank, int32_t world, const uint8_t* unique_id, kb_sim** out) {
  if (!cfg || !unique_id || !out || world < 1 || world > (int)XMAX || rank < 0 || rank >= world) {
    seterr("bad rank/world"); return KB_INVALID_ARGUMENT;
  }
  if (hipSetDevice(cfg->device >= 0 ? cfg->device : 0) != hipSuccess) { seterr("hipSetDevice failed"); return KB_NO_DEVICE; }
  if (memcmp(unique_id, IPC_MAGIC, sizeof IPC_MAGIC) == 0) {          // ranks sharing one device (test transport)
    const char* wm = getenv("KB_IPC_WINDOW_MB");
    const size_t mb = wm ? (size_t)atoll(wm) : 256;
    IpcXfer* x = new IpcXfer();
    if (!x->init(rank, world, unique_id, mb << 20)) { seterr(x->error()); delete x; return KB_IO_ERROR; }
    return (cfg->variant & KB_VARIANT_SPARSE_ROWS) ? sp_wrap(cfg, rank, world, x, out) : create_shard(cfg, rank, world, x, out);
  }
  RcclXfer* x = new RcclXfer();
  if (!x->init(rank, world, unique_id)) { seterr(x->error()); delete x; return KB_IO_ERROR; }
  return (cfg->variant & KB_VARIANT_SPARSE_ROWS) ? sp_wrap(cfg, rank, world, x, out) : create_shard(cfg, rank, world, x, out);
}

extern "C" int kb_sim_create_local(const kb_config* cfg, int32_t shards, kb_sim** out) {
  if (!cfg || !out || shards < 1 || shards > (int)XMAX) { seterr("shards out of range (1..8)"); return KB_INVALID_ARGUMENT; }
  kb_sim* g = new kb_sim();
  g->cfg = *cfg; g->C = cfg->capacity; g->world = shards; g->R = 0;
  g->hub = new LocalHub(shards);
  const bool sparse = cfg->abi_version == KB_ABI_VERSION && (cfg->variant & KB_VARIANT_SPARSE_ROWS);
  for (int k = 0; k < shards; ++k) {
    LocalXfer* x = new LocalXfer();
    x->rank = k; x->world = shards; x->hub = g->hub;
    kb_sim* s = nullptr;
    const int rc = sparse ? sp_wrap(cfg, k, shards, x, &s) : create_shard(cfg, k, shards, x, &s);
    if (rc) { for (kb_sim* t : g->shards) destroy_one(t); delete g->hub; delete g; return rc; }
    s->in_group = true;
    if (s->sp) s->sp->in_group = true;
    g->shards.push_back(s);
  }
  g->device = g->shards[0]->device;
  *out = g;
  return KB_OK;
}

extern "C" int kb_sim_destroy(kb_sim* s) {
  if (!s) return KB_INVALID_ARGUMENT;
  if (!is_group(s)) { destroy_one(s); return KB_OK; }
  for (kb_sim* t : s->shards) destroy_one(t);
  delete s->hub;
  delete s;
  return KB_OK;
}

extern "C" int kb_sim_shard_info(kb_sim* s, int32_t* rank, int32_t* world, uint32_t* lo, uint32_t* hi) {
  if (!s || !rank || !world || !lo || !hi) return KB_INVALID_ARGUMENT;
  if (is_group(s)) { *rank = 0; *world = s->world; *lo = 0; *hi = s->C; return KB_OK; }
  return visit(s, [&](auto* e) { *rank = e->rank; *world = e->world; *lo = e->lo; *hi = e->hi; return KB_OK; });
}

// Host side of the pinned hand-offs: spin on the mapped sequence word (a stream synchronisation would
// pay an interrupt wake-up, tens of microseconds with the GPU idle), with the stream's own status as
// the way out when it drained without publishing (a fault).
static hipError_t sync_st(kb_sim* s) {            // a counted host wait on the simulator's stream
  s->host_syncs++;
  return hipStreamSynchronize(s->st);
}
static int wait_pin(kb_sim* s, uint32_t seq) {
  s->host_syncs++;
  volatile uint32_t* p = s->h_pin + PIN_SEQ;
  for (uint64_t it = 0;; ++it) {
    if (*p == seq) { std::atomic_thread_fence(std::memory_order_acquire); return KB_OK; }
    if ((it & 4095) == 4095) {
      const hipError_t e = hipStreamQuery(s->st);
      if (e == hipSuccess) {
        if (*p == seq) { std::atomic_thread_fence(std::memory_order_acquire); return KB_OK; }
        seterr("stream drained without publishing its results"); return KB_IO_ERROR;
      }
      if (e != hipErrorNotReady) { seterr(std::string("stream: ") + hipGetErrorString(e)); return KB_IO_ERROR; }
    }
  }
}
static int err_status(uint32_t e) {
  if (e) {
    const char* what[] = {"", "suspect slots exhausted", "outbox region overflow", "payload pool overflow",
                          "truncated Join response too large", "inbox overflow", "Join response member count mismatch",
                          "freshness log", "fingerprint count mismatch", "wave-0 outbox exceeds preallocated capacity",
                          "?", "export buffer overflow"};
    seterr(std::string("device capacity error: ") + (e < 12 ? what[e] : "?"));
    return KB_CAPACITY;
  }
  return KB_OK;
}
// The wave-0 outbox holds the round's Join responses (src/kaboodle.rs:356-392), whose volume follows the
// mesh's dynamics (≈1 % of the members answer each joiner with up to 567 ids): when the scanned totals
// exceed it, it grows, with the buffers indexed by its slots (record status, inbox lists, send side).
// The outbox's own two buffers grow under o0.pay_cap / o0.msg_cap; the buffers that must cover it (the send side's
// payload; the slot-indexed ones) are groups under pay_cap / msg_cap and follow whenever the outbox is the larger.
static int grow_wave0(kb_sim* s, size_t need_msg, size_t need_pay) {
  OutBuf& o0 = s->ob[0];
  window_stale(s);
  const size_t lim = 0xF0000000ull;
  if (need_pay > o0.pay_cap) {
    const size_t cap = std::min(lim, need_pay + need_pay / 4);
    if (cap < need_pay) { seterr("Join-response payload beyond 2^32 ids"); return KB_CAPACITY; }
    const int rc = eng_grow(s, &o0.pay, &o0.pay_cap, cap);
    if (rc) return rc;
  }
  if (s->xf && o0.pay_cap > s->pay_cap) {
    const size_t cap = o0.pay_cap;
    const int rc = eng_grow_group(s, &s->pay_cap, cap, cap + (size_t)s->ucap * s->xs.NWW, &s->xs.spay);
    if (rc) return rc;
  }
  if (need_msg > o0.msg_cap) {
    const size_t cap = std::min(lim, need_msg + need_msg / 4);
    if (cap < need_msg) { seterr("wave-0 records beyond 2^32"); return KB_CAPACITY; }
    const int rc = eng_grow(s, &o0.msgs, &o0.msg_cap, cap);
    if (rc) return rc;
  }
  if (o0.msg_cap > s->msg_cap) {               // slot-indexed buffers cover the larger outbox
    const size_t cap = o0.msg_cap;
    // (sharded: the send side keeps the union slots' reserve past the outbox; the status bytes get it too, unused)
    const int rc = !s->xf ? eng_grow_group(s, &s->msg_cap, cap, cap, &s->wc.status, &s->wc.inbox, &s->wc.kin)
                          : eng_grow_group(s, &s->msg_cap, cap, cap + s->ucap, &s->xs.ostatus, &s->xs.smsg);
    if (rc) return rc;
  }
  return KB_OK;
}

// grow the receive side of the sharded waves to hold nm records and np payload ids (rmsg_cap covers the records
// and the three buffers their slots index)
static int ensure_recv(kb_sim* s, size_t nm, size_t np) {
  if (nm > s->rmsg_cap || !s->rmsg) {
    const size_t cap = std::max<size_t>(nm + nm / 2, 1u << 16);
    const int rc = eng_grow_group(s, &s->rmsg_cap, cap, cap, &s->rmsg, &s->rstatus, &s->rinbox, &s->rkp);
    s->wc.status = s->rstatus; s->wc.inbox = s->rinbox; s->wc.kin = s->rkp;
    if (rc) return rc;
  }
  if (np > s->rpay_cap || !s->rpay) return eng_grow(s, &s->rpay, &s->rpay_cap, std::max<size_t>(np + np / 2, 1u << 20));
  return KB_OK;
}

// all-to-all-v of this wave's delivered records; returns the received record count, and
// in `any` whether any rank delivered a record this wave (the same answer on every rank: when no
// record moves, no handler runs and every later wave of the round is empty)
static int exchange_wave(kb_sim* s, OutBuf& ob, uint32_t& nrecv, RecvBlocks& rb, bool& any) {
  const int W = s->world, me = s->rank;
  XState& x = s->xs;
  hipStream_t st = s->st;
  if (x.uon) klaunch(s, KI_XBOUND, k_union_count, dim3(1), dim3(256), 0, x);   // the unions' records, counted
  {
    ScanArgs a = scan_args(s, (uint32_t)W * x.RS, s->scan_tot + 16);
    a.narr = 2;
    a.in[0] = x.xcnt; a.out[0] = x.xoff;
    a.in[1] = x.xpay; a.out[1] = x.xpoff;
    launch_scan(s, a);
  }
  klaunch(s, KI_XBOUND, k_xbound, dim3(1), dim3(64), 0, x, s->scan_tot + 16);
  klaunch(s, KI_PACK, k_pack, dim3((s->R + 3) / 4), dim3(256), 0, s->d, ob, x);
  if (x.uon) klaunch(s, KI_PACK, k_union_pack, dim3(x.nju), dim3(256), 0, x);
  if (!s->xf->allgather_u32(x.xb, s->xall, 2 * W, st)) { seterr(s->xf->error()); return KB_IO_ERROR; }
  k_publish<<<1, 1, 0, st>>>(s->xall, 2 * W * W, s->d_pin, ++s->pin_seq);   // counts -> host, then the wait
  { const int rc = wait_pin(s, s->pin_seq); if (rc) return rc; }
  memcpy(s->h_xall.data(), s->h_pin, 4ull * 2 * W * W);
  size_t sc[XMAX], sd[XMAX], rc[XMAX], rd[XMAX], psc[XMAX], psd[XMAX], prc[XMAX], prd[XMAX];
  size_t so = 0, pso = 0, ro = 0, pro = 0;
  uint64_t total = 0;
  for (int k = 0; k < W * W; ++k) total += s->h_xall[(size_t)(k / W) * 2 * W + (k % W)];
  any = total != 0;
  if (!any) { nrecv = 0; return KB_OK; }
  for (int k = 0; k < W; ++k) {
    sc[k] = s->h_xall[(size_t)me * 2 * W + k]; psc[k] = s->h_xall[(size_t)me * 2 * W + W + k];
    rc[k] = s->h_xall[(size_t)k * 2 * W + me]; prc[k] = s->h_xall[(size_t)k * 2 * W + W + me];
    sd[k] = so; so += sc[k]; psd[k] = pso; pso += psc[k];
    rd[k] = ro; ro += rc[k]; prd[k] = pro; pro += prc[k];
    const uint64_t b = sizeof(Msg) * (uint64_t)sc[k] + 4ull * psc[k];
    s->xbytes_all += b;
    if (k != me) s->xbytes_cross += b;
  }
  int rcode = ensure_recv(s, ro, pro);
  if (rcode) return rcode;
  // records and payload as one grouped exchange; once the group is open it is always closed
  if (!s->xf->group_begin()) { seterr(s->xf->error()); return KB_IO_ERROR; }
  const bool sent = s->xf->alltoallv(x.smsg, sc, sd, s->rmsg, rc, rd, sizeof(Msg), st) &&
                    s->xf->alltoallv(x.spay, psc, psd, s->rpay, prc, prd, 4, st);
  const std::string e1 = sent ? std::string() : s->xf->error();
  if (!s->xf->group_end() || !sent) { seterr(sent ? s->xf->error() : e1); return KB_IO_ERROR; }
  rb.world = (uint32_t)W;
  for (int k = 0; k <= W && k <= (int)XMAX; ++k) {
    rb.m0[k] = k < W ? (uint32_t)rd[k] : (uint32_t)ro;
    rb.p0[k] = k < W ? (uint32_t)prd[k] : (uint32_t)pro;
  }
  nrecv = (uint32_t)ro;
  return KB_OK;
}

// the round's broadcast lists of every shard, concatenated in shard order = sender order; the same
// all-gather carries every rank's error flag (*err = the largest): one host wait per round for both
static int gather_broadcasts(kb_sim* s, uint32_t* err) {
  const int W = s->world;
  hipStream_t st = s->st;
  if (!s->xf->allgather_u32(s->rr, s->xall, 3, st)) { seterr(s->xf->error()); return KB_IO_ERROR; }
  k_publish<<<1, 1, 0, st>>>(s->xall, 3 * W, s->d_pin, ++s->pin_seq);
  { const int rc = wait_pin(s, s->pin_seq); if (rc) return rc; }
  size_t sc[XMAX], sd[XMAX], rc[XMAX], rd[XMAX], fsc[XMAX], frc[XMAX], frd[XMAX];
  size_t oj = 0, of = 0;
  uint32_t e = 0;
  for (int k = 0; k < W; ++k) {
    rc[k] = s->h_pin[3 * k]; frc[k] = s->h_pin[3 * k + 1]; e = std::max(e, s->h_pin[3 * k + 2]);
    rd[k] = oj; oj += rc[k]; frd[k] = of; of += frc[k];
  }
  for (int k = 0; k < W; ++k) { sc[k] = rc[s->rank]; fsc[k] = frc[s->rank]; sd[k] = 0; }
  *err = e;
  if (!s->xf->group_begin()) { seterr(s->xf->error()); return KB_IO_ERROR; }
  const bool sent = s->xf->alltoallv(s->bjoin_loc, sc, sd, s->bjoin, rc, rd, sizeof(BCast), st) &&
                    s->xf->alltoallv(s->bfail_loc, fsc, sd, s->bfail, frc, frd, sizeof(BCast), st);
  const std::string e1 = sent ? std::string() : s->xf->error();
  if (!s->xf->group_end() || !sent) { seterr(sent ? s->xf->error() : e1); return KB_IO_ERROR; }
  s->nj = (uint32_t)oj; s->nf = (uint32_t)of;
  return KB_OK;
}

// what the row pass launches with (rowpass_plan, below): both broadcast lists staged in LDS (ll), each row's bitset
// staged (ldsb), waves per workgroup, dynamic LDS bytes, resident workgroups per CU, workgroups
struct RowPlan { bool ldsb, ll; uint32_t wpb; size_t lds; uint32_t per_cu, blocks; };
#include "kb_rounddbg.h"

// The receive window's delivery waves.  rk is the round the kernels take as
// argument; rk < 0 makes them read it from the device (d.ctr[C_ROUND], set by k_log_mark), which lets
// the unsharded window be captured once as a HIP graph and replayed every round.
static int launch_waves(kb_sim* s, int32_t rk) {
  Dev& d = s->d;
  const int32_t r = rk;
  const uint32_t R = s->R;
  hipStream_t st = s->st;
  const uint32_t tb = 256, gnode = (R + tb - 1) / tb;
  int cur = 0;
  for (uint32_t w = 0; w <= s->cfg.max_waves; ++w) {
    OutBuf& ob = s->ob[cur];
    OutBuf& nb = s->ob[cur ^ 1];
    const int last = w == s->cfg.max_waves;
    d.wave = (int32_t)w;                               // latency clock of the wave's prologues
    s->cur_wave = (int)w;
    OutBuf ib = ob;                                    // the wave's delivered records
    uint32_t nrecv = 0;
    if (!s->xf) {
      klaunch(s, KI_ROUTE, k_route, dim3(gnode), dim3(tb), 0, d, ob, s->wc, r, w, last);
      if (last) break;
    } else {
      HIPCHK(hipMemsetAsync(s->xs.xcnt, 0, 4ull * s->world * s->xs.RS, st));
      HIPCHK(hipMemsetAsync(s->xs.xpay, 0, 4ull * s->world * s->xs.RS, st));
      // wave 0: the round's joiners' slots for the Join-response unions
      s->xs.nju = w == 0 && !last ? std::min<uint32_t>(s->nj, s->ucap) : 0u;
      s->xs.uon = s->xs.nju && !(d.dbg & KB_DBG_NO_UNION) ? 1u : 0u;
      s->xs.nj = s->xs.uon ? s->nj : 0u;
      s->xs.bjoin = s->bjoin;
      if (s->xs.uon) klaunch(s, KI_ROUTE_X, k_union_slots, dim3((s->xs.nju + 255) / 256), dim3(256), 0, s->xs);
      klaunch(s, KI_ROUTE_X, k_route_x, dim3(gnode), dim3(tb), 0, d, ob, s->xs, r, w, last);
      if (last) break;
      RecvBlocks rb;
      memset(&rb, 0, sizeof rb);
      bool any = true;
      int rc = exchange_wave(s, ob, nrecv, rb, any);
      s->xs.uon = 0;
      if (rc) return rc;
      if (!any) break;                                 // no record anywhere: the rest of the round's waves are empty
      ib.msgs = s->rmsg; ib.pay = s->rpay;
      if (nrecv) klaunch(s, KI_ROUTE_RECV, k_route_recv, dim3((nrecv + 255) / 256), dim3(256), 0, d, ib, s->wc, rb, nrecv);
    }
    {
      ScanArgs a = scan_args(s, R, s->scan_tot + 8);
      a.narr = 4;
      a.in[0] = L(s, s->wc.cnt1); a.out[0] = L(s, s->wc.in_off);
      a.in[1] = L(s, s->wc.bnd); a.out[1] = L(s, nb.off);
      a.in[2] = L(s, s->wc.bpay); a.out[2] = L(s, nb.poff);
      a.in[3] = L(s, s->wc.kcnt); a.out[3] = L(s, s->wc.koff);
      a.list = s->wc.active; a.list_count = d.ctr + C_ACTIVE; a.list_base = s->lo; a.list_or3 = 1;
      launch_scan(s, a);
    }
    { const int rc = dbg_wave_inboxes(s, r, w); if (rc) return rc; }
    // (the inbox placement, and in PROBE_GROUPS more workgroups the KPR oversize probe)
    if (!s->xf) klaunch(s, KI_SCATTER, k_scatter, dim3(gnode + PROBE_GROUPS), dim3(tb), 0, d, ob, s->wc, r, gnode);
    else if (nrecv) {
      const uint32_t nsc = (nrecv + 255) / 256;
      klaunch(s, KI_SCATTER_FLAT, k_scatter_flat, dim3(nsc + PROBE_GROUPS), dim3(256), 0, d, ib, s->wc, nrecv, r, nsc);
    }
    { const int rc = dbg_proc_clear(s); if (rc) return rc; }
    // wave 0 of a round with joiners: their BIG groups overlap the in-order handlers of every other node.  Not
    // under graph capture (the window stays one chain there), KB_DEBUG_WAVES (its read-backs follow st only) or
    // KB_DBG_WAVE0_SERIAL
    const bool split = w == 0 && s->nj > 0 && !s->xf && !s->graph_on && !s->capturing && !s->debug_waves &&
                       !(d.dbg & KB_DBG_WAVE0_SERIAL);
    {  // the KnownPeers groups: BIG ones KP_COLS workgroups per destination group (one per column part),
       // then the small ones (a wave per destination), which also set up nb.cap / nb.cnt
      const uint32_t ks = (d.NWR <= KP_LDS_WORDS && !(d.dbg & KB_DBG_KP_HBM)) ? KP_COLS : 1u;
      const uint32_t groups = std::max<uint32_t>(1u, std::min<uint32_t>((R + 1023) / 1024 * (ks > 1 ? 2u : 1u), 512u / ks));
      constexpr uint32_t KB_KPS_PER_CU = 1;        // small-group workgroups per CU (2: no faster, profiles/r04u2_ab_unrolls.txt)
      const uint32_t small = std::max<uint32_t>((R + 1023) / 1024, KB_KPS_PER_CU * s->ncu);
      if (split) {
        // split wave 0: the BIG groups (the round's joiners) alone on the side stream, from here
        // (the inboxes are placed) to the next wave's k_route; the small groups and the outbox setup stay here
        side_fork(s, 3);
        klaunch_on(s, s->st2, KI_KP, k_kp, dim3(ks * groups), dim3(1024), (uint32_t)kp_lds_bytes(d.NWR), d, ib, s->wc, r, nb,
                   ks * groups, (uint32_t*)nullptr);
        side_done(s, 3);
        klaunch(s, KI_KP, k_kp, dim3(small), dim3(1024), 0, d, ib, s->wc, r, nb, 0u, s->w0ctr);
      } else
        klaunch(s, KI_KP, k_kp, dim3(ks * groups + small), dim3(1024), (uint32_t)kp_lds_bytes(d.NWR), d, ib, s->wc, r,
                nb, ks * groups, (uint32_t*)nullptr);
    }
    // inbox sorts + the KPR oversize probe, and the fast handlers (split: a BIG group's destination goes to `defer`)
    klaunch(s, KI_SORTFAST, k_sortfast, dim3(SORT_GROUPS + (R + SORTFAST_T - 1) / SORTFAST_T), dim3(SORTFAST_T), 0, d, ib, nb,
            s->wc, r, s->slow, SORT_GROUPS, split ? s->defer : (uint32_t*)nullptr, split ? s->w0ctr : (uint32_t*)nullptr);
    // persistent: as many workgroups as stay resident (204 VGPRs: 2 waves/SIMD, 2 workgroups per CU).
    // A larger grid only queues workgroups that read the node count and exit, which set a ~40 us floor
    // on the late waves with few nodes.
    klaunch(s, KI_PROC, k_proc, dim3(std::min<uint32_t>(4096, (KB_PROC_WPE > 2 ? KB_PROC_WPE : 2) * s->ncu)), dim3(256), 0, d, ib, nb, s->wc, r,
            (const uint32_t*)s->slow, (const uint32_t*)(d.ctr + C_SLOW), split ? s->w0ctr + W0_TICKET : (uint32_t*)nullptr);
    if (split) {
      // after the join: the BIG groups' destinations, in order behind their groups (the joiners that also got a
      // Ping, Ack or KPR; the others only have their counters cleared)
      side_join(s, 3);
      klaunch(s, KI_PROC, k_proc, dim3(std::min<uint32_t>(2 * s->ncu, std::max<uint32_t>(1u, (s->nj + 3) / 4))), dim3(256), 0, d, ib, nb,
              s->wc, r, (const uint32_t*)s->defer, (const uint32_t*)(s->w0ctr + W0_DEFER), (uint32_t*)nullptr);
    }
    { const int rc = dbg_proc_report(s, r, w); if (rc) return rc; }
    cur ^= 1;
  }
  s->cur_wave = -1;
  return KB_OK;
}

// A restart's map: the old address's row packed on the shard holding it, moved (sharded: an all-to-all-v
// in which only that shard sends, to the shard holding the new row) and unpacked; the event observer
// moves with it (src/lib.rs:104: the map and its observer belong to the Kaboodle, not to its socket).
// *snap_after: an observer attached to the new address before this round (after start() returned) and the
// instance had none: its snapshot is taken from the row once the restart has applied (the caller), so the
// channel reports only later changes, not the whole inherited map
static int move_row(kb_sim* s, uint32_t from, uint32_t to, bool* snap_after) {
  *snap_after = false;
  const RowPack LP = row_pack_layout(s->W, s->d.NWR, s->d.lat != nullptr, s->d.tst != nullptr);
  if (!s->rpack) { size_t c = 0; const int rc = eng_grow(s, &s->rpack, &c, LP.words); if (rc) return rc; }
  if (s->xf && !s->rpack_in) { size_t c = 0; const int rc = eng_grow(s, &s->rpack_in, &c, LP.words); if (rc) return rc; }
  const bool have = from >= s->lo && from < s->hi, take = to >= s->lo && to < s->hi;
  size_t wk = 0;
  while (wk < s->watch_node.size() && s->watch_node[wk] != from) ++wk;
  const bool watched = have && wk < s->watch_node.size();
  const uint32_t g = (LP.words + 255) / 256 < 1024 ? (LP.words + 255) / 256 : 1024;
  if (have) k_row_pack<<<g, 256, 0, s->st>>>(s->d, from, s->rpack, LP, watched ? s->watch_snap[wk] : nullptr,
                                            watched ? s->watch_fp[wk] : 0u);
  if (watched) { s->watch_node.erase(s->watch_node.begin() + wk); s->watch_fp.erase(s->watch_fp.begin() + wk);
                 s->watch_snap.erase(s->watch_snap.begin() + wk); }
  const uint32_t* src = s->rpack;
  if (s->xf) {
    const int W = s->world, S = (int)s->xs.S;
    const int ofrom = (int)(from / (uint32_t)S), oto = (int)(to / (uint32_t)S);
    size_t sc[XMAX] = {}, sd[XMAX] = {}, rc[XMAX] = {}, rd[XMAX] = {};
    if (s->rank == ofrom) sc[oto] = LP.words;
    if (s->rank == oto) rc[ofrom] = LP.words;
    (void)W;
    if (!s->xf->group_begin()) { seterr(s->xf->error()); return KB_IO_ERROR; }
    const bool sent = s->xf->alltoallv(s->rpack, sc, sd, s->rpack_in, rc, rd, 4, s->st);
    const std::string e1 = sent ? std::string() : s->xf->error();
    if (!s->xf->group_end() || !sent) { seterr(sent ? s->xf->error() : e1); return KB_IO_ERROR; }
    src = s->rpack_in;
  }
  if (!take) return KB_OK;
  uint32_t hdr[RP_HDR];
  HIPCHK(hipMemcpyAsync(hdr, src, sizeof hdr, hipMemcpyDeviceToHost, s->st));
  HIPCHK(sync_st(s));
  uint32_t* snap = nullptr;
  size_t kt = 0;
  while (kt < s->watch_node.size() && s->watch_node[kt] != to) ++kt;
  if (hdr[RP_WATCHED]) {                           // the instance's observer replaces one attached to the new address
    if (kt < s->watch_node.size()) { snap = s->watch_snap[kt]; s->watch_fp[kt] = hdr[RP_WFP]; }
    else {
      HIPCHK(talloc(s, &snap, (size_t)s->d.NWR));
      s->watch_node.push_back(to); s->watch_fp.push_back(hdr[RP_WFP]); s->watch_snap.push_back(snap);
    }
  } else if (kt < s->watch_node.size()) {
    *snap_after = true;
  }
  k_row_unpack<<<g, 256, 0, s->st>>>(s->d, to, src, LP, snap);
  return KB_OK;
}

// ---- one round, as its phases ---------------------------------------------------------------
// What the phases hand on.  Everything here is launches on st (side work on st2, forked and joined by events) in
// one fixed order; the host waits only where a phase says so.
struct Round {
  int32_t r;
  PhaseB pb;                                         // the broadcast phase's lists, masks and per-row sums
  bool lat_fail = false;                             // latency upkeep for Failed removals runs this round (side work 1)
  uint32_t np = 0;                                   // Probes delivered this round
  uint32_t ninj = 0; bool inj_pay = false;           // records injected by external peers; they carry payload ids
  hipEvent_t er[2] = {nullptr, nullptr};             // the whole round, read back next round
  size_t krec0 = 0;                                  // profile records of earlier rounds (complete)
  bool tick_scanned = false;                         // A1 ran ahead of the Join responses
  bool resp_side = false;                            // phase 2 of the Join responses is on the third stream (side work 4)
};
constexpr uint32_t TB = 256;                         // threads of the per-node launches
static uint32_t gnode(const kb_sim* s) { return (s->R + TB - 1) / TB; }

// API events in call order; a restart first moves the instance's map to its new address (the events before it
// have been applied: its stop removed the old self), then starts it there.  One host wait.
static int apply_events(kb_sim* s, int32_t r) {
  Dev& d = s->d;
  if (s->events.empty()) return KB_OK;
  { const int rc = round_upload_events(s); if (rc) return rc; }
  size_t k0 = 0;
  for (size_t k = 0; k <= s->events.size(); ++k) {
    const bool rs = k < s->events.size() && s->events[k].kind == EV_RESTART;
    if (k == s->events.size() || rs) {
      if (k > k0) klaunch(s, KI_EVENTS, k_events, dim3(1), dim3(1), 0, d, s->d_events + k0, (uint32_t)(k - k0), r);
      k0 = k;
      if (rs) {
        bool snap_after = false;
        const uint32_t to = s->events[k].node;
        const int rc = move_row(s, s->events[k].src, to, &snap_after);
        if (rc) return rc;
        if (snap_after) {                                // the restart itself, then the observer's starting point
          klaunch(s, KI_EVENTS, k_events, dim3(1), dim3(1), 0, d, s->d_events + k, 1u, r);
          size_t kt = 0;
          while (s->watch_node[kt] != to) ++kt;
          k_events_commit<<<(d.NWR + 255) / 256, 256, 0, s->st>>>(d.bits + (size_t)to * d.NWR, s->watch_snap[kt], d.NWR);
          k0 = k + 1;
        }
      }
    }
  }
  HIPCHK(sync_st(s));
  s->events.clear();
  return KB_OK;
}
// 0. stamp window; 1. lifecycle (every shard applies the same events and churn draws to the replicated per-id state)
static int round_lifecycle(kb_sim* s, Round& q) {
  Dev& d = s->d;
  const int32_t r = q.r;
  if (r > 0 && r % EPOCH == 0) klaunch(s, KI_REBASE, k_rebase, dim3(8192), dim3(256), 0, d, r);
  { const int rc = apply_events(s, r); if (rc) return rc; }
  const bool faults_on = s->cfg.fault_end_round < 0 || r < s->cfg.fault_end_round;
  if (faults_on && s->cfg.churn_threshold) {
    klaunch(s, KI_CHURN_LEAVE, k_churn_leave, dim3((s->C + TB - 1) / TB), dim3(TB), 0, d, r);
    klaunch(s, KI_CHURN_JOIN, k_churn_join, dim3(1), dim3(64), 0, d, r);
  }
  klaunch(s, KI_LOG_MARK, k_log_mark, dim3(gnode(s)), dim3(TB), 0, d, r);
  return KB_OK;
}

// The row pass's launch shape (broadcast phase + A3 candidates, persistent waves; the broadcast lists staged in LDS
// once per workgroup when they fit).  The occupancy query runs once per shape (occ_key / occ_val).
// the four instantiations, named once: f(kernel) for the one the plan chose
template <class F> static void rowpass_with(const RowPlan& p, F&& f) {
  if (p.ldsb) { if (p.ll) f(k_rowpass<true, true>); else f(k_rowpass<true, false>); }
  else if (p.ll) f(k_rowpass<false, true>);
  else f(k_rowpass<false, false>);
}
static RowPlan rowpass_plan(kb_sim* s, bool pb_hbm) {
  const Dev& d = s->d;
  RowPlan p;
  const uint32_t budget = RP_LDS_BYTES / 4;          // dynamic LDS words per workgroup
  p.ll = s->nf <= PB_FMAX && s->nj <= PB_JMAX;       // both broadcast lists staged in LDS
  uint32_t listw = p.ll ? 2 * s->nf + s->nj : 0;
  if (listw > budget / 2 || pb_hbm) { p.ll = false; listw = 0; }
  // the LDS variant stages each row's whole bitset for the Failed group's membership tests; without a
  // Failed list (quiet rounds: A3 and a few Joins only) the row is read where A3 and the Joins touch it
  // (372K peers, no broadcasts: 3.41 -> 0.54 ms, profiles/r04e_rowpass_variants.json).  (Rows too wide for
  // more than 1-3 staged bitsets per workgroup still stage: the in-place variant with 8 waves per workgroup
  // and the lists in LDS measured 17.4 -> 21.5 ms at 262K peers and 44.7 -> 41.8 ms at 372K in rounds with
  // Failed lists, its random membership reads missing L2, profiles/r04s_nsweep.json)
  p.ldsb = s->W <= PB_LDS_W && budget - listw >= d.NWR && !pb_hbm && s->nf > 0;
  p.wpb = p.ldsb ? std::min<uint32_t>(RP_WAVES, (budget - listw) / d.NWR) : RP_WAVES;
  p.lds = 4ull * ((p.ldsb ? (size_t)p.wpb * d.NWR : 0) + listw);
  int occ = 0;                                       // resident workgroups per CU (LDS, registers)
  const uint64_t okey = ((uint64_t)p.ldsb << 63) | ((uint64_t)p.ll << 62) | ((uint64_t)p.wpb << 40) | (uint64_t)p.lds;
  if (okey == s->occ_key) occ = s->occ_val;
  else {
    rowpass_with(p, [&](auto k) { (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void*>(k), (int)(64 * p.wpb), p.lds); });
    s->occ_key = okey; s->occ_val = occ;
  }
  p.per_cu = std::max<uint32_t>(1, std::min<uint32_t>(8, (uint32_t)occ));
  p.blocks = std::min<uint32_t>((s->R + p.wpb - 1) / p.wpb, s->ncu * p.per_cu);
  return p;
}

// 2. broadcasts of round r-1 (with the external peers' Joins): the row pass, beside it side work 0 (the running set
// and its fingerprint) and 1 (the latency sweep), then the Probes.  No host wait (but merge_ext_joins' two).
static int round_broadcasts(kb_sim* s, Round& q) {
  Dev& d = s->d;
  const int32_t r = q.r;
  const uint32_t R = s->R;
  if (!s->inj_join.empty()) { const int rc = merge_ext_joins(s->st, s->bjoin, &s->nj, s->inj_join, 0, s->C); if (rc) return rc; }
  PhaseB& pb = q.pb;
  pb.bfail = s->bfail; pb.nf = s->nf; pb.bjoin = s->bjoin; pb.nj = s->nj; pb.JW = (s->nj + 63) / 64;
  pb.nresp = s->nresp; pb.paysum = s->paysum; pb.nbase = s->nbase;
  if (pb.JW) {
    const size_t words = (size_t)R * pb.JW;
    if (words > s->mask_words) {
      const int rc = eng_grow_group(s, &s->mask_words, words, words, &s->newmask_base, &s->respmask_base);
      if (rc) return rc;
    }
    s->newmask = bias(s->newmask_base, pb.JW, s->lo);
    s->respmask = bias(s->respmask_base, pb.JW, s->lo);
  }
  pb.newmask = s->newmask; pb.respmask = s->respmask;
  pb.gid = s->bf_gid; pb.dep = s->bf_dep;
  // latency upkeep for Failed removals; socket_faithful never honours Failed, so nothing to do there
  q.lat_fail = d.lat && s->nf && d.failed_mode == KB_FAILED_SIM_SENDER;
  pb.fnamed = q.lat_fail ? s->fnamed : nullptr;
  if (q.lat_fail) klaunch(s, KI_LAT_MARK, k_lat_mark, dim3((s->nf + 255) / 256), dim3(256), 0, (const BCast*)s->bfail, s->nf, s->fnamed);
  const bool pb_hbm = (d.dbg & KB_DBG_PHASEB_HBM) != 0;
  if (s->nf > BFAIL_LDS_MAX || (pb_hbm && s->nf)) klaunch(s, KI_BFAIL_PREP, k_bfail_prep, dim3((s->nf + 255) / 256), dim3(256), 0, (const BCast*)s->bfail, s->nf, s->bf_gid, s->bf_dep, d.ctr + C_PATHS);
  else if (s->nf) klaunch(s, KI_BFAIL_PREP, k_bfail_prep_lds, dim3(1), dim3(1024), 0, (const BCast*)s->bfail, s->nf, s->bf_gid, s->bf_dep);
  { const int rc = dbg_bcast_shape(s, r); if (rc) return rc; }
  {
    // the row pass; its events are taken by its own dispatch packet (hipExtLaunchKernel), so they time the kernel itself
    const RowPlan p = rowpass_plan(s, pb_hbm);
    { const int rc = dbg_rowpass_begin(s, r, p); if (rc) return rc; }
    if (p.ldsb && !p.ll) s->host_paths |= PATH_ROWPASS_LDS_HBM_LISTS;   // coverage (test surface), with the device's bits
    rowpass_with(p, [&](auto k) { klaunch(s, KI_ROWPASS, k, dim3(p.blocks), dim3(64 * p.wpb), (uint32_t)p.lds, d, pb, s->ro, r); });
    { const int rc = dbg_rowpass_shares(s, r, p); if (rc) return rc; }
  }
  // beside the Join responses: the running set and its fingerprint (read by the tick's agreement count; the
  // set changed last with the churn), and the latency sweep (writes latency entries only; the tick's A2 and
  // the waves write them next)
  side_fork(s, 0);
  klaunch_on(s, s->st2, KI_ALIVE_BITS, k_alive_bits, dim3((d.NWR + TB - 1) / TB), dim3(TB), 0, d);
  klaunch_on(s, s->st2, KI_TRUEFP_PART, k_truefp_part, dim3(TRUEFP_G), dim3(256), 0, d, d.tfpart);
  klaunch_on(s, s->st2, KI_TRUEFP_FIN, k_truefp_fin, dim3(1), dim3(64), 0, d, d.tfpart);
  side_done(s, 0);
  if (q.lat_fail) {
    klaunch_on(s, s->st2, KI_LAT_SWEEP, k_lat_sweep, dim3((lat_stride(R) / 8 + 255) / 256, std::min<uint32_t>(s->nf, 16384)), dim3(256), 0, d,
            (const BCast*)s->bfail, (const uint32_t*)s->bf_gid, s->nf, s->fnamed);
    side_done(s, 1);
  }
  // the Probes queued since the last round travel with this round's broadcasts (after Failed and Join)
  { const int rc = round_take_probes(s, R, &q.np); if (rc) return rc; }
  if (q.np) klaunch(s, KI_PROBE, k_probe, dim3(gnode(s)), dim3(TB), 0, d, q.np, r, s->d_presp, s->d_presp_n, (uint32_t)s->presp_cap);
  return KB_OK;
}

// The round's Join responses into the wave-0 outbox: a wave per responder where its LDS slice fits (4 responders
// per 64 KB workgroup); wider rows keep only the slice's head in LDS and select from the row itself (up to 4 waves
// per workgroup, as the head fits: 3 at 1M-id rows); else (or forced) a workgroup with HBM scratch
//
// phase 0: every responder, on st (the serial order).  With the overlap on (resp_overlap_on) the round instead runs
// phase 1 on st ahead of A2 — the responders k_tick_scan flagged, a few hundred at most, on a grid of one workgroup
// per CU — and phase 2, all the others, on the third stream beside the tick.
static bool resp_rows_hbm(const kb_sim* s) { return s->W > RESP_LDS_W || (s->d.dbg & KB_DBG_RESP_HBM); }
static int launch_join_responses(kb_sim* s, Round& q, uint32_t resp_nodes, uint32_t phase) {
  Dev& d = s->d;
  const int32_t r = q.r;
  OutBuf& o0 = s->ob[0];
  hipStream_t st = phase == 2 ? s->st3 : s->st;
  uint32_t* rest = s->rest[phase == 2];
  uint32_t* restn = phase == 2 ? s->rest2n : d.ctr + C_RESTN;
  const uint32_t wcap = phase == 1 ? s->ncu : 4096;            // workgroups of the wave path
  const uint32_t grid = std::min<uint32_t>(resp_nodes, 4096);   // (the workgroup path: 2 per CU when it serves only
                                                               // the few responders the wave path lists)
  const size_t words = resp_words(d.NWR, s->W / 256);
  uint32_t* scratch = nullptr;
  size_t lds = 4 * words;
  const bool resp_hbm = resp_rows_hbm(s);
  if (resp_hbm) {
    { const int rc = eng_grow(s, &s->resp_scratch, &s->resp_scratch_words, words * grid); if (rc) return rc; }
    scratch = s->resp_scratch;
    lds = 0;
  }
  const size_t wlds = 16ull * rwave_words(d.NWR, s->W / 256);
  const size_t hlds = 4ull * rwave_head(s->W / 256);
  const bool full_on = wlds <= 65536 && !(d.dbg & (KB_DBG_RESP_HBM | KB_DBG_RESP_WAVE_HBM));
  const uint32_t hwaves = (uint32_t)std::min<size_t>(4, 65536 / hlds);
  const bool head_on = !full_on && hwaves >= 1 && !(d.dbg & KB_DBG_RESP_HBM);
  const bool wave_on = full_on || head_on;
  { const int rc = dbg_resp_clear(s); if (rc) return rc; }
  if (full_on) {                                   // timed by events on its own dispatch packet
    klaunch_on(s, st, KI_RESP_WAVE, k_resp_wave<false>, dim3(std::min<uint32_t>((resp_nodes + 3) / 4, wcap)), dim3(256), (uint32_t)wlds, d,
               q.pb, (const uint32_t*)s->resp_nodes, (const uint32_t*)(s->scan_tot + 4), o0, r, rest, restn, phase, (const uint8_t*)s->a2flag);
  } else if (head_on) {
    klaunch_on(s, st, KI_RESP_WAVE, k_resp_wave<true>, dim3(std::min<uint32_t>((resp_nodes + hwaves - 1) / hwaves, wcap)),
               dim3(64 * hwaves), (uint32_t)(hwaves * hlds), d, q.pb, (const uint32_t*)s->resp_nodes,
               (const uint32_t*)(s->scan_tot + 4), o0, r, rest, restn, phase, (const uint8_t*)s->a2flag);
  }
  // the workgroup path serves what the wave path left: its phase's list when the wave path ran, else every
  // responder
  klaunch_on(s, st, KI_RESP_NODE, k_resp_node, dim3(wave_on ? std::min<uint32_t>(grid, 2 * s->ncu) : grid), dim3(256), (uint32_t)lds, d, q.pb,
             (const uint32_t*)(wave_on ? rest : s->resp_nodes), (const uint32_t*)(wave_on ? restn : s->scan_tot + 4),
             o0, r, scratch, wave_on, phase, (const uint8_t*)s->a2flag);
  return dbg_resp_report(s, r);
}
// The Join responses beside the tick: unsharded, rows whose workgroup path needs no HBM scratch (sized for one
// launch), no per-wave debug reports, and not switched off (KB_DBG_RESP_SERIAL)
static bool resp_overlap_on(const kb_sim* s) {
  return !s->xf && !resp_rows_hbm(s) && !s->debug_waves && !(s->d.dbg & KB_DBG_RESP_SERIAL);
}
// A1 (and the list and flags of A2's nodes).  It writes bs.join, bs.nfail, last_bcast, the A2 list and a2flag, and
// reads alive, n and the suspect slots: nothing the Join responses read or write, so it runs ahead of them
// when they are split around A2
static void launch_tick_scan(kb_sim* s, Round& q) {
  klaunch(s, KI_TICK_SCAN, k_tick_scan, dim3(gnode(s)), dim3(TB), 0, s->d, s->bs, q.r, s->slow, s->a2flag);
  q.tick_scanned = true;
}

// Wave 0's outbox regions: the injected records' room, the scan (responses first, then the tick's messages) and
// k_set_cap.  In a round with joiners or injected payloads the totals come back over the first pinned hand-off
// (one host wait): the outbox and the export buffers grow to them, then the Join responses are written.
static int round_wave0_regions(kb_sim* s, Round& q) {
  Dev& d = s->d;
  const int32_t r = q.r;
  const uint32_t R = s->R;
  OutBuf& o0 = s->ob[0];
  // records from external peers (kb_sim_inject): room for their KnownPeers ids in their wave-0 payload regions
  q.ninj = (uint32_t)s->inj.size();
  if (q.ninj) {
    if (q.ninj > s->d_inj_cap) { const int rc = eng_grow(s, &s->d_inj, &s->d_inj_cap, 2 * (size_t)q.ninj); if (rc) return rc; }
    if (s->inj_ids.size() > s->d_inj_ids_cap || !s->d_inj_ids) {
      const int rc = eng_grow(s, &s->d_inj_ids, &s->d_inj_ids_cap, 2 * s->inj_ids.size() + 16);
      if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(s->d_inj, s->inj.data(), sizeof(XRec) * q.ninj, hipMemcpyHostToDevice, s->st));
    if (!s->inj_ids.empty()) {
      HIPCHK(hipMemcpyAsync(s->d_inj_ids, s->inj_ids.data(), 4 * s->inj_ids.size(), hipMemcpyHostToDevice, s->st));
      q.inj_pay = true;
    }
    klaunch(s, KI_EVENTS, k_inject_prep, dim3(1), dim3(64), 0, d, (const XRec*)s->d_inj, q.ninj, s->paysum);
  }
  {  // wave-0 outbox regions: responses first, then the tick's messages
    ScanArgs a = scan_args(s, R, s->scan_tot);
    a.narr = 3;
    a.in[0] = L(s, s->nresp); a.out[0] = L(s, s->resp_off);
    a.in[1] = L(s, s->paysum); a.out[1] = L(s, o0.poff);
    a.in[2] = L(s, s->nresp); a.out[2] = L(s, o0.off); a.addc[2] = TICK_MAX;
    a.list = s->resp_nodes; a.list_base = s->lo;
    launch_scan(s, a);
  }
  const bool need_tot = s->nj > 0 || q.inj_pay;      // only Joins and injected payloads can outgrow the outbox
  klaunch(s, KI_SET_CAP, k_set_cap, dim3(gnode(s)), dim3(TB), 0, d, s->nresp, o0.cap, o0.cnt, s->scan_tot, s->d_pin, need_tot ? ++s->pin_seq : 0u,
          s->rest2n);
  if (!need_tot) return KB_OK;
  const uint32_t* tot = s->h_pin;                    // written by k_set_cap through the host mapping
  { const int rc = wait_pin(s, s->pin_seq); if (rc) return rc; }
  const uint32_t pay_tot = tot[1], msg_tot = tot[2], resp_nodes = tot[4];
  if (msg_tot > o0.msg_cap || pay_tot > o0.pay_cap) { const int rc = grow_wave0(s, msg_tot, pay_tot); if (rc) return rc; }
  if (s->n_ext) { const int rc = round_size_exports(s, msg_tot, pay_tot); if (rc) return rc; }
  if (!resp_nodes) return KB_OK;
  if (!resp_overlap_on(s)) return launch_join_responses(s, q, resp_nodes, 0);
  // Around A2: A1 first, for the flags; every unflagged responder on the third stream, forked here
  // (its inputs are final) and joined ahead of k_tick_post; then the flagged responders on st, ahead of A2.  A
  // responder's records and ids go to offsets fixed by the scan above, so the order of service does not show.
  // Phase 2 is enqueued first on purpose: its grid then has the CUs to itself for most of its 0.3 ms while phase 1's
  // workgroups queue behind it, and the fold and A3 run nearly alone afterwards.  Phase 1 first and the fork behind
  // it was measured and is no faster than the serial order: phase 1 alone takes 0.10 ms, and phase 2 then runs its
  // whole length beside the fold and A3, 0.76 ms, and ends after them (profiles/r08a_resp_trace_phase1_first.json).
  launch_tick_scan(s, q);
  side_fork(s, 4);
  { const int rc = launch_join_responses(s, q, resp_nodes, 2); if (rc) return rc; }
  side_done(s, 4);
  q.resp_side = true;
  return launch_join_responses(s, q, resp_nodes, 1);
}

// 3. tick: A1, A2, the fold and the row fingerprints, with the exact A3 order (side work 2) beside the fold; side
// work 0, 1 and 2 join here, and side work 4 (the Join responses of the responders A2 cannot touch, when they were split
// around A2: round_wave0_regions, which then ran A1 already).  Then the injected records' emissions and the round's
// broadcast lists.  No host wait.
static int round_tick(kb_sim* s, Round& q) {
  Dev& d = s->d;
  const int32_t r = q.r;
  const uint32_t R = s->R, gn = gnode(s);
  OutBuf& o0 = s->ob[0];
  if (q.lat_fail) side_join(s, 1);
  if (!q.tick_scanned) launch_tick_scan(s, q);                                                               // A1; list the A2 nodes
  klaunch(s, KI_TICK_PRE, k_tick_pre, dim3(std::min<uint32_t>((R + 3) / 4, 1024)), dim3(256), 0, d, o0, s->bs, r, s->slow,
          (const uint32_t*)s->nresp);                                                                        // A2 per listed node
  // exact A3 order beside the fold: it reads what A2 left (member bits, stamps, instants, bounds) and writes only
  // the five keys and the bounds, which nothing else reads before k_tick_post; the fold and the row fingerprints
  // write checkpoints and fingerprints only
  if (d.tst) {
    side_fork(s, 2);
    const uint32_t kpl = a3_kpl(s->W, d.dbg);
    if (kpl == 2) klaunch_on(s, s->st2, KI_A3_EXACT, k_a3_exact<2>, dim3((R + 3) / 4), dim3(256), 0, d, s->ro.part, r);
    else if (kpl) klaunch_on(s, s->st2, KI_A3_EXACT, k_a3_exact<A3X_KPL>, dim3((R + 3) / 4), dim3(256), 0, d, s->ro.part, r);
    else klaunch_on(s, s->st2, KI_A3_EXACT, k_a3_exact<0>, dim3((R + 3) / 4), dim3(256), 0, d, s->ro.part, r);
    side_done(s, 2);
  }
  // every checkpoint the round's membership changes (broadcasts, A2) made stale is refolded
  if (d.uniform) klaunch(s, KI_FOLD, k_fold, dim3(((R + 63) / 64 + 3) / 4 * s->S), dim3(256), 0, d, FoldArgs{s->S});
  if (d.uniform) klaunch(s, KI_FP_ROWS, k_fp_rows, dim3((FP_LANES * R + TB - 1) / TB), dim3(TB), 0, d);
  side_join(s, 0);
  if (d.tst) side_join(s, 2);
  if (q.resp_side) side_join(s, 4);                    // k_tick_post appends to the outboxes the responses head
  klaunch(s, KI_TICK_POST, k_tick_post, dim3(gn), dim3(TB), 0, d, s->ro, o0, r);
  if (q.ninj) {                                        // the external peers' wave-0 emissions, after the tick's
    klaunch(s, KI_EVENTS, k_inject, dim3(1), dim3(64), 0, d, o0, (const XRec*)s->d_inj, q.ninj, (const uint32_t*)s->d_inj_ids);
    s->inj.clear(); s->inj_ids.clear();
  }
  {
    ScanArgs a = scan_args(s, R, s->scan_tot);
    a.narr = 2;
    a.in[0] = L(s, s->bs.join); a.out[0] = L(s, s->join_off);
    a.in[1] = L(s, s->bs.nfail); a.out[1] = L(s, s->fail_off);
    launch_scan(s, a);
  }
  klaunch(s, KI_BCAST_WRITE, k_bcast_write, dim3(gn), dim3(TB), 0, d, s->bs, (const uint32_t*)s->join_off,
          (const uint32_t*)s->fail_off, s->xf ? s->bjoin_loc : s->bjoin, s->xf ? s->bfail_loc : s->bfail);
  return KB_OK;
}

// 4. receive window: unicast waves.  Unsharded, the window has no host decision inside it, so with
// KB_WAVE_GRAPH=1 its ≈ 80 launches are one HIP graph, captured once per buffer generation and
// replayed each round: that removes host launch gaps in multi-round steps, but the benched one-round
// steps are GPU-bound and measured no faster, so it is off by default.
static int round_window(kb_sim* s, Round& q) {
  hipStream_t st = s->st;
  if (s->xf || s->debug_waves || !s->graph_on) return launch_waves(s, q.r);
  if (!s->wave_exec || s->wave_gen != s->buf_gen) {
    if (s->wave_exec) { (void)hipGraphExecDestroy(s->wave_exec); s->wave_exec = nullptr; }
    if (s->wave_graph) { (void)hipGraphDestroy(s->wave_graph); s->wave_graph = nullptr; }
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    s->capturing = true;                           // captured launches carry no profile events
    const int rc = launch_waves(s, -1);
    s->capturing = false;
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    HIPCHK(e);
    s->wave_graph = g;
    HIPCHK(hipGraphInstantiate(&s->wave_exec, g, nullptr, nullptr, 0));
    s->wave_gen = s->buf_gen;
  }
  HIPCHK(hipGraphLaunch(s->wave_exec, st));
  return KB_OK;
}

// The round's end: the agreement count, k_round_end, and the one host wait every round has: sharded, the all-gather
// of every shard's broadcast lists and error flag (gather_broadcasts); else the second pinned hand-off, k_round_end's
// counts and error flag in the host-mapped buffer (the stream then drains by itself).  The earlier rounds' profile
// events are read while this round runs.  Then the two drains (round_drain_*: blocking copies).
static int round_finish(kb_sim* s, Round& q) {
  Dev& d = s->d;
  const int32_t r = q.r;
  hipStream_t st = s->st;
  if (s->xf && !s->xf->allreduce_sum_u32(d.ctr + C_AGREE, 1, st)) { seterr(s->xf->error()); return KB_IO_ERROR; }
  klaunch(s, KI_ROUND_END, k_round_end, dim3(1), dim3(1), 0, d, r, (const uint32_t*)s->scan_tot, s->d_pin,
          s->xf ? 0u : ++s->pin_seq, s->rr);
  (void)hipEventRecord(q.er[1], st);
  s->krec.push_back(kb_sim::KRec{(int16_t)NKI, (int16_t)-1, q.er[0], q.er[1]});
  prof_resolve(s, q.krec0);
  uint32_t err = 0;
  if (s->xf) {
    const int rc = gather_broadcasts(s, &err);
    if (rc) return rc;
  } else {
    const int rc = wait_pin(s, s->pin_seq);
    if (rc) return rc;
    s->nj = s->h_pin[0]; s->nf = s->h_pin[1]; err = s->h_pin[2];
  }
  s->bj_total += s->nj; s->bf_total += s->nf;
  { const int rc = round_drain_exports(s); if (rc) return rc; }
  { const int rc = round_drain_probes(s, q.np, r); if (rc) return rc; }
  s->round = r + 1;
  return err_status(err);                            // shards: the flag of any rank
}

static int step_round(kb_sim* s) {
  Round q;
  q.r = s->round;
  q.krec0 = s->krec.size();
  s->cur_wave = -1;
  for (int k = 0; k < 2; ++k) {
    if (!s->ev_free.empty()) { q.er[k] = s->ev_free.back(); s->ev_free.pop_back(); }
    else (void)hipEventCreate(&q.er[k]);
  }
  (void)hipEventRecord(q.er[0], s->st);
  int rc = round_lifecycle(s, q);
  if (!rc) rc = round_broadcasts(s, q);
  if (!rc) rc = round_wave0_regions(s, q);
  if (!rc) rc = round_tick(s, q);
  if (!rc) rc = round_window(s, q);
  if (!rc) rc = round_finish(s, q);
  return rc;
}

// every shard of a group steps in its own thread; a failing shard aborts the others' rendezvous
static int group_step(kb_sim* g, uint32_t rounds) {
  const size_t W = g->shards.size();
  std::vector<int> rc(W, KB_OK);
  std::vector<std::string> err(W);
  g->hub->reset();
  std::vector<std::thread> th;
  for (size_t k = 0; k < W; ++k)
    th.emplace_back([&, k] {
      kb_sim* s = g->shards[k];
      (void)hipSetDevice(s->device);
      for (uint32_t q = 0; q < rounds && rc[k] == KB_OK; ++q) rc[k] = s->sp ? sp_step(s->sp, 1) : step_round(s);
      if (rc[k] == KB_OK && !s->sp && sync_st(s) != hipSuccess) { rc[k] = KB_IO_ERROR; g_err = "stream"; }
      if (rc[k] != KB_OK) { err[k] = g_err; g->hub->abort(); }
    });
  for (auto& t : th) t.join();
  int first = KB_OK;
  for (int pass = 0; pass < 2 && first == KB_OK; ++pass)     // the root cause first, released waiters last
    for (size_t k = 0; k < W && first == KB_OK; ++k)
      if (rc[k] != KB_OK && (pass == 1 || err[k].find("aborted by another shard") == std::string::npos)) {
        first = rc[k];
        seterr(err[k]);
      }
  return first;
}

extern "C" int kb_sim_step(kb_sim* s, uint32_t rounds) {
  if (!s) return KB_INVALID_ARGUMENT;
  if (s->probed) { seterr("the handle ran the fold probe (kb_sim_debug_fold): it cannot step"); return KB_INVALID_OPERATION; }
  if (is_group(s)) return group_step(s, rounds);
  if (s->sp) return sp_step(s->sp, rounds);
  (void)hipSetDevice(s->device);
  for (uint32_t k = 0; k < rounds; ++k) {
    int rc = step_round(s);
    if (rc) { if (s->xf) s->xf->abort(); return rc; }
  }
  HIPCHK(sync_st(s));                                  // synchronous: the rounds' work has completed on return
  return KB_OK;
}

// ---------------------------------------------------------------------------------- API surface
// Every entry point checks its arguments once and hands the call to route() (above); what the call does on one
// engine is a kb_ctl.h template, or an eng_* overload where the engines really differ.  Which calls go to every
// shard, to the owner of a row or to the first shard, and which merge: DESIGN.md "Host control plane".
static int chk(kb_sim* s, uint32_t node) { return (!s || node >= s->C) ? KB_INVALID_ARGUMENT : KB_OK; }
static int read_row(kb_sim* s, uint32_t node, std::vector<uint8_t>& rw) {   // canonical bytes (0 = not a member)
  std::vector<uint32_t> bw(s->d.NWR);
  rw.resize(s->C);
  HIPCHK(hipMemcpy(rw.data(), s->d.stamp + (size_t)node * s->W, s->C, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(bw.data(), s->d.bits + (size_t)node * s->d.NWR, 4ull * s->d.NWR, hipMemcpyDeviceToHost));
  for (uint32_t j = 0; j < s->C; ++j) if (!((bw[j >> 5] >> (j & 31)) & 1u)) rw[j] = 0;
  return KB_OK;
}

#include "kb_ctl.h"

// ---- the dense engine's hooks (kb_ctl.h; upload_segments and read_row above) -------------------------------
static int mark_all_dirty(kb_sim* s) {
  k_mark_all_dirty<<<(s->R + 255) / 256, 256, 0, s->st>>>(s->d);
  HIPCHK(hipStreamSynchronize(s->st));
  return KB_OK;
}
static void window_stale(kb_sim* s) { s->buf_gen++; }   // a captured receive window holds the old Dev and buffers
static int export_alloc(kb_sim* s) {
  s->d.xrec_cap = XREC_MIN; s->d.xids_cap = XIDS_MIN;   // grown per round (round_size_exports)
  HIPCHK(talloc(s, &s->d.xrec, s->d.xrec_cap)); HIPCHK(talloc(s, &s->d.xids, s->d.xids_cap));
  window_stale(s);
  return KB_OK;
}
static int row_fp(kb_sim* s, uint32_t node, uint32_t* fp) {
  if (ctl_chk_row(s, node)) return KB_INVALID_ARGUMENT;
  k_fp_one<<<1, 64, 0, s->st>>>(s->d, node);
  HIPCHK(hipMemcpyAsync(fp, s->d.fp + node, 4, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipStreamSynchronize(s->st));
  return KB_OK;
}
static int lat_column(kb_sim* s, uint32_t node, std::vector<uint16_t>& lat) {   // track_latency only
  if (!s->d.lat) return KB_OK;
  lat.resize(s->C);
  k_lat_column<<<(s->C + 255) / 256, 256, 0, s->st>>>(s->d, node, s->lat_col);
  HIPCHK(hipMemcpyAsync(lat.data(), s->lat_col, 2ull * s->C, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipStreamSynchronize(s->st));
  return KB_OK;
}

// ---- lifecycle: every shard applies the call to its replicated per-id facts; they take effect at the next round
extern "C" int kb_sim_start_node(kb_sim* s, uint32_t node) {
  if (chk(s, node)) return KB_INVALID_ARGUMENT;
  return route(s, R_ALL, node, [&](auto* e) { return ctl_start_node(e, node); });
}
extern "C" int kb_sim_stop_node(kb_sim* s, uint32_t node) {
  if (chk(s, node)) return KB_INVALID_ARGUMENT;
  return route(s, R_ALL, node, [&](auto* e) { return ctl_stop_node(e, node); });
}
extern "C" int kb_sim_restart_node(kb_sim* s, uint32_t node, uint32_t* new_node) {
  if (chk(s, node) || !new_node) return KB_INVALID_ARGUMENT;
  bool first = true;                                 // every shard allocates the same fresh id (replicated counter)
  return route(s, R_ALL, node, [&](auto* e) -> int {
    uint32_t to = 0;
    const int rc = ctl_restart_node(e, node, &to);
    if (rc) return rc;
    if (!first && to != *new_node) { seterr("shards allocated different fresh ids"); return KB_IO_ERROR; }
    *new_node = to; first = false;
    return KB_OK;
  });
}
extern "C" int kb_sim_is_running(kb_sim* s, uint32_t node, int* running) {
  if (chk(s, node) || !running) return KB_INVALID_ARGUMENT;
  return route(s, R_FIRST, node, [&](auto* e) { return ctl_is_running(e, node, running); });
}
extern "C" int kb_sim_ping_addrs(kb_sim* s, uint32_t node, const uint32_t* peers, size_t n) {
  if (chk(s, node) || (n && !peers)) return KB_INVALID_ARGUMENT;
  return route(s, R_ALL, node, [&](auto* e) { return ctl_ping_addrs(e, node, peers, n); });
}
extern "C" int kb_sim_set_identity(kb_sim* s, uint32_t node, const uint8_t* identity, size_t len) {
  if (chk(s, node) || len > MAXID || (len && !identity)) return KB_INVALID_ARGUMENT;
  return route(s, R_ALL, node, [&](auto* e) { return ctl_set_identity(e, node, identity, len); });
}
extern "C" int kb_sim_identity(kb_sim* s, uint32_t node, uint8_t* buf, size_t cap, size_t* len) {
  if (chk(s, node) || !len) return KB_INVALID_ARGUMENT;
  return route(s, R_FIRST, node, [&](auto* e) { return ctl_identity(e, node, buf, cap, len); });   // replicated per id
}
// ---- discovery (src/discovery.rs:30-89, src/kaboodle.rs:305-331) ----------------------------------
extern "C" int kb_sim_probe(kb_sim* s, const kb_wire_addr* prober) {
  if (!s || !prober) return KB_INVALID_ARGUMENT;
  return route(s, R_ALL, 0, [&](auto* e) { e->probe_q.push_back(*prober); return KB_OK; });
}
extern "C" int kb_sim_probe_responses(kb_sim* s, kb_probe_response* out, size_t cap, size_t* n) {
  if (!s || !n) return KB_INVALID_ARGUMENT;
  std::vector<kb_probe_response> all;                // every shard's responders, merged in canonical order
  route(s, R_ALL, 0, [&](auto* e) { all.insert(all.end(), e->presp.begin(), e->presp.end()); return KB_OK; });
  std::stable_sort(all.begin(), all.end(), [](const kb_probe_response& a, const kb_probe_response& b) {
    return a.round != b.round ? a.round < b.round : a.responder != b.responder ? a.responder < b.responder : a.probe < b.probe;
  });
  *n = all.size();
  if (!out) return KB_OK;
  if (cap < all.size()) return KB_CAPACITY;
  if (!all.empty()) memcpy(out, all.data(), all.size() * sizeof(kb_probe_response));
  return route(s, R_ALL, 0, [](auto* e) { e->presp.clear(); return KB_OK; });
}
// ---- external peers ------------------------------------------------------------------------
static_assert(sizeof(XRec) == sizeof(kb_unicast), "XRec mirrors kb_unicast");
extern "C" int kb_sim_set_external(kb_sim* s, uint32_t node) {
  if (chk(s, node)) return KB_INVALID_ARGUMENT;
  return route(s, R_ALL, node, [&](auto* e) { return ctl_set_external(e, node); });
}
extern "C" int kb_sim_inject(kb_sim* s, const kb_unicast* m, const uint32_t* ids) {
  if (!s || !m) return KB_INVALID_ARGUMENT;
  return route(s, R_ALL, 0, [&](auto* e) { return ctl_inject(e, m, ids); });
}
extern "C" int kb_sim_exported(kb_sim* s, kb_unicast* out, size_t cap, size_t* n, uint32_t* ids, size_t cap_ids, size_t* n_ids) {
  if (!s || !n || !n_ids) return KB_INVALID_ARGUMENT;
  std::vector<kb_unicast> all;
  std::vector<uint32_t> all_ids;
  route(s, R_ALL, 0, [&](auto* e) {
    for (const kb_unicast& u : e->xq) {
      kb_unicast v = u;
      v.pay_off = (uint32_t)all_ids.size();
      all_ids.insert(all_ids.end(), e->xq_ids.begin() + u.pay_off, e->xq_ids.begin() + u.pay_off + u.pay_len);
      std::sort(all_ids.begin() + v.pay_off, all_ids.end());   // a KnownPeers map has no order: ascending ids
      all.push_back(v);
    }
    return KB_OK;
  });
  std::stable_sort(all.begin(), all.end(), [](const kb_unicast& a, const kb_unicast& b) {
    return a.round != b.round ? a.round < b.round : a.wave != b.wave ? a.wave < b.wave : a.sender != b.sender ? a.sender < b.sender
                                                                                       : a.seq < b.seq; });
  *n = all.size(); *n_ids = all_ids.size();
  if (!out && !ids) return KB_OK;
  if (cap < all.size() || (!all_ids.empty() && (!ids || cap_ids < all_ids.size()))) { seterr("export buffer too small"); return KB_CAPACITY; }
  if (!all.empty()) memcpy(out, all.data(), all.size() * sizeof(kb_unicast));
  if (!all_ids.empty()) memcpy(ids, all_ids.data(), 4 * all_ids.size());
  return route(s, R_ALL, 0, [](auto* e) { e->xq.clear(); e->xq_ids.clear(); return KB_OK; });
}

extern "C" int kb_sim_broadcasts(kb_sim* s, kb_broadcast* out, size_t cap, size_t* n) {
  if (!s || !n) return KB_INVALID_ARGUMENT;
  return route(s, R_FIRST, 0, [&](auto* e) { return ctl_broadcasts(e, out, cap, n); });   // every shard holds the lists
}
extern "C" int kb_sim_fingerprint(kb_sim* s, uint32_t node, uint32_t* fp) {
  if (chk(s, node) || !fp) return KB_INVALID_ARGUMENT;
  return route(s, R_OWNER, node, [&](auto* e) { return row_fp(e, node, fp); });
}
// the census frame's hooks (kb_ctl.h): the engine's stream, its device fingerprints and running flags, and the
// refresh of the rows whose view changed since their fingerprint was last taken
static hipStream_t eng_stream(kb_sim* s) { return s->st; }
static const uint32_t* eng_fp(kb_sim* s) { return s->d.fp; }
static const uint8_t* eng_alive(kb_sim* s) { return s->d.alive; }
static int eng_refresh_fps(kb_sim* s) {
  if (s->R) k_fp_all<<<(s->R + 3) / 4, 256, 0, s->st>>>(s->d);
  HIPCHK(hipGetLastError());
  return KB_OK;
}
// all ids; 0 for non-running ids and for rows held by other shards
static int eng_fingerprints(kb_sim* s, uint32_t* fps) {
  k_fp_all<<<(s->R + 3) / 4, 256, 0, s->st>>>(s->d);
  std::vector<uint8_t> al(s->C);
  memset(fps, 0, 4ull * s->C);
  HIPCHK(hipMemcpyAsync(fps + s->lo, s->d.fp + s->lo, 4ull * s->R, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipMemcpyAsync(al.data(), s->d.alive, s->C, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipStreamSynchronize(s->st));
  for (uint32_t i = 0; i < s->C; ++i) if (!al[i]) fps[i] = 0;
  return KB_OK;
}
extern "C" int kb_sim_fingerprints(kb_sim* s, uint32_t* fps, size_t cap) {
  if (!s || !fps || cap < s->C) return KB_INVALID_ARGUMENT;
  if (!is_group(s)) return visit(s, [&](auto* e) { return eng_fingerprints(e, fps); });
  std::vector<uint32_t> part(s->C);
  memset(fps, 0, 4ull * s->C);
  return route(s, R_ALL, 0, [&](auto* e) {
    const int rc = eng_fingerprints(e, part.data());
    for (uint32_t j = e->lo; !rc && j < e->hi; ++j) fps[j] = part[j];
    return rc;
  });
}
static int eng_true_fingerprint(kb_sim* s, uint32_t* fp) {
  k_alive_bits<<<(s->d.NWR + 255) / 256, 256, 0, s->st>>>(s->d);
  k_truefp_part<<<TRUEFP_G, 256, 0, s->st>>>(s->d, s->d.tfpart);
  k_truefp_fin<<<1, 64, 0, s->st>>>(s->d, s->d.tfpart);
  HIPCHK(hipMemsetAsync(s->d.ctr + C_ALIVE, 0, 4, s->st));
  HIPCHK(hipMemcpyAsync(fp, s->d.truefp, 4, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipStreamSynchronize(s->st));
  return KB_OK;
}
extern "C" int kb_sim_true_fingerprint(kb_sim* s, uint32_t* fp) {
  if (!s || !fp) return KB_INVALID_ARGUMENT;
  return route(s, R_FIRST, 0, [&](auto* e) { return eng_true_fingerprint(e, fp); });
}
extern "C" int kb_sim_dump_row(kb_sim* s, uint32_t node, uint8_t* rw, size_t cap) {
  if (chk(s, node) || !rw || cap < s->C) return KB_INVALID_ARGUMENT;
  return route(s, R_OWNER, node, [&](auto* e) {
    std::vector<uint8_t> v;
    int rc = ctl_chk_row(e, node);
    if (!rc) rc = read_row(e, node, v);
    if (!rc) memcpy(rw, v.data(), s->C);
    return rc;
  });
}
extern "C" int kb_sim_peers(kb_sim* s, uint32_t node, uint32_t* peers, size_t cap, size_t* n) {
  if (chk(s, node) || !n) return KB_INVALID_ARGUMENT;
  return route(s, R_OWNER, node, [&](auto* e) { return ctl_peers(e, node, peers, cap, n); });
}
extern "C" int kb_sim_peer_states(kb_sim* s, uint32_t node, kb_peer_state* out, size_t cap, size_t* n) {
  if (chk(s, node) || !n) return KB_INVALID_ARGUMENT;
  return route(s, R_OWNER, node, [&](auto* e) { return ctl_peer_states(e, node, out, cap, n); });
}
// ---- event observers: a device snapshot here, a host snapshot on the sparse rows (eng_watch, eng_events) -------
static int eng_watch(kb_sim* s, uint32_t node) {
  if (ctl_chk_row(s, node)) return KB_INVALID_ARGUMENT;
  for (uint32_t w : s->watch_node) if (w == node) return KB_OK;      // one observer per node
  if (!s->ev_out) HIPCHK(talloc(s, &s->ev_out, 2ull * s->C + 4));
  uint32_t* snap = nullptr;
  HIPCHK(talloc(s, &snap, (size_t)s->d.NWR));
  HIPCHK(hipMemsetAsync(snap, 0, 4ull * s->d.NWR, s->st));          // attached empty, as in Kaboodle::new
  HIPCHK(hipStreamSynchronize(s->st));
  s->watch_node.push_back(node); s->watch_fp.push_back(0); s->watch_snap.push_back(snap);
  return KB_OK;
}
extern "C" int kb_sim_watch(kb_sim* s, uint32_t node) {
  if (chk(s, node)) return KB_INVALID_ARGUMENT;
  return route(s, R_OWNER, node, [&](auto* e) { return eng_watch(e, node); });
}
static int eng_events(kb_sim* s, uint32_t node, uint32_t* discovered, size_t cap_d, size_t* n_d, uint32_t* departed,
                      size_t cap_p, size_t* n_p, uint32_t* fp, int* fp_changed) {
  if (ctl_chk_row(s, node)) return KB_INVALID_ARGUMENT;
  size_t k = 0;
  while (k < s->watch_node.size() && s->watch_node[k] != node) ++k;
  if (k == s->watch_node.size()) { seterr("node is not watched (kb_sim_watch)"); return KB_INVALID_OPERATION; }
  const uint32_t* row = s->d.bits + (size_t)node * s->d.NWR;
  uint32_t ctr[3];
  k_events_diff<<<1, 1024, 0, s->st>>>(row, s->watch_snap[k], s->C, s->ev_out);
  k_fp_one<<<1, 64, 0, s->st>>>(s->d, node);
  HIPCHK(hipMemcpyAsync(ctr, s->ev_out + 2ull * s->C, 12, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipMemcpyAsync(fp, s->d.fp + node, 4, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipStreamSynchronize(s->st));
  *n_d = ctr[0]; *n_p = ctr[1];
  // the fingerprint batch rule (src/events.rs:103-122): only with a non-empty map, only on change
  *fp_changed = ctr[2] > 0 && *fp != s->watch_fp[k];
  const bool fit = (!ctr[0] || (discovered && cap_d >= ctr[0])) && (!ctr[1] || (departed && cap_p >= ctr[1]));
  if (!fit) {
    if (discovered || departed) { seterr("event buffer too small"); return KB_CAPACITY; }
    return KB_OK;                                                    // size query: nothing drained
  }
  if (ctr[0]) HIPCHK(hipMemcpyAsync(discovered, s->ev_out, 4ull * ctr[0], hipMemcpyDeviceToHost, s->st));
  if (ctr[1]) HIPCHK(hipMemcpyAsync(departed, s->ev_out + s->C, 4ull * ctr[1], hipMemcpyDeviceToHost, s->st));
  k_events_commit<<<(s->d.NWR + 255) / 256, 256, 0, s->st>>>(row, s->watch_snap[k], s->d.NWR);
  HIPCHK(hipStreamSynchronize(s->st));
  if (*fp_changed) s->watch_fp[k] = *fp;
  return KB_OK;
}
extern "C" int kb_sim_events(kb_sim* s, uint32_t node, uint32_t* discovered, size_t cap_d, size_t* n_d,
                             uint32_t* departed, size_t cap_p, size_t* n_p, uint32_t* fp, int* fp_changed) {
  if (chk(s, node) || !n_d || !n_p || !fp || !fp_changed) return KB_INVALID_ARGUMENT;
  return route(s, R_OWNER, node, [&](auto* e) {
    return eng_events(e, node, discovered, cap_d, n_d, departed, cap_p, n_p, fp, fp_changed); });
}
// the per-workgroup partial counters (d.sacc) folded into d.stats; the stream is idle afterwards
__global__ __launch_bounds__(256) void k_stats_fold(Dev d) {
  const uint32_t k = blockIdx.x;                   // one counter per workgroup
  unsigned long long t = 0;
  for (uint32_t q = threadIdx.x; q < NACC; q += blockDim.x) {
    unsigned long long& x = d.sacc[(size_t)q * NSTAT + k];
    t += x; x = 0;
  }
  t = block_sum(t);
  if (threadIdx.x == 0 && t) d.stats[k] += t;
}
static int fold_stats(kb_sim* s) {
  (void)hipSetDevice(s->device);
  k_stats_fold<<<NSTAT, 256, 0, s->st>>>(s->d);
  HIPCHK(hipStreamSynchronize(s->st));
  return KB_OK;
}
// the counters summed over the shards (a rank handle: over the mesh, a collective), replicated facts from one
extern "C" int kb_sim_stats(kb_sim* s, kb_stats* out) {
  if (!s || !out) return KB_INVALID_ARGUMENT;
  unsigned long long st[NSTAT] = {0};
  const int rc = route(s, R_ALL, 0, [&](auto* e) {
    unsigned long long v[NSTAT];
    const int rc = ctl_read_stats(e, v);
    for (int k = 0; !rc && k < NSTAT; ++k) st[k] += v[k];
    return rc;
  });
  return rc ? rc : route(s, R_FIRST, 0, [&](auto* e) { return ctl_stats_fill(e, st, out); });
}
// per id: alive, n, last_bcast, start_round; n and last_bcast only for the rows this handle holds
extern "C" int kb_sim_dump_scalars(kb_sim* s, int32_t* out, size_t cap) {
  if (!s || !out || cap < 4ull * s->C) return KB_INVALID_ARGUMENT;
  if (!is_group(s)) return visit(s, [&](auto* e) { return ctl_dump_scalars(e, out); });
  std::vector<int32_t> part(4ull * s->C);
  bool first = true;                                 // the per-id facts from the first shard, each row's from its shard
  return route(s, R_ALL, 0, [&](auto* e) {
    const int rc = ctl_dump_scalars(e, part.data());
    for (uint32_t i = 0; !rc && i < s->C; ++i)
      if ((i >= e->lo && i < e->hi) || first) memcpy(out + 4 * i, part.data() + 4 * i, 16);
    first = false;
    return rc;
  });
}
extern "C" int kb_sim_dump_suspects(kb_sim* s, uint32_t node, int32_t* out, size_t cap, size_t* n) {
  if (chk(s, node) || !n) return KB_INVALID_ARGUMENT;
  return route(s, R_OWNER, node, [&](auto* e) { return ctl_dump_suspects(e, node, out, cap, n); });
}
extern "C" int kb_sim_dump_curious(kb_sim* s, uint32_t node, int32_t* out, size_t cap, size_t* n) {
  if (chk(s, node) || !n) return KB_INVALID_ARGUMENT;
  return route(s, R_OWNER, node, [&](auto* e) { return ctl_dump_curious(e, node, out, cap, n); });
}
extern "C" uint32_t kb_fingerprint_of_set(const uint32_t* ids, size_t n, const uint8_t* identities, size_t id_stride,
                                          const uint8_t* id_lens) {
  h_crc_init();
  std::vector<uint32_t> v(ids, ids + n);
  std::sort(v.begin(), v.end());
  uint32_t reg = 0xFFFFFFFFu;
  char a[32];
  for (uint32_t id : v) {
    kb_format_addr(id, a, sizeof a);
    reg = h_crc_update(reg, (const uint8_t*)a, strlen(a));
    if (identities && id_lens) reg = h_crc_update(reg, identities + (size_t)id * id_stride, id_lens[id]);
  }
  return reg ^ 0xFFFFFFFFu;
}
// ---- kernel profile: per engine; a group answers with its first shard's (this handle's rows) --------------------
static int kt_kid(int kind) {
  return kind == KB_KT_ROWPASS ? KI_ROWPASS : kind == KB_KT_FOLD ? KI_FOLD : kind == KB_KT_RESP ? KI_RESP_WAVE
       : kind == KB_KT_PROC ? KI_PROC : -1;
}
// the stream is idle: every pending kernel record can be read
static void prof_flush(kb_sim* s) {
  (void)hipSetDevice(s->device);
  if (s->st) (void)hipStreamSynchronize(s->st);
  prof_resolve(s, s->krec.size());
}
static int eng_kernel_time(kb_sim* s, int kind, double* ms, uint64_t* launches) {
  prof_flush(s);
  if (kind == KB_KT_ROUND) { *ms = s->round_ms; *launches = s->round_launches; return KB_OK; }
  const int k = kt_kid(kind);
  if (k < 0) return KB_INVALID_ARGUMENT;
  *ms = s->k_ms[k]; *launches = s->k_n[k];
  return KB_OK;
}
extern "C" int kb_sim_kernel_time(kb_sim* s, int kind, double* ms, uint64_t* launches) {
  if (!s || !ms || !launches) return KB_INVALID_ARGUMENT;
  return route(s, R_FIRST, 0, [&](auto* e) { return eng_kernel_time(e, kind, ms, launches); });
}
static uint64_t stat_counter(kb_sim* s, int idx) {
  unsigned long long v = 0;
  if (fold_stats(s)) return 0;
  if (hipMemcpy(&v, s->d.stats + idx, 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return v;
}
static int eng_reset_kernel_time(kb_sim* s) {
  prof_flush(s);
  s->round_ms = 0; s->round_launches = 0;
  memset(s->k_ms, 0, sizeof s->k_ms); memset(s->k_wms, 0, sizeof s->k_wms); memset(s->k_n, 0, sizeof s->k_n);
  for (int k = 0; k < NKI; ++k) {                   // baselines of the device-side byte counters
    const int b = kbytes_stat(k);
    if (b >= 0) s->k_bytes0[b] = stat_counter(s, b);
  }
  return KB_OK;
}
extern "C" int kb_sim_reset_kernel_time(kb_sim* s) {
  if (!s) return KB_INVALID_ARGUMENT;
  return route(s, R_ALL, 0, [](auto* e) { return eng_reset_kernel_time(e); });
}
// algorithmic bytes a kernel moved since the last reset, counted in-kernel; the sparse rows count none
static int eng_kernel_bytes(kb_sim* s, int kind, uint64_t* bytes) {
  const int k = kt_kid(kind), b = k < 0 ? -1 : kbytes_stat(k);
  if (b < 0) return KB_INVALID_ARGUMENT;
  *bytes = stat_counter(s, b) - s->k_bytes0[b];
  return KB_OK;
}
static int eng_kernel_bytes(SpSim*, int, uint64_t* bytes) { *bytes = 0; return KB_INVALID_ARGUMENT; }
extern "C" int kb_sim_kernel_bytes(kb_sim* s, int kind, uint64_t* bytes) {
  if (!s || !bytes) return KB_INVALID_ARGUMENT;
  return route(s, R_FIRST, 0, [&](auto* e) { return eng_kernel_bytes(e, kind, bytes); });
}
extern "C" int kb_sim_set_profiling(kb_sim* s, int level) {
  if (!s || level < 0 || level > 2) return KB_INVALID_ARGUMENT;
  return route(s, R_ALL, 0, [&](auto* e) { e->prof_level = level; return KB_OK; });
}
// every kernel the rounds launched since the last reset: HIP-event time (sum and per delivery wave),
// launches, algorithmic bytes where counted in-kernel; kernels never launched are omitted
static int eng_kernel_breakdown(kb_sim* s, kb_kernel_time* out, size_t cap, size_t* n) {
  prof_flush(s);
  size_t c = 0;
  for (int k = 0; k < NKI; ++k) {
    if (!s->k_n[k]) continue;
    if (out && c < cap) {
      kb_kernel_time& o = out[c];
      memset(&o, 0, sizeof o);
      snprintf(o.name, sizeof o.name, "%s", KNAME[k]);
      o.ms = s->k_ms[k]; o.launches = s->k_n[k];
      const int b = kbytes_stat(k);
      o.bytes = b >= 0 ? stat_counter(s, b) - s->k_bytes0[b] : 0;
      o.has_bytes = b >= 0;
      for (int w = 0; w < KB_WAVE_SLOTS; ++w) o.wave_ms[w] = s->k_wms[k][w];
    }
    c++;
  }
  *n = c;
  return (out && cap < c) ? KB_CAPACITY : KB_OK;
}
extern "C" int kb_sim_kernel_breakdown(kb_sim* s, kb_kernel_time* out, size_t cap, size_t* n) {
  if (!s || !n) return KB_INVALID_ARGUMENT;
  return route(s, R_FIRST, 0, [&](auto* e) { return eng_kernel_breakdown(e, out, cap, n); });
}
// host waits on the device since creation (stream synchronisations and pinned hand-offs); for a
// group, the largest over its shards
extern "C" int kb_sim_host_syncs(kb_sim* s, uint64_t* n) {
  if (!s || !n) return KB_INVALID_ARGUMENT;
  *n = 0;
  return route(s, R_ALL, 0, [&](auto* e) { *n = std::max<uint64_t>(*n, e->host_syncs); return KB_OK; });
}
// OR of the PATH_* bits (kb_common.h) of the kernel variants that did work since creation (none on the sparse rows)
static int eng_debug_paths(kb_sim* s, uint32_t* mask) {
  HIPCHK(hipMemcpy(mask, s->d.ctr + C_PATHS, 4, hipMemcpyDeviceToHost));
  *mask |= s->host_paths;
  return KB_OK;
}
static int eng_debug_paths(SpSim*, uint32_t* mask) { *mask = 0; return KB_OK; }
extern "C" int kb_sim_debug_paths(kb_sim* s, uint32_t* mask) {
  if (!s || !mask) return KB_INVALID_ARGUMENT;
  *mask = 0;
  return route(s, R_ALL, 0, [&](auto* e) {
    uint32_t x = 0;
    const int rc = eng_debug_paths(e, &x);
    *mask |= x;
    return rc;
  });
}
// development counters (test surface; include/kaboodle_sim.h): the A3 scan's [0..2], the row-shard exchange's bytes
// [3..4], k_a3_exact's exits [5..9]; an in-process group's are summed over its shards; zeros on the sparse rows
static size_t debug_counters_n(size_t cap) { return cap >= 10 ? 10 : cap >= 5 ? 5 : 3; }
static int eng_debug_counters(kb_sim* t, uint64_t* out, size_t cap) {
  static_assert(S_A3CHUNKS == S_A3ROWS + 2 && S_A3XWIDE == S_A3X32 + 4, "the A3 counters are read as two blocks");
  const size_t n = debug_counters_n(cap);
  unsigned long long v[3], x[5];
  { const int rc = fold_stats(t); if (rc) return rc; }
  HIPCHK(hipMemcpy(v, t->d.stats + S_A3ROWS, sizeof v, hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; ++k) out[k] += v[k];
  if (n >= 5) { out[3] += t->xbytes_cross; out[4] += t->xbytes_all; }   // 0 unsharded
  if (n < 10) return KB_OK;
  HIPCHK(hipMemcpy(x, t->d.stats + S_A3X32, sizeof x, hipMemcpyDeviceToHost));
  for (int k = 0; k < 5; ++k) out[5 + k] += x[k];
  return KB_OK;
}
static int eng_debug_counters(SpSim*, uint64_t* out, size_t cap) { for (size_t k = 0; k < cap && k < 10; ++k) out[k] = 0; return KB_OK; }
extern "C" int kb_sim_debug_counters(kb_sim* s, uint64_t* out, size_t cap) {
  if (!s || !out || cap < 3) return KB_INVALID_ARGUMENT;
  for (size_t k = 0; k < debug_counters_n(cap); ++k) out[k] = 0;
  return route(s, R_ALL, 0, [&](auto* e) { return eng_debug_counters(e, out, cap); });
}
// the sparse layout's footprint, summed over the shards' rows (the largest row: the max)
static int eng_footprint(kb_sim*, uint64_t*, size_t) { seterr("not a KB_VARIANT_SPARSE_ROWS handle"); return KB_INVALID_OPERATION; }
extern "C" int kb_sim_sparse_footprint(kb_sim* s, uint64_t* out, size_t cap) {
  if (!s || !out) return KB_INVALID_ARGUMENT;
  uint64_t acc[6] = {0};
  const int rc = route(s, R_ALL, 0, [&](auto* e) {
    uint64_t t[6];
    const int rc = eng_footprint(e, t, cap);
    for (int k = 0; !rc && k < 6; ++k) acc[k] = k == 3 ? std::max(acc[k], t[k]) : acc[k] + t[k];
    return rc;
  });
  if (!rc) memcpy(out, acc, sizeof acc);
  return rc;
}


// ---- the fingerprint checkpoints as stored, and the fold probe (test surface) -------------
static bool fold_surface_ok(kb_sim* s) {             // dense, and no rank of a kb_sim_create_rank mesh
  if (kind_of(s).sparse) { seterr("dense handles only"); return false; }
  if (kind_of(s).rank) { seterr("not on a kb_sim_create_rank handle"); return false; }
  return true;
}
extern "C" int kb_sim_dump_checkpoints(kb_sim* s, uint32_t node, uint32_t* seg, uint64_t* stale, uint32_t* dirty,
                                       uint32_t* fp_cached) {
  if (!s) return KB_INVALID_ARGUMENT;
  if (!fold_surface_ok(s)) return KB_INVALID_OPERATION;
  if (chk(s, node) || !seg || !stale || !dirty || !fp_cached) return KB_INVALID_ARGUMENT;
  if (is_group(s)) s = owner(s, node);
  if (ctl_chk_row(s, node)) return KB_INVALID_ARGUMENT;
  (void)hipSetDevice(s->device);
  uint8_t dy = 0;
  HIPCHK(hipMemcpy(seg, s->d.segp + (size_t)node * NSEG, 8ull * NSEG, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(stale, s->d.sdirty + node, 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&dy, s->d.dirty + node, 1, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(fp_cached, s->d.fp + node, 4, hipMemcpyDeviceToHost));
  *dirty = dy;
  return KB_OK;
}

// the tick's thread-per-row fingerprint refresh alone (k_tick_post's), for the probe
__global__ void k_probe_thread_fp(Dev d) {
  const uint32_t i = d.lo + blockIdx.x * blockDim.x + threadIdx.x;
  if (i < d.hi && d.alive[i]) thread_refresh_fp(d, i);
}
// one shard's part of a probe: the listed rows it holds
static int fold_probe_shard(kb_sim* s, const kb_fold_probe* p, uint64_t* fold_bytes) {
  (void)hipSetDevice(s->device);
  const Dev& d = s->d;
  const uint32_t R = s->R, NWR = d.NWR;
  HIPCHK(hipStreamSynchronize(s->st));
  const uint64_t b0 = stat_counter(s, S_FOLDB);
  HIPCHK(hipMemset(d.alive, 0, s->C));
  HIPCHK(hipMemset(L(s, d.dirty), 0, R));
  HIPCHK(hipMemset(L(s, d.sdirty), 0, 8ull * R));
  for (uint32_t q = 0; q < p->nrows; ++q) {
    const uint32_t i = p->rows[q];
    const uint8_t run = p->running[q] ? 1 : 0, one = 1;
    HIPCHK(hipMemcpy(d.alive + i, &run, 1, hipMemcpyHostToDevice));          // per id: replicated on every shard
    if (i < s->lo || i >= s->hi) continue;
    HIPCHK(hipMemcpy(d.bits + (size_t)i * NWR, p->bits + (size_t)q * NWR, 4ull * NWR, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.segp + (size_t)i * NSEG, p->segp_in + (size_t)q * NSEG * 2, 8ull * NSEG, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.sdirty + i, p->stale + q, 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.dirty + i, &one, 1, hipMemcpyHostToDevice));
  }
  HIPCHK(hipDeviceSynchronize());
  const uint32_t tb = 256;
  if (p->path == KB_FOLD_TICK) {                     // the two launches of step_round's tick, with the split asked for
    const uint32_t S = p->split ? p->split : s->S;
    if (d.uniform) k_fold<<<dim3(((R + 63) / 64 + 3) / 4 * S), dim3(256), 0, s->st>>>(d, FoldArgs{S});
    if (d.uniform) k_fp_rows<<<dim3((FP_LANES * R + tb - 1) / tb), dim3(tb), 0, s->st>>>(d);
  } else if (p->path == KB_FOLD_FP_ALL) {
    k_fp_all<<<(R + 3) / 4, 256, 0, s->st>>>(d);
  } else if (p->path == KB_FOLD_FP_ONE) {
    for (uint32_t q = 0; q < p->nrows; ++q)
      if (p->rows[q] >= s->lo && p->rows[q] < s->hi) k_fp_one<<<1, 64, 0, s->st>>>(d, p->rows[q]);
  } else {
    k_probe_thread_fp<<<(R + tb - 1) / tb, tb, 0, s->st>>>(d);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->st));
  for (uint32_t q = 0; q < p->nrows; ++q) {
    const uint32_t i = p->rows[q];
    if (i < s->lo || i >= s->hi) continue;
    uint8_t dy = 0;
    HIPCHK(hipMemcpy(p->segp_out + (size_t)q * NSEG * 2, d.segp + (size_t)i * NSEG, 8ull * NSEG, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(p->stale_out + q, d.sdirty + i, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&dy, d.dirty + i, 1, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(p->fp_out + q, d.fp + i, 4, hipMemcpyDeviceToHost));
    p->dirty_out[q] = dy;
  }
  *fold_bytes += stat_counter(s, S_FOLDB) - b0;
  return KB_OK;
}
extern "C" int kb_sim_debug_fold(kb_sim* s, const kb_fold_probe* p) {
  if (!s || !p) return KB_INVALID_ARGUMENT;
  if (!fold_surface_ok(s)) return KB_INVALID_OPERATION;
  kb_sim* h = is_group(s) ? s->shards[0] : s;
  if (s->cfg.initial_nodes != 0 || h->round != 0) {
    seterr("the fold probe needs a handle created with initial_nodes = 0 that has not stepped"); return KB_INVALID_OPERATION;
  }
  if (p->path > KB_FOLD_THREAD || p->split > 64 || (p->split & (p->split - 1)) || !p->nrows || !p->rows || !p->running ||
      !p->bits || !p->stale || !p->segp_in || !p->segp_out || !p->stale_out || !p->dirty_out || !p->fp_out || !p->fold_bytes) {
    seterr("fold probe: path, split (a power of two up to 64, or 0) or a null array"); return KB_INVALID_ARGUMENT;
  }
  const uint32_t C = s->C, NWR = h->d.NWR;
  for (uint32_t q = 0; q < p->nrows; ++q) {
    if (p->rows[q] >= C || (q && p->rows[q] <= p->rows[q - 1])) { seterr("fold probe: rows are ascending ids below the capacity"); return KB_INVALID_ARGUMENT; }
    if (p->path == KB_FOLD_THREAD && h->d.uniform && p->stale[q]) { seterr("fold probe: the thread path needs fresh checkpoints on uniform identities"); return KB_INVALID_ARGUMENT; }
    const uint32_t* b = p->bits + (size_t)q * NWR;
    for (uint32_t w = C / 32; w < NWR; ++w)
      if (w * 32 >= C ? b[w] != 0 : (b[w] >> (C & 31)) != 0) { seterr("fold probe: a member bit at an id >= capacity"); return KB_INVALID_ARGUMENT; }
    // the kernels index Z^cnt tables of capacity + 2 entries by the counts they combine: what the fresh checkpoints
    // claim plus what the stale segments hold must stay a member count of this capacity
    uint64_t total = 0;
    const uint32_t wps = NWR / NSEG;                 // bitset words per segment
    for (uint32_t k = 0; k < (uint32_t)NSEG && h->d.uniform; ++k) {
      if (!((p->stale[q] >> k) & 1ull)) { total += p->segp_in[((size_t)q * NSEG + k) * 2 + 1]; continue; }
      for (uint32_t w = k * wps; w < (k + 1) * wps; ++w) total += (uint32_t)__builtin_popcount(b[w]);
    }
    if (total > C) { seterr("fold probe: the checkpoints' member counts exceed the capacity"); return KB_INVALID_ARGUMENT; }
  }
  s->probed = true;                                  // no round after a probe: its rows are no simulator state
  *p->fold_bytes = 0;
  std::vector<kb_sim*> one{s};
  for (kb_sim* t : is_group(s) ? s->shards : one) {
    t->probed = true;
    const int rc = fold_probe_shard(t, p, p->fold_bytes);
    if (rc) return rc;
  }
  return KB_OK;
}

// ---- the censuses' shared host frame ------------------------------------------------------------------------
#include "kb_censusframe.h"
#include "kb_bitpass.h"

// ---- the view census (include/kaboodle_census.h) ----------------------------------------------------------
#include "kb_census.h"

// ---- the reciprocity census (include/kaboodle_reciprocity.h) ---------------------------------------------
#include "kb_recip.h"

// ---- the fingerprint-class census (include/kaboodle_classes.h) -------------------------------------------
#include "kb_classes.h"

// ---- the latency census (include/kaboodle_latency.h) ------------------------------------------------------
#include "kb_latcensus.h"

// ---- the contact-age census (include/kaboodle_age.h) -------------------------------------------------------
#include "kb_agecensus.h"

// ---- the view-delta census (include/kaboodle_delta.h) -------------------------------------------------------
#include "kb_delta.h"

// ---- the island census (include/kaboodle_islands.h) ---------------------------------------------------------
#include "kb_islands.h"

// ---- the gap list and the holders query (include/kaboodle_gaps.h) -------------------------------------------
#include "kb_gaps.h"

// ---- snapshot and restore (include/kaboodle_snapshot.h) ----------------------------------------------------
#include "kb_snapshot.h"
