// kb_latcensus.h — the latency census (include/kaboodle_latency.h): per id how many observers hold
// a first-hand latency of it and their sum, minimum and maximum; per row how many of its entries are measured and
// their sum; a histogram of all measured values; and the cells that hold a value under a clear member bit.
// Included at the end of kb_sim.hip; reads the dense engine's state, writes only its own scratch.
//
// One streaming pass over the latency table (Dev::lat, peer-major [W][lat_stride(R)] u16).  The table is
// contiguous along rows, so a lane owns LC_LANE_ROWS = 8 consecutive rows and takes one 16-byte load per peer: a
// wave reads 1 KiB contiguous per peer, a workgroup's 4 waves 4 KiB (a tile of 2,048 rows).  A workgroup walks a
// slab of LC_SLAB = 512 peers; LC_U = 8 peers' loads are issued before the first is used.
//
// The member mask.  A lane needs bit j of each of its 8 rows for every peer j of the slab.  The bits are row-major
// ([rows][W/32]), so a row's bits of a slab are one run of slab/8 bytes out of the row, fetched in 64-byte
// sectors: a 32-peer slab takes 4 of every 64 bytes fetched, 64 B per row per 32 peers = 2 B of bit traffic per
// 2-byte cell (the kernel's traffic doubles); a 128-peer slab (one 16-byte load per row) 64 B per 128 cells =
// +25 %; a 512-peer slab uses the whole sector, 64 B per 512 cells = +6 %.  The slab is 512 peers, walked as four
// sub-slabs of LC_SUB = 128: one 16-byte load per row each (32 registers of bits per lane, not 128), the sector's
// three later reads served by the cache that holds it from the first.
//
// Most of a real table is None (an observer measures the peers it pinged itself), so a peer whose 1 KiB holds no
// value in the whole wave costs four ANDs, a compare and a ballot.  Otherwise the lane classifies its 8 cells,
// adds them to its rows' (count, sum) registers, and the wave reduces count, sum, min, max and the orphan count
// by DPP (kb_device.h); the histogram is reduced by ballots, one per distinct bucket among the counting lanes.
// One lane adds the wave's results to the workgroup's LDS words; global atomics are issued once per workgroup:
// per peer of the slab, per histogram bucket, per row (DESIGN.md §3 "Same-address atomics").
//
// Widths.  The partial sums are u32 inside a workgroup's tile and u64 everywhere across tiles: a tile is
// LC_TILE_ROWS = 2,048 rows x LC_SLAB = 512 peers, so a peer's sum over the tile is at most 2,048 x 65,534 < 2^27,
// a histogram bucket at most 2^20; a lane keeps a row's count and sum over a sub-slab in one word (at most 128 and
// 128 x 65,534 < 2^23: 8 + 24 bits) and adds them to the row's global words after each sub-slab (the static_asserts
// below; a u32 sum would hold up to 65,536 rows).  Per-id sums, per-row sums and the histogram are u64 in global memory.
#pragma once
#include "../../include/kaboodle_latency.h"

namespace kb {

constexpr uint32_t LC_LANE_ROWS = 8;              // rows per lane: one 16-byte load per peer
constexpr uint32_t LC_WAVE_ROWS = 64 * LC_LANE_ROWS;
constexpr uint32_t LC_TILE_ROWS = 4 * LC_WAVE_ROWS;   // rows per workgroup (4 waves)
constexpr uint32_t LC_SLAB = 512;                 // peers per workgroup
constexpr uint32_t LC_SUB = 128;                  // peers per member-bit load (16 bytes of a bit row)
constexpr uint32_t LC_U = 8;                      // peers per batch (16-byte loads in flight per lane)
constexpr uint32_t LC_HEAD = KB_LAT_HIST + 1;     // summary words: the histogram, then the orphans
static_assert((uint64_t)LC_TILE_ROWS * (LAT_NONE - 1u) < (1ull << 32), "a peer's sum over a tile is u32");
static_assert((uint64_t)LC_SUB * (LAT_NONE - 1u) < (1ull << 24) && LC_SUB < 256, "a row's count and sum over a sub-slab share a word");
static_assert(LC_WAVE_ROWS < (1u << 16), "a wave's count and orphan count share a word");

struct LcArgs {
  const uint16_t* lat;                            // [>= C][RS] peer-major
  const uint32_t* bits;                           // [R][NWR] member bits of the local rows
  const uint8_t* alive;                           // [R] the local rows' running flags
  uint32_t R, RS, C, NWR;                         // rows, lat_stride(R), ids, bit words per row
  unsigned long long* head;                       // [LC_HEAD] histogram, orphans (zeroed)
  unsigned long long* sum;                        // [C] (zeroed)
  unsigned long long* rsum;                       // [RS] (zeroed)
  uint32_t* mb; uint32_t* mx; uint32_t* rcnt;     // [C], [C], [RS] (zeroed)
  uint32_t* mn;                                   // [C] (all ones)
};

// grid (ceil(C / 512) peer slabs, ceil(RS / 2048) row tiles), 256 threads
__global__ __launch_bounds__(256) void k_lat_census(LcArgs a) {
  __shared__ uint32_t pc[LC_SLAB], ps[LC_SLAB], pmn[LC_SLAB], pmx[LC_SLAB], lh[LC_HEAD];
  for (uint32_t k = threadIdx.x; k < LC_SLAB; k += 256) { pc[k] = 0; ps[k] = 0; pmn[k] = 0xFFFFFFFFu; pmx[k] = 0; }
  if (threadIdx.x < LC_HEAD) lh[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t l = lane();
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t g0 = blockIdx.y * LC_TILE_ROWS + wv * LC_WAVE_ROWS + l * LC_LANE_ROWS;   // the lane's first local row
  // RS is a multiple of 8: a lane's 8 rows are all inside the table's columns or all past them.  The padding rows
  // R .. RS-1 hold None by construction; neither their running flag nor their bits exist, and neither is read.
  const bool in = g0 < a.RS;
  uint32_t am = 0;                                // the lane's running rows
  if (in) {
#pragma unroll
    for (uint32_t u = 0; u < LC_LANE_ROWS; ++u) if (g0 + u < a.R && a.alive[g0 + u]) am |= 1u << u;
  }
  const uint32_t j_begin = blockIdx.x * LC_SLAB;
  const uint32_t j_end = a.C - j_begin > LC_SLAB ? j_begin + LC_SLAB : a.C;   // never past C: the padding columns are not read
  uint32_t ra[LC_LANE_ROWS] = {};                 // the rows' (count << 24 | sum) over a sub-slab
  if (__ballot(am != 0)) {                        // a wave without a running row reads nothing
    const uint32_t gl = in ? g0 : 0;              // a lane past the table re-reads group 0; am == 0 masks it off
    const char* lat0 = reinterpret_cast<const char*>(a.lat);
    const uint32_t loff = gl * 2u;                // the lane's bytes into a column: a uniform base plus a 32-bit offset
    const size_t cbytes = 2ull * a.RS;
    const uint4* brow = reinterpret_cast<const uint4*>(a.bits);
    const size_t nw4 = a.NWR >> 2;
#pragma unroll 1
    for (uint32_t j0 = j_begin; j0 < j_end; j0 += LC_SUB) {
      uint4 bw[LC_LANE_ROWS];                     // bits j0 .. j0+127 of the lane's running rows
#pragma unroll
      for (uint32_t u = 0; u < LC_LANE_ROWS; ++u)
        bw[u] = (am >> u) & 1u ? brow[(size_t)(gl + u) * nw4 + (j0 >> 7)] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll 1
      for (uint32_t q = 0; q < 4 && j0 + 32 * q < j_end; ++q) {
        uint32_t mw[LC_LANE_ROWS];                // the word holding peers j0 + 32q .. + 31
#pragma unroll
        for (uint32_t u = 0; u < LC_LANE_ROWS; ++u) mw[u] = q == 0 ? bw[u].x : q == 1 ? bw[u].y : q == 2 ? bw[u].z : bw[u].w;
#pragma unroll 1
        for (uint32_t c0 = 0; c0 < 32; c0 += LC_U) {
          const uint32_t jb = j0 + 32 * q + c0;
          if (jb >= j_end) break;
          uint4 v[LC_U];
#pragma unroll
          for (uint32_t t = 0; t < LC_U; ++t) {   // every load of the batch before its first use
            const uint32_t jj = jb + t < j_end ? jb + t : j_end - 1;
            v[t] = *reinterpret_cast<const uint4*>(lat0 + (size_t)jj * cbytes + loff);
          }
          uint32_t hot = 0;                       // the batch's peers with a value in a running row of this wave
#pragma unroll
          for (uint32_t t = 0; t < LC_U; ++t) {
            const bool any = am && (v[t].x & v[t].y & v[t].z & v[t].w) != 0xFFFFFFFFu;
            if (__ballot(any) && jb + t < j_end) hot |= 1u << t;
          }
          hot = (uint32_t)__builtin_amdgcn_readfirstlane((int)hot);
          while (hot) {                           // wave-uniform: EXEC stays whole for the DPP reductions
            const uint32_t t = (uint32_t)__builtin_ctz(hot);
            hot &= hot - 1;
            uint4 x = v[0];
#pragma unroll
            for (uint32_t k = 1; k < LC_U; ++k) if (t == k) x = v[k];
            const uint32_t bit = c0 + t, jl = jb + t - j_begin;
            const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
            uint32_t c = 0, s = 0, mn = 0xFFFFFFFFu, mx = 0, o = 0;
#pragma unroll
            for (uint32_t u = 0; u < LC_LANE_ROWS; ++u) {
              // 0 / 1 words and masks, no lane-mask compares: eight cells' worth of those would not fit the SGPRs
              const uint32_t val = (u & 1u) ? xs[u >> 1] >> 16 : xs[u >> 1] & 0xFFFFu;
              const uint32_t nn = ((val + 1u) >> 16) ^ 1u;           // val != LAT_NONE
              const uint32_t mem = (mw[u] >> bit) & 1u;              // 0 for a row that is not running
              const uint32_t cnt = nn & mem;
              const uint32_t cm = 0u - cnt, cv = val & cm;           // the value where the cell counts, else 0
              c += cnt; s += cv; o += nn & ~mem & (am >> u);
              mn = min(mn, val | ~cm);
              mx = max(mx, cv);
              ra[u] += cv + (cnt << 24);
              // the histogram: one ballot per distinct bucket among the counting lanes
              const uint32_t b = 32u - (uint32_t)__clz((int)val);    // 0 for 0, floor(log2 v) + 1 otherwise
              unsigned long long act = __ballot(cnt != 0);
              while (act) {
                const uint32_t b0 = rdl(b, __builtin_ctzll(act));
                const unsigned long long same = __ballot(cnt != 0 && b == b0);
                if (l == 0) atomicAdd(&lh[b0], (uint32_t)__popcll(same));
                act &= ~same;
              }
            }
            const uint32_t co = wave_sum(c | (o << 16));             // <= 512 each
            if (co) {
              const uint32_t ws = wave_sum(s), wmn = wave_min(mn), wmx = wave_max(mx);
              if (l == 0) {
                if (co & 0xFFFFu) {
                  atomicAdd(&pc[jl], co & 0xFFFFu); atomicAdd(&ps[jl], ws);
                  atomicMin(&pmn[jl], wmn); atomicMax(&pmx[jl], wmx);
                }
                if (co >> 16) atomicAdd(&lh[KB_LAT_HIST], co >> 16);
              }
            }
          }
        }
      }
      // a counting cell's row is running, so g0 + u < R
#pragma unroll
      for (uint32_t u = 0; u < LC_LANE_ROWS; ++u) {
        if (!ra[u]) continue;
        atomicAdd(&a.rcnt[g0 + u], ra[u] >> 24); atomicAdd(&a.rsum[g0 + u], (unsigned long long)(ra[u] & 0xFFFFFFu));
        ra[u] = 0;
      }
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < LC_SLAB; k += 256) {
    if (!pc[k]) continue;                         // set only for peers < j_end
    const uint32_t j = j_begin + k;
    atomicAdd(&a.mb[j], pc[k]); atomicAdd(&a.sum[j], (unsigned long long)ps[k]);
    atomicMin(&a.mn[j], pmn[k]); atomicMax(&a.mx[j], pmx[k]);
  }
  if (threadIdx.x < LC_HEAD && lh[threadIdx.x]) atomicAdd(&a.head[threadIdx.x], (unsigned long long)lh[threadIdx.x]);
}

}  // namespace kb

// ---- host side -------------------------------------------------------------------------------------------
// the scratch of one pass (a.C, a.RS set): all but the minima is cleared before every pass, the minima set to all ones
static void lc_lay(Carve& c, kb::LcArgs& a) {
  c.zero_from();
  a.head = c.take<unsigned long long>(kb::LC_HEAD); a.sum = c.take<unsigned long long>(a.C); a.rsum = c.take<unsigned long long>(a.RS);
  a.mb = c.take<uint32_t>(a.C); a.mx = c.take<uint32_t>(a.C); a.rcnt = c.take<uint32_t>(a.RS);
  c.zero_to();
  a.mn = c.take<uint32_t>(a.C);
}

// a census being put together: the ids' and rows' arrays, added to shard by shard
struct LcPart {
  std::vector<uint32_t> mb, mn, mx, rcnt;
  std::vector<uint64_t> sum, rsum;
  uint64_t head[kb::LC_HEAD] = {};
  uint32_t observers = 0;
  double ms = 0;
};
static void lc_part_init(LcPart& p, size_t n_ids, size_t n_rows) {
  p.mb.assign(n_ids, 0); p.mn.assign(n_ids, KB_CENSUS_NONE); p.mx.assign(n_ids, 0); p.sum.assign(n_ids, 0);
  p.rcnt.assign(n_rows, 0); p.rsum.assign(n_rows, 0);
}

// The pass over a.lat / a.bits / a.alive with the scratch laid out in `c` by lc_lay, on stream st; its results join
// `p`, the rows' at index lo onwards.
static int lc_exec(const Carve& c, const kb::LcArgs& a, hipStream_t st, uint32_t lo, bool want_rows, LcPart& p) {
  const uint32_t C = a.C, R = a.R;
  CsTimer tm;
  if (!tm.start(st)) { seterr("latency census: events"); return KB_IO_ERROR; }
  HIPCHK(hipMemsetAsync(c.zero_ptr(), 0, c.zero_bytes(), st));
  HIPCHK(hipMemsetAsync(a.mn, 0xFF, 4ull * C, st));
  k_lat_census<<<dim3((C + kb::LC_SLAB - 1) / kb::LC_SLAB, (a.RS + kb::LC_TILE_ROWS - 1) / kb::LC_TILE_ROWS), 256, 0, st>>>(a);
  tm.stop(st);
  HIPCHK(hipGetLastError());
  unsigned long long head[kb::LC_HEAD];
  std::vector<uint32_t> mb, mn, mx, rcnt;
  std::vector<uint64_t> sum, rsum;
  std::vector<uint8_t> alive;
  HIPCHK(hipMemcpyAsync(head, a.head, sizeof head, hipMemcpyDeviceToHost, st));
  HIPCHK(fetch(mb, a.mb, C, st));
  HIPCHK(fetch(mn, a.mn, C, st));
  HIPCHK(fetch(mx, a.mx, C, st));
  HIPCHK(fetch(sum, a.sum, C, st));
  HIPCHK(fetch(alive, a.alive, R, st));
  HIPCHK(fetch(rcnt, a.rcnt, want_rows ? R : 0, st));
  HIPCHK(fetch(rsum, a.rsum, want_rows ? R : 0, st));
  HIPCHK(hipStreamSynchronize(st));
  p.ms += tm.ms();
  for (uint32_t k = 0; k < kb::LC_HEAD; ++k) p.head[k] += head[k];
  for (uint32_t j = 0; j < C; ++j) {
    p.mb[j] += mb[j]; p.sum[j] += sum[j];
    p.mn[j] = std::min(p.mn[j], mn[j]); p.mx[j] = std::max(p.mx[j], mx[j]);
  }
  for (uint32_t k = 0; k < R; ++k) p.observers += alive[k] != 0;
  if (want_rows) for (uint32_t k = 0; k < R; ++k) { p.rcnt[lo + k] = rcnt[k]; p.rsum[lo + k] = rsum[k]; }
  return KB_OK;
}

// the O(ids) reductions of the summary, on the host
static void lc_summary(const LcPart& p, int32_t round, kb_lat_census* out) {
  memset(out, 0, sizeof *out);
  out->round = round;
  out->observers = p.observers;
  out->min_ms = KB_CENSUS_NONE; out->max_peer = KB_CENSUS_NONE;
  for (size_t j = 0; j < p.mb.size(); ++j) {
    if (!p.mb[j]) continue;
    out->measured += p.mb[j]; out->sum_ms += p.sum[j]; out->measured_ids++;
    out->min_ms = std::min(out->min_ms, p.mn[j]);
    if (out->max_peer == KB_CENSUS_NONE || p.mx[j] > out->max_ms) { out->max_peer = (uint32_t)j; out->max_ms = p.mx[j]; }
  }
  for (uint32_t k = 0; k < KB_LAT_HIST; ++k) out->hist[k] = p.head[k];
  out->orphans = p.head[KB_LAT_HIST];
}
static void lc_deliver(const LcPart& p, uint32_t* measured_by, uint64_t* sum_ms, uint32_t* min_ms, uint32_t* max_ms,
                       uint32_t* measured, uint64_t* row_sum_ms) {
  deliver(measured_by, p.mb); deliver(sum_ms, p.sum); deliver(min_ms, p.mn); deliver(max_ms, p.mx);
  deliver(measured, p.rcnt); deliver(row_sum_ms, p.rsum);
}

// one leaf's pass (route() hands every shard of a group here in turn)
static int lc_leaf(kb_sim* s, bool want_rows, LcPart& p) {
  (void)hipSetDevice(s->device);
  const Dev& d = s->d;
  kb::LcArgs a{};
  a.lat = d.lat; a.bits = d.bits + (size_t)s->lo * d.NWR; a.alive = d.alive + s->lo;   // d.bits is biased by -lo rows
  a.R = s->R; a.RS = lat_stride(s->R); a.C = s->C; a.NWR = d.NWR;
  auto lay = [&](Carve& c) { lc_lay(c, a); };
  if (!s->lc_buf) HIPCHK(talloc(s, &s->lc_buf, carve_bytes(lay) / 4));
  const Carve c = carve(s->lc_buf, lay);
  return lc_exec(c, a, s->st, s->lo, want_rows, p);
}
static int lc_leaf(SpSim*, bool, LcPart&) { return KB_INVALID_OPERATION; }   // not reached: census_gate refuses sparse rows

extern "C" int kb_sim_latency_census(kb_sim* s, kb_lat_census* out, uint32_t* measured_by, uint64_t* sum_ms, uint32_t* min_ms,
                                     uint32_t* max_ms, size_t cap_ids, uint32_t* measured, uint64_t* row_sum_ms, size_t cap_rows) {
  if (!s) return KB_INVALID_ARGUMENT;
  { const int rc = census_caps("kb_sim_latency_census", out, any_of(measured_by, sum_ms, min_ms, max_ms), cap_ids, s->C,
                               any_of(measured, row_sum_ms), cap_rows, s->C); if (rc) return rc; }
  { const int rc = census_gate(s, "kb_sim_latency_census", {"", "keep no latency table", nullptr}); if (rc) return rc; }
  if (!s->cfg.track_latency) { seterr("kb_sim_latency_census: the handle was created without track_latency"); return KB_INVALID_OPERATION; }
  LcPart p;
  lc_part_init(p, s->C, s->C);
  const bool want_rows = measured || row_sum_ms;
  int32_t round = 0;
  { const int rc = route(s, R_ALL, 0, [&](auto* e) { return lc_leaf(e, want_rows, p); }); if (rc) return rc; }
  { const int rc = route(s, R_FIRST, 0, [&](auto* e) { round = e->round; return KB_OK; }); if (rc) return rc; }
  s->census_ms[CM_LAT] = p.ms;
  lc_summary(p, round, out);
  lc_deliver(p, measured_by, sum_ms, min_ms, max_ms, measured, row_sum_ms);
  return KB_OK;
}

extern "C" int kb_sim_latency_census_device_ms(kb_sim* s, double* ms) { return census_ms_get(s, CM_LAT, ms); }

extern "C" int kb_latency_census_of(int device, const uint16_t* lat, const uint8_t* member, const uint8_t* running, size_t n_ids,
                                    size_t n_rows, kb_lat_census* out, uint32_t* measured_by, uint64_t* sum_ms, uint32_t* min_ms,
                                    uint32_t* max_ms, size_t cap_ids, uint32_t* measured, uint64_t* row_sum_ms, size_t cap_rows) {
  { const int rc = census_caps("kb_latency_census_of", out, any_of(measured_by, sum_ms, min_ms, max_ms), cap_ids, n_ids,
                               any_of(measured, row_sum_ms), cap_rows, n_rows); if (rc) return rc; }
  if (n_ids && n_rows && (!lat || !member || !running)) return KB_INVALID_ARGUMENT;
  if (n_ids > (1u << 24) || n_rows > (1u << 26)) { seterr("kb_latency_census_of: more than 2^24 ids or 2^26 rows"); return KB_CAPACITY; }
  std::vector<uint32_t> hb;                         // the member bits and running flags as uploaded: they outlive the stream
  std::vector<uint8_t> ha;
  OfScope o;
  { const int rc = o.open(device, "kb_latency_census_of"); if (rc) return rc; }
  LcPart p;
  lc_part_init(p, n_ids, n_rows);
  if (n_ids && n_rows) {
    // the layout of a handle: columns of lat_stride(rows) cells, bit rows of W/32 words (W: whole 8192-id steps)
    const uint32_t C = (uint32_t)n_ids, R = (uint32_t)n_rows, RS = lat_stride(R), NWR = (C + 8191) / 8192 * 8192 / 32;
    hb.assign((size_t)R * NWR, 0u);
    for (size_t i = 0; i < R; ++i)
      for (size_t j = 0; j < C; ++j) if (member[i * C + j]) hb[i * NWR + (j >> 5)] |= 1u << (j & 31);
    ha.resize(R);
    for (size_t i = 0; i < R; ++i) ha[i] = running[i] != 0;
    kb::LcArgs a{};
    a.R = R; a.RS = RS; a.C = C; a.NWR = NWR;
    uint16_t* dl = nullptr; uint32_t* db = nullptr; uint8_t* da = nullptr;
    auto lay = [&](Carve& c) {                      // the table and the bit rows (16-byte loads), the flags, the scratch
      dl = c.take<uint16_t>((size_t)C * RS, 16); db = c.take<uint32_t>((size_t)R * NWR, 16); da = c.take<uint8_t>(R);
      lc_lay(c, a);
    };
    { const int rc = dev_reserve(&o.buf, &o.cap, carve_bytes(lay), "kb_latency_census_of: device allocation failed"); if (rc) return rc; }
    const Carve c = carve(o.buf, lay);
    a.lat = dl; a.bits = db; a.alive = da;
    HIPCHK(hipMemsetAsync(dl, 0xFF, 2ull * C * RS, o.st));                             // the padding rows: None
    HIPCHK(hipMemcpy2DAsync(dl, 2ull * RS, lat, 2ull * R, 2ull * R, C, hipMemcpyHostToDevice, o.st));
    HIPCHK(hipMemcpyAsync(db, hb.data(), 4ull * R * NWR, hipMemcpyHostToDevice, o.st));
    HIPCHK(hipMemcpyAsync(da, ha.data(), R, hipMemcpyHostToDevice, o.st));
    { const int rc = lc_exec(c, a, o.st, 0, measured || row_sum_ms, p); if (rc) return rc; }
  }
  lc_summary(p, -1, out);
  lc_deliver(p, measured_by, sum_ms, min_ms, max_ms, measured, row_sum_ms);
  return KB_OK;
}
