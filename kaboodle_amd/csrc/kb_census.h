// kb_census.h — the view census (include/kaboodle_census.h): for every id the number of running
// rows whose view holds it, and for every running row how far its view is from the running set.  Included at
// the end of kb_sim.hip; reads the engines' state, writes only its own scratch.  The host side stands on the
// frame of kb_censusframe.h: cs_leaf(kb_sim*) / cs_leaf(SpSim*) are the leaves that route() hands the shards to.
//
// Dense engine: one streaming pass over the member bits (Dev::bits, [rows][W/32]).  A lane owns one 16-byte
// column group (4 words = 128 ids) and walks down a tile of rows, so each row read is 1 KiB contiguous per
// wave.  The column counts are BIT-SLICED (ColCount<4>, kb_bitpass.h): the 5 low planes are folded into the 12
// high ones every 24 rows, and only at the end of the tile is each of the lane's 128 counters read out of them.
// A workgroup's 4 waves (4 row tiles of one column block) combine their counters in LDS and add them to the
// [W] result with integer atomics: order-free, so the result is deterministic.  The per-row counts (|view|,
// running members, stale members) come in the same pass: three popcounts per word against loop-invariant
// masks, a DPP reduction per row.
//
// Sparse rows: known_by[j] = B·base[j] + Σ over running rows of their exception entries (−1 for a based row's
// exception that is a base member, +1 otherwise), B = running rows that adopted the base: O(entries) signed
// atomics into a delta array, then one finishing kernel over the ids.  The rows' counts follow the same way
// from the base's counts.
#pragma once
#include "../../include/kaboodle_census.h"

namespace kb {

constexpr uint32_t CS_FOLD = 24;                  // rows between folds (<= 2^BP_LOW - 1, a multiple of BP_U)
constexpr uint32_t CS_COLS = 8192;                // ids per column block: 64 lanes x 128
static_assert(CS_FOLD % BP_U == 0 && CS_FOLD < (1u << BP_LOW) && BP_MAX_RPW % CS_FOLD == 0, "kb_census.h fold period");

struct CsDense {
  uint32_t* kb;                                   // [W] known_by (zeroed)
  uint32_t* rowc;                                 // [3][R] |view|, running members, stale members (zeroed)
  IdMasks m;                                      // k_id_masks, all three
  uint32_t rpw;                                   // rows per wave
};

// grid (W / 8192 column blocks, row tiles of 4 x rpw rows), 256 threads
__global__ __launch_bounds__(256) void k_cs_dense(Dev d, CsDense a) {
  __shared__ uint32_t cnt[col_lds(4)];
  for (uint32_t k = threadIdx.x; k < col_lds(4); k += 256) cnt[k] = 0;
  __syncthreads();
  const uint32_t l = lane();
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t nw4 = d.NWR / 4;
  const uint32_t cg = blockIdx.x * 64 + l;                       // this lane's column group (< nw4: the grid is exact)
  const uint4 ab = reinterpret_cast<const uint4*>(a.m.ab)[cg];
  const uint4 sb = reinterpret_cast<const uint4*>(a.m.sb)[cg];
  const uint4 vb = reinterpret_cast<const uint4*>(a.m.vb)[cg];
  uint32_t r0, r1;
  wave_rows(d.lo, d.hi, blockIdx.y, wv, a.rpw, r0, r1);
  const uint4* rows = reinterpret_cast<const uint4*>(d.bits);
  ColCount<4> cc;
  uint32_t nlow = 0;
  for (uint32_t r = r0; r < r1; r += BP_U) {
    uint32_t am = 0;                                             // the batch's running rows: a scalar mask
#pragma unroll
    for (uint32_t u = 0; u < BP_U; ++u) if (r + u < r1 && d.alive[r + u]) am |= 1u << u;
    am = (uint32_t)__builtin_amdgcn_readfirstlane((int)am);
    if (!am) continue;                                           // no running row: nothing is read
    uint4 v[BP_U];
#pragma unroll
    for (uint32_t u = 0; u < BP_U; ++u) {                        // every load of the batch before its first use
      const uint32_t rr = r + u < r1 ? r + u : r1 - 1;
      v[u] = rows[(size_t)rr * nw4 + cg];
    }
#pragma unroll
    for (uint32_t u = 0; u < BP_U; ++u) {
      if (!((am >> u) & 1u)) continue;                           // a scalar branch: the row is not an observer
      const uint32_t x0 = v[u].x & vb.x, x1 = v[u].y & vb.y, x2 = v[u].z & vb.z, x3 = v[u].w & vb.w;
      cc.add(0, x0); cc.add(1, x1); cc.add(2, x2); cc.add(3, x3);
      const uint32_t nv = __popc(x0) + __popc(x1) + __popc(x2) + __popc(x3);
      const uint32_t nr = __popc(x0 & ab.x) + __popc(x1 & ab.y) + __popc(x2 & ab.z) + __popc(x3 & ab.w);
      const uint32_t ns = __popc(x0 & sb.x) + __popc(x1 & sb.y) + __popc(x2 & sb.z) + __popc(x3 & sb.w);
      const uint32_t t0 = wave_sum(nv | (nr << 16));             // <= 8192 each per wave: 16 bits hold them
      const uint32_t t1 = wave_sum(ns);
      if (l == 0) {
        const size_t R = d.hi - d.lo, k = r + u - d.lo;
        if (t0 & 0xFFFFu) atomicAdd(&a.rowc[k], t0 & 0xFFFFu);
        if (t0 >> 16) atomicAdd(&a.rowc[R + k], t0 >> 16);
        if (t1) atomicAdd(&a.rowc[2 * R + k], t1);
      }
    }
    nlow += BP_U;
    if (nlow == CS_FOLD) { cc.fold(); nlow = 0; }
  }
  cc.fold();
  cc.readout(cnt, l);
  __syncthreads();
  col_flush<4>(cnt, a.kb + (size_t)blockIdx.x * CS_COLS);
}

// ---- sparse rows ---------------------------------------------------------------------------------------
struct CsSparse {
  int32_t* delta;                                 // [C] signed exception counts (zeroed)
  uint32_t* kb;                                   // [C] known_by
  uint32_t* rowc;                                 // [3][R] |view|, running members, stale members
  uint32_t* acc;                                  // [4] base ∩ running, base ∩ stale class, B, spare (zeroed)
};
// the base's counts: its running members and its members that are neither running nor external
__global__ __launch_bounds__(256) void k_cs_sp_base(SpDev d, CsSparse a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t run = 0, st = 0;
  if (j < d.C && sp_bbit(d, j)) {
    const bool al = d.alive[j] != 0;
    run = al; st = !al && !d.ext[j];
  }
  const uint32_t t = wave_sum(run | (st << 16));
  if (lane() == 0 && t) {
    if (t & 0xFFFFu) atomicAdd(&a.acc[0], t & 0xFFFFu);
    if (t >> 16) atomicAdd(&a.acc[1], t >> 16);
  }
}
// a thread per local row: its exceptions into the delta array and its own counts
__global__ __launch_bounds__(256) void k_cs_sp_rows(SpDev d, CsSparse a) {
  const uint32_t i = sp_gid(d);
  const bool obs = i < d.hi && d.alive[i];
  const bool based = obs && d.based[i];
  const uint64_t nb = __ballot(based);
  if (nb && lane() == (uint32_t)__builtin_ctzll(nb)) atomicAdd(&a.acc[2], (uint32_t)__popcll(nb));
  if (!obs) return;
  const uint32_t n = d.ne[i];
  const uint4* e4 = reinterpret_cast<const uint4*>(sp_row(d, i));
  int32_t dv = 0, dr = 0, ds = 0;
  for (uint32_t g = 0; g < (n + 3u) >> 2; ++g) {                 // 16-byte loads (rows are 16-byte aligned)
    const uint4 w4 = e4[g];
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const bool on = g * 4 + q < n && (w[q] & SP_XF);
      // the lanes of a wave that hold the same exception as its first such lane add it once between them: an id
      // that left sits in every row's list, at the same place wherever the lists are otherwise alike
      const uint32_t j = w[q] >> 9;
      const int32_t sg = on && based && sp_bbit(d, j) ? -1 : 1;
      const uint32_t key = on ? (j << 1) | (sg < 0 ? 1u : 0u) : 0xFFFFFFFFu;
      const uint64_t act = __ballot(on);
      if (!act) continue;
      const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, __builtin_ctzll(act));
      const uint64_t same = __ballot(on && key == k0);
      if (on) {
        if (key == k0) { if (lane() == (uint32_t)__builtin_ctzll(same)) atomicAdd(&a.delta[j], sg * (int32_t)__popcll(same)); }
        else atomicAdd(&a.delta[j], sg);
        const bool al = d.alive[j] != 0;
        dv += sg; if (al) dr += sg; else if (!d.ext[j]) ds += sg;
      }
    }
  }
  const size_t R = d.hi - d.lo, k = i - d.lo;
  a.rowc[k] = (uint32_t)((int32_t)(based ? d.nb : 0u) + dv);
  a.rowc[R + k] = (uint32_t)((int32_t)(based ? a.acc[0] : 0u) + dr);
  a.rowc[2 * R + k] = (uint32_t)((int32_t)(based ? a.acc[1] : 0u) + ds);
}
__global__ __launch_bounds__(256) void k_cs_sp_finish(SpDev d, CsSparse a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < d.C) a.kb[j] = (uint32_t)((int32_t)(sp_bbit(d, j) ? a.acc[2] : 0u) + a.delta[j]);
}

}  // namespace kb

// ---- host side -------------------------------------------------------------------------------------------
// one handle's part of a census: known_by over all ids from its rows, the row counts at its rows' ids
struct CsPart {
  std::vector<uint32_t> kb, view, run, stale;     // [C] each (rows the handle does not hold: 0)
  std::vector<uint8_t> alive, ext;                // [C] replicated facts
  std::vector<uint8_t> held;                      // [C] 1 = a row of this handle (or of a shard already added)
  double ms = 0;
};
static void cs_part_init(CsPart& p, uint32_t C) {
  p.kb.assign(C, 0); p.view.assign(C, 0); p.run.assign(C, 0); p.stale.assign(C, 0); p.held.assign(C, 0);
}
// the end of a leaf's pass: its device time, the rows' counts of the shard (device [3][R]) and its known_by join the part
static int cs_collect(CsPart& p, uint32_t C, uint32_t lo, uint32_t R, const uint32_t* d_kb, const uint32_t* d_rowc,
                      const uint8_t* d_alive, const uint8_t* d_ext, hipStream_t st, CsTimer& tm) {
  tm.stop(st);                                                   // the pass ends here: its launches are all issued
  HIPCHK(hipGetLastError());
  // sized before the first copy waits for the kernels: zero-filling [C] and [3][R] words overlaps their run
  std::vector<uint32_t> kb(C), rc(3ull * R);
  p.alive.resize(C); p.ext.resize(C);
  HIPCHK(fetch(kb, d_kb, C, st));
  HIPCHK(fetch(rc, d_rowc, 3ull * R, st));
  HIPCHK(fetch(p.alive, d_alive, C, st));
  HIPCHK(fetch(p.ext, d_ext, C, st));
  HIPCHK(hipStreamSynchronize(st));
  p.ms += tm.ms();
  for (uint32_t j = 0; j < C; ++j) p.kb[j] += kb[j];
  for (uint32_t k = 0; k < R; ++k) {
    p.view[lo + k] = rc[k]; p.run[lo + k] = rc[R + k]; p.stale[lo + k] = rc[2ull * R + k]; p.held[lo + k] = 1;
  }
  return KB_OK;
}

// one leaf's pass (route() hands every shard of a group here in turn): dense rows
static int cs_leaf(kb_sim* s, CsPart& p) {
  (void)hipSetDevice(s->device);
  const Dev& d = s->d;
  CsDense a;
  auto lay = [&](Carve& c) {                                     // known_by and the rows' counts are cleared every pass
    c.zero_from(); a.kb = c.take<uint32_t>(s->W); a.rowc = c.take<uint32_t>(3ull * s->R); c.zero_to();
    a.m = carve_masks(c, d.NWR, true);
  };
  if (!s->cs_buf) HIPCHK(talloc(s, &s->cs_buf, carve_bytes(lay) / 4));
  const Carve c = carve(s->cs_buf, lay);
  // env KB_CENSUS_RPW overrides the rows per wave, in whole fold periods (tools/census_cost.py records its value,
  // DESIGN.md §12)
  const uint32_t cb = s->W / CS_COLS;
  a.rpw = rows_per_wave(s->R, cb, s->ncu, rpw_env("KB_CENSUS_RPW"), CS_FOLD, BP_MAX_RPW);
  CsTimer tm;
  if (!tm.start(s->st)) { seterr("census: events"); return KB_IO_ERROR; }
  HIPCHK(hipMemsetAsync(c.zero_ptr(), 0, c.zero_bytes(), s->st));
  id_masks(d.alive, d.ext, d.C, d.NWR, a.m, s->st);
  k_cs_dense<<<dim3(cb, row_tiles(s->R, a.rpw)), 256, 0, s->st>>>(d, a);
  return cs_collect(p, s->C, s->lo, s->R, a.kb, a.rowc, d.alive, d.ext, s->st, tm);
}
// sparse rows (the contact-age census reuses the pass and its scratch, kb_agecensus.h)
static int cs_leaf(SpSim* S, CsPart& p) {
  (void)hipSetDevice(S->device);
  const SpDev& d = S->d;
  const uint32_t C = S->C, R = S->R;
  CsSparse a;
  auto lay = [&](Carve& c) {                                     // all but known_by is cleared every pass
    c.zero_from(); a.delta = c.take<int32_t>(C); a.acc = c.take<uint32_t>(4); a.rowc = c.take<uint32_t>(3ull * R); c.zero_to();
    a.kb = c.take<uint32_t>(C);
  };
  if (!S->cs_buf && sp_alloc(S, &S->cs_buf, carve_bytes(lay) / 4) != hipSuccess) { seterr("census: device allocation failed"); return KB_CAPACITY; }
  const Carve c = carve(S->cs_buf, lay);
  CsTimer tm;
  if (!tm.start(S->st)) { seterr("census: events"); return KB_IO_ERROR; }
  HIPCHK(hipMemsetAsync(c.zero_ptr(), 0, c.zero_bytes(), S->st));
  k_cs_sp_base<<<(C + 255) / 256, 256, 0, S->st>>>(d, a);
  k_cs_sp_rows<<<(R + 255) / 256, 256, 0, S->st>>>(d, a);
  k_cs_sp_finish<<<(C + 255) / 256, 256, 0, S->st>>>(d, a);
  return cs_collect(p, C, S->lo, R, a.kb, a.rowc, d.alive, d.ext, S->st, tm);
}

// the O(ids) reductions of the summary, on the host
static void cs_summary(const CsPart& p, uint32_t C, int32_t round, kb_census* out, uint32_t* missing, uint32_t* stale) {
  memset(out, 0, sizeof *out);
  out->round = round;
  uint32_t running = 0;
  for (uint32_t j = 0; j < C; ++j) running += p.alive[j] != 0;
  out->running = running;
  for (uint32_t i = 0; i < C; ++i) {
    const bool obs = p.held[i] && p.alive[i];
    const uint32_t m = obs ? running - p.run[i] : 0u, st = obs ? p.stale[i] : 0u;
    if (missing) missing[i] = m;
    if (stale) stale[i] = st;
    if (!obs) continue;
    out->observers++; out->pairs += p.view[i]; out->missing += m; out->stale += st;
    out->exact_views += m == 0 && st == 0;
  }
  out->least_known = out->top_ghost = KB_CENSUS_NONE;
  for (uint32_t j = 0; j < C; ++j) {
    const uint32_t k = p.kb[j];
    if (p.alive[j]) {
      out->full_ids += k == out->observers;
      if (out->least_known == KB_CENSUS_NONE || k < out->least_known_by) { out->least_known = j; out->least_known_by = k; }
    } else if (!p.ext[j] && k) {
      out->ghost_ids++;
      if (k > out->top_ghost_by) { out->top_ghost = j; out->top_ghost_by = k; }
    }
  }
}

extern "C" int kb_sim_census(kb_sim* s, kb_census* out, uint32_t* known_by, size_t cap_ids, uint32_t* missing,
                             uint32_t* stale, size_t cap_rows) {
  if (!s) return KB_INVALID_ARGUMENT;
  { const int rc = census_caps("kb_sim_census", out, known_by, cap_ids, s->C, any_of(missing, stale), cap_rows, s->C); if (rc) return rc; }
  CsPart p;
  cs_part_init(p, s->C);
  int32_t round = 0;
  { const int rc = route(s, R_ALL, 0, [&](auto* e) { return cs_leaf(e, p); }); if (rc) return rc; }
  { const int rc = route(s, R_FIRST, 0, [&](auto* e) { round = e->round; return KB_OK; }); if (rc) return rc; }
  s->census_ms[CM_VIEW] = p.ms;
  cs_summary(p, s->C, round, out, missing, stale);
  deliver(known_by, p.kb);
  return KB_OK;
}

extern "C" int kb_sim_census_device_ms(kb_sim* s, double* ms) { return census_ms_get(s, CM_VIEW, ms); }
