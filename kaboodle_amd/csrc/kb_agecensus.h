// kb_agecensus.h — the contact-age census (include/kaboodle_age.h): per id how many observers hold
// it as suspect, ancient, windowed and fresh and the latest instant any of them heard from it; per row the same four
// counts over its view; a histogram of the windowed cells by age.  Included at the end of kb_sim.hip; reads the
// sparse engine's state, writes only its own scratch.  Dense handles are refused (§17: their pass is left out).
//
// Sparse rows: a thread per row over its entry list, the shape of k_cs_sp_rows.  Explicit entries carry the stamp,
// so suspect, windowed and fresh cells are the entries with a nonzero stamp that are members; the ancient counts
// follow from the view census's sparse pass (cs_leaf(SpSim*), reused): ancient = |view| - [self] - suspects - windowed.
// The histogram (windowed cells by stamp byte; the host turns bytes into ages) goes through a workgroup's LDS words.
#pragma once
#include "../../include/kaboodle_age.h"

namespace kb {

// the decode (kb_ctl.h): since = byte + epoch_base(r) - EOFF; the freshest byte is enc(r, r) = r % EPOCH + EOFF
static_assert(EPOCH - 1 + EOFF <= 255, "Known(r) fits the byte");
static_assert(EPOCH - 1 + EOFF - (ST_ANCIENT + 1) < KB_AGE_HIST, "every age has a bucket");

// ---- sparse rows ---------------------------------------------------------------------------------------
struct AgSparse {
  uint32_t* by;                                   // [4][C]: suspected_by, windowed_by, fresh_by, the byte maximum (zeroed)
  uint32_t* rowc;                                 // [4][R]: suspects, windowed, fresh, [the row holds itself]
  unsigned long long* hist;                       // [256] windowed cells by byte (zeroed)
  uint32_t fresh_thr;
};
// a thread per local row: its stamped entries into the per-id arrays and the histogram, its own counts
__global__ __launch_bounds__(256) void k_age_sp_rows(SpDev d, AgSparse a) {
  __shared__ uint32_t lh[256];
  lh[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = sp_gid(d);
  const bool obs = i < d.hi && d.alive[i];
  if (obs) {
    const bool based = d.based[i];
    const uint32_t n = d.ne[i], C = d.C;
    const uint4* e4 = reinterpret_cast<const uint4*>(sp_row(d, i));
    uint32_t ns = 0, nw = 0, nf = 0, self = based && sp_bbit(d, i);
    for (uint32_t g = 0; g < (n + 3u) >> 2; ++g) {                 // 16-byte loads (rows are 16-byte aligned)
      const uint4 w4 = e4[g];
      const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) {
        const bool in = g * 4 + q < n;
        const uint32_t j = w[q] >> 9, b = w[q] & 255u;
        const bool mem = in && ((based && sp_bbit(d, j)) != ((w[q] & SP_XF) != 0));
        if (in && j == i) self = mem;
        const bool on = mem && j != i && (b == ST_SUSPECT || b > ST_ANCIENT);
        // the lanes of a wave that hold the same (id, byte) as its first such lane add it once between them: a
        // joiner heard by every row in the same round sits in every list with the same stamp
        const uint32_t key = on ? (j << 8) | b : 0xFFFFFFFFu;
        const uint64_t act = __ballot(on);
        if (!act) continue;
        const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, __builtin_ctzll(act));
        const uint64_t same = __ballot(on && key == k0);
        if (on) {
          const bool win = b > ST_ANCIENT, fr = b >= a.fresh_thr;
          ns += !win; nw += win; nf += fr;
          uint32_t m = 1;
          if (key == k0) m = lane() == (uint32_t)__builtin_ctzll(same) ? (uint32_t)__popcll(same) : 0u;
          if (m) {
            atomicAdd(&a.by[(win ? C : 0u) + j], m);
            if (fr) atomicAdd(&a.by[2ull * C + j], m);
            if (win) { atomicAdd(&lh[b], m); atomicMax(&a.by[3ull * C + j], b); }
          }
        }
      }
    }
    const size_t R = d.hi - d.lo, k = i - d.lo;
    a.rowc[k] = ns; a.rowc[R + k] = nw; a.rowc[2 * R + k] = nf; a.rowc[3 * R + k] = self;
  }
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&a.hist[threadIdx.x], (unsigned long long)lh[threadIdx.x]);
}

}  // namespace kb

// ---- host side -------------------------------------------------------------------------------------------
// a census being put together: the ids' and rows' arrays, added to shard by shard; the histogram by stamp byte
struct AgPart {
  std::vector<uint32_t> sb, ab, wb, fb, mx;       // [n_ids] the four *_by, the largest windowed byte (0: none)
  std::vector<uint32_t> rs, ra, rw, rf;           // [n_rows]
  std::vector<uint8_t> alive, ext;                // [n_ids] replicated facts
  uint64_t hist[256] = {};
  uint32_t observers = 0;
  double ms = 0;
};
static void ag_part_init(AgPart& p, size_t n_ids, size_t n_rows) {
  p.sb.assign(n_ids, 0); p.ab.assign(n_ids, 0); p.wb.assign(n_ids, 0); p.fb.assign(n_ids, 0); p.mx.assign(n_ids, 0);
  p.rs.assign(n_rows, 0); p.ra.assign(n_rows, 0); p.rw.assign(n_rows, 0); p.rf.assign(n_rows, 0);
  p.alive.assign(n_ids, 0); p.ext.assign(n_ids, 0);
}
// the decode of the last simulated round (kb_ctl.h, ctl_peer_states)
struct AgEpoch { int32_t r, E0; uint32_t top, fresh_thr; };
static AgEpoch ag_epoch(int32_t round) {
  AgEpoch e;
  e.r = round > 0 ? round - 1 : 0;
  e.E0 = kb::epoch_base(e.r);
  e.top = (uint32_t)(e.r - e.E0 + kb::EOFF);                      // enc(r, r): the freshest byte, age 0
  e.fresh_thr = e.top - (uint32_t)kb::SHARE_AGE + 1u;             // age < SHARE_AGE <=> byte >= this
  return e;
}

// the O(ids) reductions of the summary, on the host; bytes become ages and rounds here
static int ag_summary(const AgPart& p, int32_t round, kb_age_census* out, int32_t* last_heard, const char* who) {
  const AgEpoch e = ag_epoch(round);
  memset(out, 0, sizeof *out);
  out->round = round;
  out->observers = p.observers;
  // age = top - byte is in [0, top - 3], inside the histogram: no engine stamps past Known(r)
  for (uint32_t b = e.top + 1; b < 256; ++b)
    if (p.hist[b]) { seterr(std::string(who) + ": a stamp byte decodes to an instant after the last simulated round"); return KB_INVALID_ARGUMENT; }
  for (uint32_t b = kb::ST_ANCIENT + 1; b <= e.top; ++b) out->hist[e.top - b] = p.hist[b];
  out->oldest_heard_id = KB_CENSUS_NONE; out->oldest_heard = INT32_MIN;
  for (size_t j = 0; j < p.sb.size(); ++j) {
    const int32_t lh = p.mx[j] > kb::ST_ANCIENT ? (int32_t)p.mx[j] + e.E0 - kb::EOFF : INT32_MIN;
    if (last_heard) last_heard[j] = lh;
    out->suspects += p.sb[j]; out->ancient += p.ab[j]; out->windowed += p.wb[j]; out->fresh += p.fb[j];
    if (p.alive[j]) {
      out->unheard_ids += p.wb[j] == 0;
      if (out->oldest_heard_id == KB_CENSUS_NONE || lh < out->oldest_heard) { out->oldest_heard_id = (uint32_t)j; out->oldest_heard = lh; }
    } else if (!p.ext[j]) {
      out->dead_suspects += p.sb[j]; out->dead_ancient += p.ab[j]; out->dead_windowed += p.wb[j]; out->dead_fresh += p.fb[j];
    }
  }
  out->cells = out->suspects + out->ancient + out->windowed;
  return KB_OK;
}

// one leaf's pass (route() hands every shard of a group here in turn)
static int ag_leaf(kb_sim*, AgPart&) { return KB_INVALID_OPERATION; }   // not reached: census_gate refuses dense rows
static int ag_leaf(SpSim* S, AgPart& p) {
  (void)hipSetDevice(S->device);
  const SpDev& d = S->d;
  const uint32_t C = S->C, R = S->R;
  // |view| and known_by of this shard's rows: the view census's sparse pass (it uses that census's scratch, cs_buf)
  CsPart cp;
  cs_part_init(cp, C);
  { const int rc = cs_leaf(S, cp); if (rc) return rc; }
  const size_t words = 512ull + 4ull * C + 4ull * R;
  if (!S->ag_buf) {
    if (sp_alloc(S, &S->ag_buf, words) != hipSuccess) { seterr("age census: device allocation failed"); return KB_CAPACITY; }
  }
  kb::AgSparse a;
  a.hist = reinterpret_cast<unsigned long long*>(S->ag_buf); a.by = S->ag_buf + 512; a.rowc = a.by + 4ull * C;
  a.fresh_thr = ag_epoch(S->round).fresh_thr;
  CsTimer tm;
  if (!tm.start(S->st)) { seterr("age census: events"); return KB_IO_ERROR; }
  HIPCHK(hipMemsetAsync(S->ag_buf, 0, 4ull * words, S->st));
  kb::k_age_sp_rows<<<(R + 255) / 256, 256, 0, S->st>>>(d, a);
  tm.stop(S->st);
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> by, rowc;
  unsigned long long hist[256];
  HIPCHK(hipMemcpyAsync(hist, a.hist, sizeof hist, hipMemcpyDeviceToHost, S->st));
  HIPCHK(fetch(by, a.by, 4ull * C, S->st));
  HIPCHK(fetch(rowc, a.rowc, 4ull * R, S->st));
  HIPCHK(hipStreamSynchronize(S->st));
  p.ms += cp.ms + tm.ms();
  p.alive = cp.alive; p.ext = cp.ext;
  for (uint32_t k = 0; k < 256; ++k) p.hist[k] += hist[k];
  // ancient_by = known_by - [self] - suspected_by - windowed_by, over this shard's rows (sums of shards add up)
  for (uint32_t j = 0; j < C; ++j) {
    p.sb[j] += by[j]; p.wb[j] += by[(size_t)C + j]; p.fb[j] += by[2ull * C + j];
    p.mx[j] = std::max(p.mx[j], by[3ull * C + j]);
    p.ab[j] += cp.kb[j] - by[j] - by[(size_t)C + j];
  }
  for (uint32_t k = 0; k < R; ++k) {
    const uint32_t i = S->lo + k;
    if (!cp.alive[i]) continue;
    const uint32_t self = rowc[3ull * R + k];
    p.observers++;
    p.rs[i] = rowc[k]; p.rw[i] = rowc[(size_t)R + k]; p.rf[i] = rowc[2ull * R + k];
    p.ra[i] = cp.view[i] - self - p.rs[i] - p.rw[i];
    p.ab[i] -= self;
  }
  return KB_OK;
}

extern "C" int kb_sim_age_census(kb_sim* s, kb_age_census* out, uint32_t* suspected_by, uint32_t* ancient_by, uint32_t* windowed_by,
                                 uint32_t* fresh_by, int32_t* last_heard, size_t cap_ids, uint32_t* suspects, uint32_t* ancient,
                                 uint32_t* windowed, uint32_t* fresh, size_t cap_rows) {
  if (!s) return KB_INVALID_ARGUMENT;
  { const int rc = census_caps("kb_sim_age_census", out, any_of(suspected_by, ancient_by, windowed_by, fresh_by, last_heard), cap_ids, s->C,
                               any_of(suspects, ancient, windowed, fresh), cap_rows, s->C); if (rc) return rc; }
  { const int rc = census_gate(s, "kb_sim_age_census", {"", nullptr, "are not answered yet (KB_VARIANT_SPARSE_ROWS handles are)"});
    if (rc) return rc; }
  AgPart p;
  ag_part_init(p, s->C, s->C);
  int32_t round = 0;
  { const int rc = route(s, R_ALL, 0, [&](auto* e) { return ag_leaf(e, p); }); if (rc) return rc; }
  { const int rc = route(s, R_FIRST, 0, [&](auto* e) { round = e->round; return KB_OK; }); if (rc) return rc; }
  s->census_ms[CM_AGE] = p.ms;
  { const int rc = ag_summary(p, round, out, last_heard, "kb_sim_age_census"); if (rc) return rc; }
  deliver(suspected_by, p.sb); deliver(ancient_by, p.ab); deliver(windowed_by, p.wb); deliver(fresh_by, p.fb);
  deliver(suspects, p.rs); deliver(ancient, p.ra); deliver(windowed, p.rw); deliver(fresh, p.rf);
  return KB_OK;
}

extern "C" int kb_sim_age_census_device_ms(kb_sim* s, double* ms) { return census_ms_get(s, CM_AGE, ms); }
