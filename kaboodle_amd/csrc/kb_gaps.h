// kb_gaps.h — the gap list and the holders query (include/kaboodle_gaps.h): the cells the view census
// counts, by name.  Included at the end of kb_sim.hip beside the censuses; stands on the frame of kb_censusframe.h and
// kb_bitpass.h (masks, row table, scratch carver).  It reads the member bits, the running set and the external ids
// (never the stamps or the latency table) and writes only its own scratch.
//
// One piece of code lists the set bits of a bit table, a row at a time, in three launches:
//   COUNT  a wave per row: the row's words in 16-byte loads, turned into the listed set by a GpSel (an optional
//          inversion and up to two AND masks: missing = ~bits & ab & vb, stale = bits & sb), popcounted, a DPP sum per
//          row.  A row that is no observer is a scalar skip and is not read.  Up to two lists in one pass.
//   SCAN   one workgroup per list: the exclusive 64-bit prefix of the rows' counts, 1,024 rows a step; its last entry
//          is the total, and the rows with a nonzero count are counted on the way.
//   EMIT   launched only for a list the caller's buffer holds.  A wave per row; a row whose scan slice is empty is
//          skipped before its bits are touched.  Each lane popcounts its four words, the wave takes an exclusive
//          prefix over its lanes, and each lane writes its set bits in ascending order from row offset + prefix.  Rows
//          wider than one pass (64 lanes x 4 words = 8,192 ids) loop and carry the running base.
// Every element's place follows from the scan, not from an atomic, so the output is ordered and the same on every run.
//
// The gap list runs this over the member bits (rows = ids' rows, through BitRows: a group is one table).  The holders
// query first cuts the asked columns out of the member bits: a wave takes 64 consecutive rows of one query, each lane
// loads the word of its row that holds the id, and one __ballot of the id's bit, ANDed with the observer bits of those
// 64 rows, is 64 holders as one 64-bit word of a [queries][ceil(C / 64)] transposed table.  The same three launches
// then list that table, with rows = queries, no masks, and row ids instead of (row, id) pairs.
//
// No workgroup waits for another; every loop is bounded by counts the host passes or by the bits of a word.
#pragma once
#include "../../include/kaboodle_gaps.h"

namespace kb {

constexpr uint32_t GP_PASS = 64;                  // 16-byte groups a wave reads per pass: 256 words, 8,192 ids

// what of a table's words is listed: word w of a row counts as (x ^ inv) & m0[w] & m1[w]; a null mask is all ones
struct GpSel { const uint32_t* m0; const uint32_t* m1; uint32_t inv; };

struct GpArgs {
  BitRows rows;                                   // rows.C rows of rows.NWR words (a multiple of 4: 16-byte loads)
  const uint32_t* active;                         // bit i: row i is listed (null: every row is)
  uint32_t nsel;                                  // lists taken in one pass: 1 or 2
  GpSel sel[2];
  uint32_t* cnt;                                  // [nsel][rows] the rows' counts
  uint64_t* off;                                  // [nsel][rows + 1] their exclusive prefix; the last entry: the total
  uint32_t* nz;                                   // [nsel] rows with a nonzero count
};

__device__ __attribute__((always_inline)) inline uint4 gp_words(const GpSel& s, uint4 x, uint32_t g) {
  x.x ^= s.inv; x.y ^= s.inv; x.z ^= s.inv; x.w ^= s.inv;
  if (s.m0) { const uint4 m = reinterpret_cast<const uint4*>(s.m0)[g]; x.x &= m.x; x.y &= m.y; x.z &= m.z; x.w &= m.w; }
  if (s.m1) { const uint4 m = reinterpret_cast<const uint4*>(s.m1)[g]; x.x &= m.x; x.y &= m.y; x.z &= m.z; x.w &= m.w; }
  return x;
}
__device__ __attribute__((always_inline)) inline uint32_t gp_popc(const uint4& x) { return __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w); }
// the row of wave wv of this block (4 rows a block), wave-uniform
__device__ __attribute__((always_inline)) inline uint32_t gp_row() {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
}

// grid ceil(rows / 4), 256 threads
__global__ __launch_bounds__(256) void k_gp_count(GpArgs a) {
  const uint32_t l = lane(), i = gp_row(), n = a.rows.C;
  if (i >= n) return;
  uint32_t c0 = 0, c1 = 0;
  const bool on = !a.active || (((uint32_t)__builtin_amdgcn_readfirstlane((int)a.active[i >> 5]) >> (i & 31u)) & 1u);
  if (on) {                                                      // scalar: a row that is not listed is not read
    const uint4* row = reinterpret_cast<const uint4*>(bit_row(a.rows, i));
    const uint32_t nw4 = a.rows.NWR / 4;
    for (uint32_t g0 = 0; g0 < nw4; g0 += GP_PASS) {
      const uint32_t g = g0 + l;
      if (g < nw4) {
        const uint4 x = row[g];
        c0 += gp_popc(gp_words(a.sel[0], x, g));
        if (a.nsel > 1) c1 += gp_popc(gp_words(a.sel[1], x, g));
      }
    }
    c0 = wave_sum(c0);                                           // the whole wave is here again
    c1 = wave_sum(c1);
  }
  if (l == 0) {
    a.cnt[i] = c0;
    if (a.nsel > 1) a.cnt[(size_t)n + i] = c1;
  }
}

// grid nsel, 1024 threads: block s scans list s
__global__ __launch_bounds__(1024) void k_gp_scan(GpArgs a) {
  __shared__ uint64_t wsum[16];
  __shared__ uint32_t wnz[16];
  const uint32_t n = a.rows.C, s = blockIdx.x, l = lane(), wv = threadIdx.x >> 6;
  const uint32_t* cnt = a.cnt + (size_t)s * n;
  uint64_t* off = a.off + (size_t)s * ((size_t)n + 1);
  uint64_t base = 0;
  uint32_t nz = 0;
  for (uint32_t t0 = 0; t0 < n; t0 += 1024) {                    // n and t0 are uniform: every thread takes every step
    const uint32_t i = t0 + threadIdx.x;
    const uint32_t v = i < n ? cnt[i] : 0u;
    uint64_t x = v;                                              // the wave's inclusive prefix
#pragma unroll
    for (uint32_t k = 1; k < 64; k <<= 1) {
      const uint64_t y = __shfl_up((unsigned long long)x, k, 64);
      if (l >= k) x += y;
    }
    const uint64_t nzb = __ballot(v != 0);
    if (l == 63) { wsum[wv] = x; wnz[wv] = (uint32_t)__popcll(nzb); }
    __syncthreads();
    uint64_t pre = base;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      const uint64_t w = wsum[k];
      if (k < wv) pre += w;
      base += w; nz += wnz[k];
    }
    if (i < n) off[i] = pre + x - v;
    __syncthreads();                                             // the sums are read before the next step writes them
  }
  if (threadIdx.x == 0) { off[n] = base; a.nz[s] = nz; }
}

// List s of the table: (row, id) pairs (pairs != 0: 8-byte stores) or ids alone, `cap` elements at `out`, which is
// the list's total (every store is checked against it).  grid ceil(rows / 4), 256 threads.
__global__ __launch_bounds__(256) void k_gp_emit(GpArgs a, uint32_t s, uint32_t pairs, uint32_t* out, uint64_t cap) {
  const uint32_t l = lane(), i = gp_row(), n = a.rows.C;
  if (i >= n) return;
  const uint64_t* off = a.off + (size_t)s * ((size_t)n + 1);
  uint64_t base = off[i];
  if (base == off[i + 1]) return;                                // scalar: nothing to list, the row is not read
  const GpSel sel = a.sel[s];
  const uint4* row = reinterpret_cast<const uint4*>(bit_row(a.rows, i));
  const uint32_t nw4 = a.rows.NWR / 4;
  uint2* out2 = reinterpret_cast<uint2*>(out);
  for (uint32_t g0 = 0; g0 < nw4; g0 += GP_PASS) {
    const uint32_t g = g0 + l;
    uint4 x = make_uint4(0, 0, 0, 0);
    if (g < nw4) x = gp_words(sel, row[g], g);
    const uint32_t c = gp_popc(x);
    const uint32_t inc = wave_iscan<0u>(c, OpAdd{});             // the whole wave: the loop's bounds are uniform
    const uint32_t tot = wave_last(inc);
    uint64_t at = base + (inc - c);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      for (uint32_t y = w[q]; y; y &= y - 1, ++at) {
        const uint32_t id = (4 * g + q) * 32 + (uint32_t)__builtin_ctz(y);
        if (at < cap) {
          if (pairs) out2[at] = make_uint2(i, id);
          else out[at] = id;
        }
      }
    }
    base += tot;
  }
}

// ---- the holders' columns -------------------------------------------------------------------------------
struct HdArgs {
  BitRows rows;                                   // the member bits
  const uint32_t* ab;                             // [rows.NWR] the running ids: the observers
  const uint32_t* ids;                            // [nq] the asked ids, each < rows.C
  uint32_t nq, hw;                                // queries; 64-bit words a query's row of the table takes (even)
  uint64_t* tab;                                  // [nq][hw] bit r of a row: observer r holds the id
};
// grid (ceil(hw / 4), nq), 256 threads: a wave makes one word
__global__ __launch_bounds__(256) void k_hd_column(HdArgs a) {
  const uint32_t l = lane(), b = gp_row();
  if (b >= a.hw) return;
  const uint32_t q = blockIdx.y;
  const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.ids[q]);
  const uint32_t r = b * 64 + l;
  bool bit = false;
  if (r < a.rows.C) bit = (bit_row(a.rows, r)[j >> 5] >> (j & 31u)) & 1u;
  uint64_t w = __ballot(bit);
  const uint32_t w0 = 2 * b, w1 = 2 * b + 1;                     // the observer bits of rows 64 b .. 64 b + 63
  const uint64_t obs = (uint64_t)(w0 < a.rows.NWR ? a.ab[w0] : 0u) | ((uint64_t)(w1 < a.rows.NWR ? a.ab[w1] : 0u) << 32);
  w &= obs;
  if (l == 0) a.tab[(size_t)q * a.hw + b] = w;
}

}  // namespace kb

// ---- host side -------------------------------------------------------------------------------------------
// the count and the scan of a.nsel lists on st (the caller has filled the masks); tot / nz: each list's total and its
// rows with a nonzero count.  ms: the device time of the span, added.
static int gp_totals(const char* who, const kb::GpArgs& a, hipStream_t st, CsTimer& tm, uint64_t tot[2], uint32_t nz[2]) {
  const uint32_t n = a.rows.C;
  kb::k_gp_count<<<(n + 3) / 4, 256, 0, st>>>(a);
  kb::k_gp_scan<<<a.nsel, 1024, 0, st>>>(a);
  tm.stop(st);
  HIPCHK(hipGetLastError());
  tot[1] = 0; nz[1] = 0;
  for (uint32_t s = 0; s < a.nsel; ++s)
    HIPCHK(hipMemcpyAsync(&tot[s], a.off + (size_t)s * ((size_t)n + 1) + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(nz, a.nz, 4ull * a.nsel, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  (void)who;
  return KB_OK;
}
// The lists whose want[s] is set, written by k_gp_emit into the handle's list buffer (grown to exactly the listed
// elements) and fetched into got[s]: pairs of words (pairs) or single ids.  ms: the device time of the launches.
static int gp_lists(kb_sim* h, const char* who, const kb::GpArgs& a, const bool want[2], const uint64_t tot[2], bool pairs,
                    std::vector<uint32_t> got[2], double* ms) {
  const uint64_t per = pairs ? 2 : 1;
  uint64_t words = 0;
  for (uint32_t s = 0; s < a.nsel; ++s) if (want[s]) words += per * tot[s];
  if (!words) return KB_OK;
  { const int rc = eng_grow(h, &h->gp_list, &h->gp_list_cap, (size_t)words); if (rc) return rc; }
  CsTimer tm;
  if (!tm.start(h->st)) { seterr(std::string(who) + ": events"); return KB_IO_ERROR; }
  uint64_t at = 0;
  for (uint32_t s = 0; s < a.nsel; ++s) {
    if (!want[s] || !tot[s]) continue;
    kb::k_gp_emit<<<(a.rows.C + 3) / 4, 256, 0, h->st>>>(a, s, pairs ? 1u : 0u, h->gp_list + at, tot[s]);
    at += per * tot[s];
  }
  tm.stop(h->st);
  HIPCHK(hipGetLastError());
  at = 0;
  for (uint32_t s = 0; s < a.nsel; ++s) {
    if (!want[s] || !tot[s]) continue;
    HIPCHK(fetch(got[s], h->gp_list + at, (size_t)(per * tot[s]), h->st));
    at += per * tot[s];
  }
  HIPCHK(hipStreamSynchronize(h->st));
  *ms += tm.ms();
  return KB_OK;
}

// a list argument: both or neither of the array and its capacity
static int gp_list_arg(const char* who, const void* p, size_t cap) {
  if ((p != nullptr) == (cap != 0)) return KB_OK;
  seterr(std::string(who) + (p ? ": a list with capacity 0" : ": a capacity without a list"));
  return KB_INVALID_ARGUMENT;
}

static const Refuse GP_REFUSE = {"; the lists are in row order across every rank's rows",
                                 "keep no member bits to list", nullptr};

// the dense table of the handle or group, checked for the 16-byte loads of the passes
static int gp_table(kb_sim* s, const char* who, kb::BitRows& t, kb_sim** h) {
  { const int rc = census_gate(s, who, GP_REFUSE); if (rc) return rc; }
  { const int rc = bit_rows(s, who, t, h); if (rc) return rc; }
  if ((*h)->d.NWR % 4 || (*h)->d.NWR != (*h)->W / 32) { seterr(std::string(who) + ": the row stride is not a multiple of 128 ids"); return KB_INVALID_OPERATION; }
  return KB_OK;
}

extern "C" int kb_sim_gaps(kb_sim* s, kb_gaps* out, uint32_t* missing_pairs, size_t cap_missing, uint32_t* stale_pairs,
                           size_t cap_stale) {
  static const char* who = "kb_sim_gaps";
  if (!s || !out) return KB_INVALID_ARGUMENT;
  { const int rc = gp_list_arg(who, missing_pairs, cap_missing); if (rc) return rc; }
  { const int rc = gp_list_arg(who, stale_pairs, cap_stale); if (rc) return rc; }
  kb::GpArgs a{};
  kb_sim* h = nullptr;
  { const int rc = gp_table(s, who, a.rows, &h); if (rc) return rc; }
  const Dev& d = h->d;
  const uint32_t C = s->C;
  kb::IdMasks m{};
  auto lay = [&](Carve& c) {                      // everything is written before it is read: nothing to clear
    m = carve_masks(c, d.NWR, true);
    a.off = c.take<uint64_t>(2ull * ((size_t)C + 1)); a.cnt = c.take<uint32_t>(2ull * C); a.nz = c.take<uint32_t>(2);
  };
  if (!h->gp_buf) HIPCHK(talloc(h, &h->gp_buf, (carve_bytes(lay) + 3) / 4));
  const Carve c = carve(h->gp_buf, lay);
  (void)c;
  a.active = m.ab; a.nsel = 2;
  a.sel[0] = kb::GpSel{m.ab, m.vb, 0xFFFFFFFFu};  // missing: ~bits & ab & vb
  a.sel[1] = kb::GpSel{m.sb, nullptr, 0u};        // stale: bits & sb
  CsTimer tm;
  if (!tm.start(h->st)) { seterr("gaps: events"); return KB_IO_ERROR; }
  id_masks(d.alive, d.ext, C, d.NWR, m, h->st);
  uint64_t tot[2]; uint32_t nz[2];
  { const int rc = gp_totals(who, a, h->st, tm, tot, nz); if (rc) return rc; }
  std::vector<uint8_t> alive;
  HIPCHK(fetch(alive, d.alive, C, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  double ms = tm.ms();
  const bool want[2] = {missing_pairs && tot[0] <= cap_missing, stale_pairs && tot[1] <= cap_stale};
  std::vector<uint32_t> got[2];
  { const int rc = gp_lists(h, who, a, want, tot, true, got, &ms); if (rc) return rc; }
  s->census_ms[CM_GAPS] = ms;
  memset(out, 0, sizeof *out);
  out->round = h->round;
  for (uint32_t i = 0; i < C; ++i) out->observers += alive[i] != 0;
  out->missing = tot[0]; out->stale = tot[1];
  out->rows_missing = nz[0]; out->rows_stale = nz[1];
  if (want[0]) { deliver(missing_pairs, got[0]); out->missing_listed = tot[0]; }
  if (want[1]) { deliver(stale_pairs, got[1]); out->stale_listed = tot[1]; }
  return KB_OK;
}

extern "C" int kb_sim_gaps_device_ms(kb_sim* s, double* ms) { return census_ms_get(s, CM_GAPS, ms); }

extern "C" int kb_sim_holders(kb_sim* s, const uint32_t* ids, size_t n_ids, uint64_t* offsets, uint32_t* rows, size_t cap_rows,
                              uint64_t* n_rows) {
  static const char* who = "kb_sim_holders";
  if (!s || !ids || !offsets) return KB_INVALID_ARGUMENT;
  if (n_ids == 0 || n_ids > KB_HOLDERS_MAX) { seterr(std::string(who) + ": the number of ids is outside 1 .. KB_HOLDERS_MAX"); return KB_INVALID_ARGUMENT; }
  { const int rc = gp_list_arg(who, rows, cap_rows); if (rc) return rc; }
  for (size_t q = 0; q < n_ids; ++q)
    if (ids[q] >= s->C) { seterr(std::string(who) + ": an id is not below the capacity"); return KB_INVALID_ARGUMENT; }
  kb::HdArgs ha{};
  kb_sim* h = nullptr;
  { const int rc = gp_table(s, who, ha.rows, &h); if (rc) return rc; }
  const Dev& d = h->d;
  const uint32_t C = s->C, nq = (uint32_t)n_ids;
  ha.nq = nq; ha.hw = ((C + 63) / 64 + 1) / 2 * 2;               // rows of 16-byte groups for the listing passes
  kb::GpArgs a{};
  kb::IdMasks m{};
  uint32_t* d_ids = nullptr;
  auto lay = [&](Carve& c) {
    m = carve_masks(c, d.NWR, false);
    ha.tab = c.take<uint64_t>((size_t)nq * ha.hw, 16); a.off = c.take<uint64_t>((size_t)nq + 1);
    d_ids = c.take<uint32_t>(nq); a.cnt = c.take<uint32_t>(nq); a.nz = c.take<uint32_t>(1);
  };
  { const int rc = eng_grow(h, &h->hd_buf, &h->hd_cap, carve_bytes(lay)); if (rc) return rc; }
  const Carve c = carve(h->hd_buf, lay);
  (void)c;
  ha.ab = m.ab; ha.ids = d_ids;
  bit_rows(reinterpret_cast<const uint32_t*>(ha.tab), nq, 2 * ha.hw, a.rows);
  a.active = nullptr; a.nsel = 1;
  a.sel[0] = kb::GpSel{nullptr, nullptr, 0u};                    // the table's bits as they are
  CsTimer tm;
  if (!tm.start(h->st)) { seterr("holders: events"); return KB_IO_ERROR; }
  HIPCHK(hipMemcpyAsync(d_ids, ids, 4ull * nq, hipMemcpyHostToDevice, h->st));
  id_masks(d.alive, nullptr, C, d.NWR, m, h->st);
  kb::k_hd_column<<<dim3((ha.hw + 3) / 4, nq), 256, 0, h->st>>>(ha);
  uint64_t tot[2]; uint32_t nz[2];
  { const int rc = gp_totals(who, a, h->st, tm, tot, nz); if (rc) return rc; }
  std::vector<uint64_t> off;
  HIPCHK(fetch(off, a.off, (size_t)nq + 1, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  double ms = tm.ms();
  const bool want[2] = {rows && tot[0] <= cap_rows, false};
  std::vector<uint32_t> got[2];
  { const int rc = gp_lists(h, who, a, want, tot, false, got, &ms); if (rc) return rc; }
  s->census_ms[CM_HOLDERS] = ms;
  deliver(offsets, off);
  if (n_rows) *n_rows = tot[0];
  if (want[0]) deliver(rows, got[0]);
  return KB_OK;
}

extern "C" int kb_sim_holders_device_ms(kb_sim* s, double* ms) { return census_ms_get(s, CM_HOLDERS, ms); }
