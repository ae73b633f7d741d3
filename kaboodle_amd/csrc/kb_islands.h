// kb_islands.h — the island census (include/kaboodle_islands.h): the connected components of the
// "i holds j" graph over the running peers, each labelled with its lowest id.  Included at the end of kb_sim.hip
// beside the other censuses; stands on the frame of kb_censusframe.h and kb_bitpass.h (masks, row table).  It reads the
// member bits and the running set only (never the stamps or the latency table) and writes only its own scratch.
//
// Labels: L[j] = j for a running id, KB_CENSUS_NONE otherwise.  A SWEEP is two launches.  k_is_words jumps every
// label one pointer (L[j] = L[L[j]]) and reduces the labels of every 32-id word to wmin[w] / wmax[w] over its running
// ids.  k_is_sweep gives a wave to each running row (a row that does not run is a scalar skip and is not read): the
// row is read in 16-byte loads, 8192 ids a step.  PULL: m = min(L[i], L of the row's running members); a word whose
// summary cannot lower m is skipped, a word whose running bits are all set takes wmin[w] with one load, a word with
// many members reads its 32 labels in eight 16-byte loads, the others walk their bits; then a wave min.  PUSH: every
// word with a running member and wmax[w] > m does atomicMin(&L[j], m) for its members whose label is larger (the
// label is read first; reading a dense word's 32 labels in 16-byte loads here too measured slower); then
// atomicMin(&L[i], m).  A lowering sets the `changed` word.  The host runs sweeps until one changes nothing.
//
// Why live updates and stale summaries are sound: labels only ever decrease, and every value a label ever held is
// an id of the same island (L[x] <= x throughout).  A stale wmin / wmax or a stale cached label is a value the label
// once held: pulling it is pulling an id of the island, and a prune against it skips only work a later sweep redoes.
// A sweep that lowers nothing read exact values everywhere (nothing was written), so every edge joins equal labels,
// and the one id of an island whose label is its own is the lowest.  The result is integer min only: order-free.
//
// No workgroup waits for another: there is no grid barrier, no wait on a value another workgroup writes, and no
// loop whose trip count another workgroup decides; every device loop is bounded by counts the host passes (or by
// the 32 bits of a word).  The kernels take IsArgs and do not reach into Dev, so kb_islands_of runs them on host
// arrays.
#pragma once
#include "../../include/kaboodle_islands.h"
#include "kb_islands_sum.h"

namespace kb {

constexpr uint32_t IS_STEP_WORDS = 256;           // words a wave reads per step: 64 lanes x 16 bytes = 8192 ids
constexpr uint32_t IS_DENSE = 8;                  // members of a word from which its 32 labels are read in 16-byte loads

struct IsArgs {
  BitRows rows;                                   // rows.C ids, rows.NWR = W/32 words a row (whole IS_STEP_WORDS)
  IdMasks m;                                      // k_id_masks: ab and vb
  uint32_t* L;                                    // [W] labels
  uint32_t* wmin; uint32_t* wmax;                 // [NWR] per word: min / max label over its running ids
  uint32_t* rown;                                 // [C] entries of each running row (zeroed)
  uint32_t* changed;                              // [1] the sweep lowered a label
};

// grid W / 256: a thread per id of the padded row
__global__ __launch_bounds__(256) void k_is_init(IsArgs a) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  a.L[j] = ((a.m.ab[j >> 5] >> (j & 31u)) & 1u) ? j : KB_CENSUS_NONE;
}

// grid W / 256: a thread per id; the 32 lanes of a half wave are one word
__global__ __launch_bounds__(256) void k_is_words(IsArgs a) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0) *a.changed = 0;
  const bool on = (a.m.ab[j >> 5] >> (j & 31u)) & 1u;
  uint32_t lo = 0xFFFFFFFFu, hi = 0;
  if (on) {
    const uint32_t x = a.L[j];                    // <= j < C: an id
    const uint32_t y = a.L[x];                    // <= x
    if (y < x) a.L[j] = y;                        // only this thread writes L[j] in this launch
    lo = hi = y < x ? y : x;
  }
#pragma unroll
  for (int k = 16; k >= 1; k >>= 1) {             // lane ^ k stays inside the 32-lane half
    const uint32_t ol = __shfl_xor(lo, k, 64), oh = __shfl_xor(hi, k, 64);
    lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
  }
  if ((j & 31u) == 0) { a.wmin[j >> 5] = lo; a.wmax[j >> 5] = hi; }
}

// min(m, the labels of the members x of word w), ab = the word's running ids
__device__ __attribute__((always_inline)) inline uint32_t is_pull(const IsArgs& a, uint32_t w, uint32_t x, uint32_t ab, uint32_t m) {
  if (!x) return m;
  const uint32_t wm = a.wmin[w];
  if (wm >= m) return m;                          // no label of the word was below m when the sweep began
  if (x == ab) return wm;                         // every running id of the word is a member
  if (__popc(x) >= IS_DENSE) {
    const uint4* p = reinterpret_cast<const uint4*>(a.L + (size_t)w * 32);
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      const uint4 v = p[k];
      const uint32_t b = x >> (4 * k);
      if ((b & 1u) && v.x < m) m = v.x;
      if ((b & 2u) && v.y < m) m = v.y;
      if ((b & 4u) && v.z < m) m = v.z;
      if ((b & 8u) && v.w < m) m = v.w;
    }
    return m;
  }
  for (; x; x &= x - 1) {
    const uint32_t v = a.L[w * 32 + (uint32_t)__builtin_ctz(x)];
    if (v < m) m = v;
  }
  return m;
}
// m goes to the members x of word w whose label is larger; true when one was lowered
__device__ __attribute__((always_inline)) inline bool is_push(const IsArgs& a, uint32_t w, uint32_t x, uint32_t m) {
  if (!x || a.wmax[w] <= m) return false;         // labels only decrease: none of the word's is above m
  bool chg = false;
  for (; x; x &= x - 1) {
    uint32_t* p = a.L + w * 32 + (uint32_t)__builtin_ctz(x);
    if (*p > m) chg |= atomicMin(p, m) > m;
  }
  return chg;
}

// grid ceil(C / 4), 256 threads: wave wv of block b owns row 4 b + wv
__global__ __launch_bounds__(256) void k_is_sweep(IsArgs a) {
  const uint32_t l = lane();
  const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (i >= a.rows.C) return;
  if (!((uint32_t)__builtin_amdgcn_readfirstlane((int)a.m.ab[i >> 5]) >> (i & 31u) & 1u)) return;   // scalar: the row is not read
  const uint4* row = reinterpret_cast<const uint4*>(bit_row(a.rows, i));
  const uint4* ab4 = reinterpret_cast<const uint4*>(a.m.ab);
  const uint4* vb4 = reinterpret_cast<const uint4*>(a.m.vb);
  const uint32_t steps = a.rows.NWR / IS_STEP_WORDS;
  uint32_t m = a.L[i], n = 0;
  for (uint32_t s = 0; s < steps; ++s) {
    const uint32_t g = s * 64 + l;                               // this lane's 16-byte group: words 4 g .. 4 g + 3
    const uint4 r = row[g], ab = ab4[g], vb = vb4[g];
    n += __popc(r.x & vb.x) + __popc(r.y & vb.y) + __popc(r.z & vb.z) + __popc(r.w & vb.w);
    m = is_pull(a, 4 * g + 0, r.x & ab.x, ab.x, m);
    m = is_pull(a, 4 * g + 1, r.y & ab.y, ab.y, m);
    m = is_pull(a, 4 * g + 2, r.z & ab.z, ab.z, m);
    m = is_pull(a, 4 * g + 3, r.w & ab.w, ab.w, m);
  }
  m = wave_min(m);
  n = wave_sum(n);
  bool chg = false;
  for (uint32_t s = 0; s < steps; ++s) {                         // the row again: from the cache it was just read into
    const uint32_t g = s * 64 + l;
    const uint4 r = row[g], ab = ab4[g];
    chg |= is_push(a, 4 * g + 0, r.x & ab.x, m);
    chg |= is_push(a, 4 * g + 1, r.y & ab.y, m);
    chg |= is_push(a, 4 * g + 2, r.z & ab.z, m);
    chg |= is_push(a, 4 * g + 3, r.w & ab.w, m);
  }
  if (l == 0) {
    a.rown[i] = n;
    if (a.L[i] > m) chg |= atomicMin(&a.L[i], m) > m;
  }
  if (__ballot(chg) && l == 0) *a.changed = 1;
}

}  // namespace kb

// ---- host side -------------------------------------------------------------------------------------------
struct IsPart {
  std::vector<uint32_t> label, rown;              // [C]: KB_CENSUS_NONE where the id does not run; row entries
  uint32_t sweeps = 0;
  double ms = 0;
};
// the scratch (a.rows set): masks, labels (16-byte loads), word summaries; cleared every pass: entry counts, changed
static void is_lay(Carve& c, kb::IsArgs& a, uint32_t W) {
  const uint32_t C = a.rows.C, NWR = a.rows.NWR;
  a.m = carve_masks(c, NWR, false);
  a.L = c.take<uint32_t>(W, 16); a.wmin = c.take<uint32_t>(NWR); a.wmax = c.take<uint32_t>(NWR);
  c.zero_from(); a.rown = c.take<uint32_t>(C); a.changed = c.take<uint32_t>(1); c.zero_to();
}

// the sweeps over a.rows with the running set `alive` ([C], device), scratch laid out in `c` by is_lay, on stream st
static int is_exec(const Carve& c, const kb::IsArgs& a, const uint8_t* alive, uint32_t W, hipStream_t st, IsPart& p) {
  const uint32_t C = a.rows.C;
  CsTimer tm;
  if (!tm.start(st)) { seterr("islands: events"); return KB_IO_ERROR; }
  HIPCHK(hipMemsetAsync(c.zero_ptr(), 0, c.zero_bytes(), st));
  id_masks(alive, nullptr, C, a.rows.NWR, a.m, st);
  k_is_init<<<W / 256, 256, 0, st>>>(a);
  HIPCHK(hipGetLastError());
  p.sweeps = 0;
  for (;;) {
    if (p.sweeps > C) { seterr("islands: the labels have not settled after capacity + 1 sweeps"); return KB_IO_ERROR; }
    k_is_words<<<W / 256, 256, 0, st>>>(a);
    k_is_sweep<<<(C + 3) / 4, 256, 0, st>>>(a);
    ++p.sweeps;
    tm.stop(st);                                                 // recorded again after every sweep: the last one stands
    HIPCHK(hipGetLastError());
    uint32_t changed = 0;
    HIPCHK(hipMemcpyAsync(&changed, a.changed, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!changed) break;
  }
  HIPCHK(fetch(p.label, a.L, C, st));
  HIPCHK(fetch(p.rown, a.rown, C, st));
  HIPCHK(hipStreamSynchronize(st));
  p.ms = tm.ms();
  return KB_OK;
}

static int is_finish(const char* who, const IsPart& p, int32_t round, kb_islands* out, uint32_t* label, uint32_t* size) {
  if (!is_summary(p.label, p.rown, round, p.sweeps, out, size)) {
    seterr(std::string(who) + ": the settled labels are not the lowest ids of their islands");
    return KB_IO_ERROR;
  }
  deliver(label, p.label);
  return KB_OK;
}

static const Refuse IS_REFUSE = {"; an island spans ranks", "need an algorithm of their own: a based row holds the whole base set implicitly (not built yet)", nullptr};

extern "C" int kb_sim_islands(kb_sim* s, kb_islands* out, uint32_t* label, uint32_t* size, size_t cap_ids) {
  if (!s) return KB_INVALID_ARGUMENT;
  { const int rc = census_caps("kb_sim_islands", out, any_of(label, size), cap_ids, s->C, nullptr, 0, 0); if (rc) return rc; }
  { const int rc = census_gate(s, "kb_sim_islands", IS_REFUSE); if (rc) return rc; }
  kb::IsArgs a{};
  kb_sim* h = nullptr;
  { const int rc = bit_rows(s, "kb_sim_islands", a.rows, &h); if (rc) return rc; }
  const Dev& d = h->d;
  if (h->W % 8192 || d.NWR != h->W / 32) { seterr("kb_sim_islands: the row stride is not a multiple of 8192 ids"); return KB_INVALID_OPERATION; }
  auto lay = [&](Carve& c) { is_lay(c, a, h->W); };
  if (!h->is_buf) HIPCHK(talloc(h, &h->is_buf, carve_bytes(lay) / 4));
  const Carve c = carve(h->is_buf, lay);
  IsPart p;
  { const int rc = is_exec(c, a, d.alive, h->W, h->st, p); if (rc) return rc; }
  s->census_ms[CM_ISLANDS] = p.ms;
  return is_finish("kb_sim_islands", p, h->round, out, label, size);
}

extern "C" int kb_sim_islands_device_ms(kb_sim* s, double* ms) { return census_ms_get(s, CM_ISLANDS, ms); }

extern "C" int kb_islands_of(int device, const uint32_t* bits, const uint8_t* running, size_t capacity, kb_islands* out,
                             uint32_t* label, uint32_t* size, size_t cap_ids) {
  { const int rc = census_caps("kb_islands_of", out, any_of(label, size), cap_ids, capacity, nullptr, 0, 0); if (rc) return rc; }
  if (capacity == 0 || capacity > (1u << 24)) { seterr("kb_islands_of: capacity outside 1 .. 2^24"); return KB_CAPACITY; }
  if (!bits || !running) return KB_INVALID_ARGUMENT;
  OfScope o;
  { const int rc = o.open(device, "kb_islands_of"); if (rc) return rc; }
  const uint32_t C = (uint32_t)capacity, W = (C + 8191) / 8192 * 8192, NWR = W / 32;
  kb::IsArgs a{};
  uint32_t* tab = nullptr; uint8_t* run = nullptr;
  auto lay = [&](Carve& c) {                      // the bit table (16-byte loads), the running flags, then the pass's scratch
    tab = c.take<uint32_t>((size_t)C * NWR, 16); run = c.take<uint8_t>(C);
    bit_rows(tab, C, NWR, a.rows);
    is_lay(c, a, W);
  };
  { const int rc = dev_reserve(&o.buf, &o.cap, carve_bytes(lay), "kb_islands_of: device allocation failed"); if (rc) return rc; }
  const Carve c = carve(o.buf, lay);
  HIPCHK(hipMemcpyAsync(tab, bits, 4ull * C * NWR, hipMemcpyHostToDevice, o.st));
  HIPCHK(hipMemcpyAsync(run, running, C, hipMemcpyHostToDevice, o.st));
  IsPart p;
  { const int rc = is_exec(c, a, run, W, o.st, p); if (rc) return rc; }
  return is_finish("kb_islands_of", p, -1, out, label, size);
}
