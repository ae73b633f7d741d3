// kb_islands.h — the island census (include/kaboodle_islands.h): the connected components of the
// "i holds j" graph over the running peers, each labelled with its lowest id.  Included at the end of kb_sim.hip
// beside the other censuses; stands on the frame of kb_censusframe.h and on k_cs_masks of kb_census.h.  It reads the
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

constexpr uint32_t IS_SHARDS = 8;                 // XMAX
constexpr uint32_t IS_STEP_WORDS = 256;           // words a wave reads per step: 64 lanes x 16 bytes = 8192 ids
constexpr uint32_t IS_DENSE = 8;                  // members of a word from which its 32 labels are read in 16-byte loads

struct IsArgs {
  const uint32_t* bits[IS_SHARDS];                // every shard's member bits (biased: indexed by global row)
  uint32_t lo[IS_SHARDS];                         // its first row; 0xFFFFFFFF for unused entries
  const uint32_t* ab; const uint32_t* vb;         // [NWR] running ids, valid ids (k_cs_masks)
  uint32_t* L;                                    // [W] labels
  uint32_t* wmin; uint32_t* wmax;                 // [NWR] per word: min / max label over its running ids
  uint32_t* rown;                                 // [C] entries of each running row (zeroed)
  uint32_t* changed;                              // [1] the sweep lowered a label
  uint32_t C, NWR;                                // capacity, words per row (W/32, a multiple of IS_STEP_WORDS)
};

// the shard that holds row r: the last entry whose first row is <= r (lo[] ascending, lo[0] = 0, unused 0xFFFFFFFF:
// kb_sim_islands checks that before it launches)
__device__ __attribute__((always_inline)) inline const uint32_t* is_row(const IsArgs& a, uint32_t r) {
  const uint32_t* p = a.bits[0];
#pragma unroll
  for (uint32_t k = 1; k < IS_SHARDS; ++k) if (r >= a.lo[k]) p = a.bits[k];
  return p + (size_t)r * a.NWR;
}

// grid W / 256: a thread per id of the padded row
__global__ __launch_bounds__(256) void k_is_init(IsArgs a) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  a.L[j] = ((a.ab[j >> 5] >> (j & 31u)) & 1u) ? j : KB_CENSUS_NONE;
}

// grid W / 256: a thread per id; the 32 lanes of a half wave are one word
__global__ __launch_bounds__(256) void k_is_words(IsArgs a) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0) *a.changed = 0;
  const bool on = (a.ab[j >> 5] >> (j & 31u)) & 1u;
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
  if (i >= a.C) return;
  if (!((uint32_t)__builtin_amdgcn_readfirstlane((int)a.ab[i >> 5]) >> (i & 31u) & 1u)) return;   // scalar: the row is not read
  const uint4* row = reinterpret_cast<const uint4*>(is_row(a, i));
  const uint4* ab4 = reinterpret_cast<const uint4*>(a.ab);
  const uint4* vb4 = reinterpret_cast<const uint4*>(a.vb);
  const uint32_t steps = a.NWR / IS_STEP_WORDS;
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
// words of the pass's scratch: the three masks of k_cs_masks, the two word summaries, the labels, then (zeroed before
// every pass) the rows' entry counts and the changed word.  Every part but the last two is whole KiB, so the 16-byte
// loads of the masks and the labels are aligned.
static size_t is_scratch_words(uint32_t W, uint32_t C) { return 5ull * (W / 32) + W + C + 1; }

// The sweeps over the rows behind a.bits / a.lo with the running set dm.alive (dm: what k_cs_masks reads: C, NWR,
// alive, ext), scratch at `buf`, on stream st.
static int is_exec(uint32_t* buf, kb::IsArgs a, const Dev& dm, uint32_t W, hipStream_t st, IsPart& p) {
  const uint32_t C = a.C, NWR = a.NWR;
  CsDense m{};
  m.ab = buf; m.sb = m.ab + NWR; m.vb = m.sb + NWR;
  a.ab = m.ab; a.vb = m.vb; a.wmin = m.vb + NWR; a.wmax = a.wmin + NWR; a.L = a.wmax + NWR; a.rown = a.L + W;
  a.changed = a.rown + C;
  CsTimer tm;
  if (!tm.start(st)) { seterr("islands: events"); return KB_IO_ERROR; }
  HIPCHK(hipMemsetAsync(a.rown, 0, 4ull * ((size_t)C + 1), st));
  k_cs_masks<<<(NWR + 255) / 256, 256, 0, st>>>(dm, m);
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
  kb_sim* h = is_group(s) ? s->shards[0] : s;     // owns the scratch and the stream; every shard is on its device
  (void)hipSetDevice(h->device);
  if (is_group(s)) {
    const int rc = route(s, R_ALL, 0, [](auto* e) -> int { HIPCHK(hipStreamSynchronize(eng_stream(e))); return KB_OK; });
    if (rc) return rc;
  }
  const Dev& d = h->d;
  kb::IsArgs a{};
  a.C = s->C; a.NWR = d.NWR;
  for (uint32_t k = 0; k < IS_SHARDS; ++k) { a.bits[k] = d.bits; a.lo[k] = 0xFFFFFFFFu; }
  if (is_group(s)) {
    for (size_t k = 0; k < s->shards.size() && k < IS_SHARDS; ++k) { a.bits[k] = s->shards[k]->d.bits; a.lo[k] = s->shards[k]->lo; }
  }
  a.lo[0] = 0;
  {                                               // is_row's precondition: contiguous shards in row order, covering [0, C)
    const size_t ns = is_group(s) ? s->shards.size() : 1;
    bool ok = ns >= 1 && ns <= IS_SHARDS && (is_group(s) ? s->shards[0]->lo == 0 && s->shards[ns - 1]->hi == s->C : true);
    for (size_t k = 1; ok && k < ns; ++k) ok = s->shards[k]->lo == s->shards[k - 1]->hi && a.lo[k] > a.lo[k - 1];
    if (!ok) { seterr("kb_sim_islands: the group's shards are not contiguous in row order"); return KB_INVALID_OPERATION; }
  }
  if (h->W % 8192 || d.NWR != h->W / 32) { seterr("kb_sim_islands: the row stride is not a multiple of 8192 ids"); return KB_INVALID_OPERATION; }
  if (!h->is_buf) HIPCHK(talloc(h, &h->is_buf, is_scratch_words(h->W, s->C)));
  IsPart p;
  { const int rc = is_exec(h->is_buf, a, d, h->W, h->st, p); if (rc) return rc; }
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
  // the scratch first (whole KiB in front of its masks and labels), then the bit table (whole KiB each row), then the
  // running flags and as many zero bytes for the external set k_cs_masks reads
  const size_t scr_b = 4ull * is_scratch_words(W, C), o_bits = (scr_b + 255) & ~(size_t)255, bits_b = 4ull * C * NWR,
               o_run = o_bits + bits_b, o_ext = o_run + C;
  { const int rc = dev_reserve(&o.buf, &o.cap, o_ext + C, "kb_islands_of: device allocation failed"); if (rc) return rc; }
  char* b = static_cast<char*>(o.buf);
  HIPCHK(hipMemcpyAsync(b + o_bits, bits, bits_b, hipMemcpyHostToDevice, o.st));
  HIPCHK(hipMemcpyAsync(b + o_run, running, C, hipMemcpyHostToDevice, o.st));
  HIPCHK(hipMemsetAsync(b + o_ext, 0, C, o.st));
  Dev dm{};
  dm.C = C; dm.NWR = NWR; dm.alive = reinterpret_cast<uint8_t*>(b + o_run); dm.ext = reinterpret_cast<uint8_t*>(b + o_ext);
  kb::IsArgs a{};
  a.C = C; a.NWR = NWR;
  for (uint32_t k = 0; k < IS_SHARDS; ++k) { a.bits[k] = reinterpret_cast<const uint32_t*>(b + o_bits); a.lo[k] = 0xFFFFFFFFu; }
  a.lo[0] = 0;
  IsPart p;
  { const int rc = is_exec(reinterpret_cast<uint32_t*>(b), a, dm, W, o.st, p); if (rc) return rc; }
  return is_finish("kb_islands_of", p, -1, out, label, size);
}
