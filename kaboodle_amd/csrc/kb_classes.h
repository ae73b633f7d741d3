// kb_classes.h — the fingerprint-class census (include/kaboodle_classes.h): the running rows grouped
// by equal fingerprint, with each class's size and lowest id, the classes' canonical order (size descending, then
// fingerprint ascending) and, per row, the class it belongs to.  Included at the end of kb_sim.hip; reads the
// engines' fingerprints and running flags, writes only its own scratch.
//
// Four steps, every one integer adds, maxima and compares, so the result does not depend on the order in which
// anything arrives:
//   k_fc_count   a row's key goes into an open-addressing table of T >= 2 n slots {valid | key, count, ~lowest id}
//                in global memory.  The common case is one class holding nearly every row, and an atomic per row
//                on its counter would serialise (DESIGN.md §3 "Same-address atomics"), so a row's add is combined
//                three times on the way: the lanes of a wave that hold the first active lane's key add their
//                popcount once, a workgroup's 2048 rows meet in a 1024-slot LDS table, and the workgroup flushes
//                each LDS slot with one global add.  A key that finds no place within 8 LDS probes (more distinct
//                keys than the LDS table holds) goes to the global table directly.
//                The valid bit sits beside the key in one 64-bit word claimed by compare-and-swap: every 32-bit
//                value, 0 and 0xFFFFFFFF included, is a legal key, and an empty slot is the word 0.
//                The lowest id is kept as the maximum of ~id, so the zeroed table is its identity too.
//   k_fc_scan    one pass over the slots, 4096 per workgroup: classes, singletons, the size histogram, the
//                largest size, the true class (found by probing) and the classes ahead of it in canonical order.
//                In the same pass the workgroup sorts its slots' 64-bit keys (size << 32 | ~fp, descending: the
//                canonical order, and unique per class) in LDS and keeps the first 1024.
//   k_fc_merge   four such blocks in, the first 1024 of their union out, until one block is left; k_fc_list turns
//                it into {fp, size, rep} entries.  The host receives the summary words and at most 1024 entries.
//   k_fc_lookup  rep[i] and size[i]: a row probes the table for its key.
#pragma once
#include "../../include/kaboodle_classes.h"

namespace kb {

constexpr uint32_t FC_THREADS = 256;
constexpr uint32_t FC_PER = 8;                    // rows per thread in k_fc_count (every load before the first use)
constexpr uint32_t FC_ROWS = FC_THREADS * FC_PER; // rows per workgroup
constexpr uint32_t FC_LT = 1024;                  // LDS table slots (a power of two)
constexpr uint32_t FC_LPROBE = 8;                 // LDS probes before a key goes to the global table
constexpr uint32_t FC_TILE = 4096;                // slots per workgroup of k_fc_scan = keys one workgroup sorts
constexpr uint32_t FC_K = KB_FPC_LIST_MAX;        // keys a workgroup keeps
constexpr unsigned long long FC_VALID = 1ull << 32;
constexpr uint32_t FC_NOSLOT = 0xFFFFFFFFu;
// the summary words on the device
enum : uint32_t { FA_OBS = 0, FA_CLASSES, FA_SINGLE, FA_AHEAD, FA_LARGEST, FA_TRUE_SIZE, FA_TRUE_HERE, FA_HIST = 8, FA_WORDS = 40 };
static_assert(FC_TILE == 4 * FC_K && FC_TILE % FC_THREADS == 0 && (FC_LT & (FC_LT - 1)) == 0, "kb_classes.h tiling");

struct FcSlot { unsigned long long tag; uint32_t cnt; uint32_t inv; };   // tag = FC_VALID | key, or 0: empty
static_assert(sizeof(FcSlot) == 16, "a slot is one 16-byte load");

struct FcArgs {
  const uint32_t* fp; const uint8_t* run; uint32_t n;   // the rows: fingerprint, running flag
  FcSlot* tab; uint32_t mask;                     // the table: T slots, mask = T - 1 (zeroed)
  uint32_t* acc;                                  // [FA_WORDS] summary words (zeroed)
  uint32_t true_fp;
  uint32_t want_list;                             // k_fc_scan sorts and writes its block
  unsigned long long* cand;                       // k_fc_scan's blocks: [T / FC_TILE][FC_K] sort keys
  uint32_t* rep; uint32_t* size;                  // [n] k_fc_lookup's outputs
};

// a bijection of the 32-bit keys (the finaliser of MurmurHash3): keys that agree in any 16 bits still spread
__device__ __attribute__((always_inline)) inline uint32_t fc_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
__device__ __attribute__((always_inline)) inline unsigned long long fc_sortkey(uint32_t size, uint32_t fp) {
  return ((unsigned long long)size << 32) | (uint32_t)~fp;
}

// c rows of key `key`, the lowest of them id ~inv, into the global table.  A tag never changes once set, so a
// stale read of an empty slot only costs the compare-and-swap that then returns the owner.  The table holds at
// least twice as many slots as there are rows, so the probe ends; the bound keeps a broken caller from spinning.
__device__ inline void fc_glob_add(const FcArgs& a, uint32_t key, uint32_t c, uint32_t inv) {
  const unsigned long long tag = FC_VALID | key;
  uint32_t s = fc_mix(key) & a.mask;
  for (uint32_t p = 0; p <= a.mask; ++p, s = (s + 1) & a.mask) {
    unsigned long long cur = __hip_atomic_load(&a.tab[s].tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) { cur = atomicCAS(&a.tab[s].tag, 0ull, tag); if (cur == 0) cur = tag; }
    if (cur == tag) { atomicAdd(&a.tab[s].cnt, c); atomicMax(&a.tab[s].inv, inv); return; }
  }
}
// the slot of `key` in the finished table, FC_NOSLOT when no observer holds it
__device__ inline uint32_t fc_find(const FcArgs& a, uint32_t key) {
  const unsigned long long tag = FC_VALID | key;
  uint32_t s = fc_mix(key) & a.mask;
  for (uint32_t p = 0; p <= a.mask; ++p, s = (s + 1) & a.mask) {
    const unsigned long long cur = a.tab[s].tag;
    if (cur == tag) return s;
    if (cur == 0) break;
  }
  return FC_NOSLOT;
}

// grid: ceil(n / 2048) workgroups of 256 threads; thread t's rows are base + q * 256 + t
__global__ __launch_bounds__(FC_THREADS) void k_fc_count(FcArgs a) {
  __shared__ unsigned long long ltag[FC_LT];
  __shared__ uint32_t lcnt[FC_LT], linv[FC_LT];
  __shared__ uint32_t lobs;
  for (uint32_t k = threadIdx.x; k < FC_LT; k += FC_THREADS) { ltag[k] = 0; lcnt[k] = 0; linv[k] = 0; }
  if (threadIdx.x == 0) lobs = 0;
  __syncthreads();
  const uint32_t l = lane();
  const uint32_t base = blockIdx.x * FC_ROWS + threadIdx.x;     // n <= 2^30: no wrap
  uint32_t key[FC_PER]; bool on[FC_PER];
#pragma unroll
  for (uint32_t q = 0; q < FC_PER; ++q) {
    const uint32_t i = base + q * FC_THREADS;
    const bool in = i < a.n;
    const uint32_t f = in ? a.fp[i] : 0u;
    on[q] = in && a.run[i] != 0;
    key[q] = on[q] ? f : 0u;
  }
  uint32_t nobs = 0;                                            // wave-uniform
#pragma unroll
  for (uint32_t q = 0; q < FC_PER; ++q) {
    const uint64_t act = __ballot(on[q]);
    if (!act) continue;
    nobs += (uint32_t)__popcll(act);
    // the lanes that hold the first active lane's key add once between them; ids ascend with the lanes, so the
    // first of them holds the lowest id.  The other lanes add for themselves (the LDS table absorbs them)
    const uint32_t first = (uint32_t)__builtin_ctzll(act);
    const uint32_t k0 = rdl(key[q], (int)first);
    const uint64_t same = __ballot(on[q] && key[q] == k0);
    const bool lead = on[q] && key[q] == k0;
    if (on[q] && (!lead || l == first)) {
      const uint32_t c = lead ? (uint32_t)__popcll(same) : 1u;
      const uint32_t inv = ~(base + q * FC_THREADS);
      const unsigned long long tag = FC_VALID | key[q];
      uint32_t s = fc_mix(key[q]) >> 22;                        // the top 10 bits: FC_LT slots
      bool done = false;
      for (uint32_t p = 0; p < FC_LPROBE && !done; ++p, s = (s + 1) & (FC_LT - 1)) {
        const unsigned long long cur = atomicCAS(&ltag[s], 0ull, tag);
        if (cur == 0 || cur == tag) { atomicAdd(&lcnt[s], c); atomicMax(&linv[s], inv); done = true; }
      }
      if (!done) fc_glob_add(a, key[q], c, inv);
    }
  }
  if (l == 0 && nobs) atomicAdd(&lobs, nobs);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < FC_LT; k += FC_THREADS) {
    const unsigned long long t = ltag[k];
    if (t) fc_glob_add(a, (uint32_t)t, lcnt[k], linv[k]);
  }
  if (threadIdx.x == 0 && lobs) atomicAdd(&a.acc[FA_OBS], lobs);
}
static_assert(FC_LT == 1u << 10, "k_fc_count takes the LDS slot from the hash's top 10 bits");

// FC_TILE keys in LDS into descending order (a bitonic network; every thread of the workgroup calls it)
__device__ inline void fc_sort_desc(unsigned long long* sk) {
  for (uint32_t k = 2; k <= FC_TILE; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t x = threadIdx.x; x < FC_TILE / 2; x += FC_THREADS) {
        const uint32_t i = ((x & ~(j - 1)) << 1) | (x & (j - 1));   // the pair (i, i + j)
        const unsigned long long u = sk[i], v = sk[i + j];
        const bool desc = (i & k) == 0;
        if (desc ? u < v : u > v) { sk[i] = v; sk[i + j] = u; }
      }
      __syncthreads();
    }
  }
}

// grid: T / 4096 workgroups of 256 threads
__global__ __launch_bounds__(FC_THREADS) void k_fc_scan(FcArgs a) {
  __shared__ unsigned long long sk[FC_TILE];
  __shared__ uint32_t sacc[FA_WORDS];
  if (threadIdx.x < FA_WORDS) sacc[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t l = lane();
  // the true class: every thread probes the same few slots (one cached line)
  const uint32_t ts = fc_find(a, a.true_fp);
  const uint32_t tsize = ts != FC_NOSLOT ? a.tab[ts].cnt : 0u;
  const unsigned long long tkey = ts != FC_NOSLOT ? fc_sortkey(tsize, a.true_fp) : ~0ull;
  uint32_t ncls = 0, nsing = 0, nahead = 0, big = 0;
  const uint4* slots = reinterpret_cast<const uint4*>(a.tab);
  for (uint32_t q = 0; q < FC_TILE / FC_THREADS; ++q) {
    const uint32_t e = q * FC_THREADS + threadIdx.x;
    const uint4 v = slots[(size_t)blockIdx.x * FC_TILE + e];    // x: key, y: valid, z: count, w: ~lowest id
    const bool val = v.y != 0;
    const unsigned long long key = val ? fc_sortkey(v.z, v.x) : 0ull;   // a class has a row: its key is > 0
    if (a.want_list) sk[e] = key;
    ncls += val; nsing += val && v.z == 1; nahead += key > tkey;
    big = val && v.z > big ? v.z : big;
    // the histogram: one LDS add per distinct bin among the wave's slots
    const uint32_t b = val ? 31u - (uint32_t)__clz((int)v.z) : 32u;
    uint64_t act = __ballot(val);
    while (act) {
      const uint32_t b0 = rdl(b, __builtin_ctzll(act));
      const uint64_t same = __ballot(val && b == b0);
      if (l == 0) atomicAdd(&sacc[FA_HIST + b0], (uint32_t)__popcll(same));
      act &= ~same;
    }
  }
  ncls = wave_sum(ncls | (nsing << 16));                        // <= 1024 each per wave
  nahead = wave_sum(nahead);
  big = wave_max(big);
  if (l == 0) {
    if (ncls & 0xFFFFu) atomicAdd(&sacc[FA_CLASSES], ncls & 0xFFFFu);
    if (ncls >> 16) atomicAdd(&sacc[FA_SINGLE], ncls >> 16);
    if (nahead) atomicAdd(&sacc[FA_AHEAD], nahead);
    if (big) atomicMax(&sacc[FA_LARGEST], big);
  }
  __syncthreads();
  if (threadIdx.x < FA_WORDS) {                                 // a class costs the workgroup at most these adds
    const uint32_t v = sacc[threadIdx.x];
    if (v) { if (threadIdx.x == FA_LARGEST) atomicMax(&a.acc[FA_LARGEST], v); else atomicAdd(&a.acc[threadIdx.x], v); }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && ts != FC_NOSLOT) { a.acc[FA_TRUE_SIZE] = tsize; a.acc[FA_TRUE_HERE] = 1; }
  if (!a.want_list) return;
  unsigned long long* out = a.cand + (size_t)blockIdx.x * FC_K;
  if (sacc[FA_CLASSES] == 0) {                                  // workgroup-uniform: an empty tile
    for (uint32_t k = threadIdx.x; k < FC_K; k += FC_THREADS) out[k] = 0;
    return;
  }
  fc_sort_desc(sk);
  for (uint32_t k = threadIdx.x; k < FC_K; k += FC_THREADS) out[k] = sk[k];
}

// blocks 4g .. 4g+3 of `in` (nblk blocks of FC_K keys, each descending) -> block g of `out`: their first FC_K
__global__ __launch_bounds__(FC_THREADS) void k_fc_merge(const unsigned long long* in, uint32_t nblk, unsigned long long* out) {
  __shared__ unsigned long long sk[FC_TILE];
  int any = 0;
  for (uint32_t e = threadIdx.x; e < FC_TILE; e += FC_THREADS) {
    const uint32_t blk = blockIdx.x * 4 + e / FC_K;
    const unsigned long long v = blk < nblk ? in[(size_t)blk * FC_K + e % FC_K] : 0ull;
    sk[e] = v; any |= v != 0;
  }
  unsigned long long* o = out + (size_t)blockIdx.x * FC_K;
  if (!__syncthreads_or(any)) {
    for (uint32_t k = threadIdx.x; k < FC_K; k += FC_THREADS) o[k] = 0;
    return;
  }
  fc_sort_desc(sk);
  for (uint32_t k = threadIdx.x; k < FC_K; k += FC_THREADS) o[k] = sk[k];
}

// the first `cap` keys of the last block as {fp, size, rep, 0}; entries past the classes are left alone
__global__ void k_fc_list(FcArgs a, const unsigned long long* top, uint32_t cap, uint4* list) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cap) return;
  const unsigned long long key = top[k];
  if (!key) return;
  const uint32_t fp = ~(uint32_t)key;
  const uint32_t s = fc_find(a, fp);
  list[k] = make_uint4(fp, (uint32_t)(key >> 32), s != FC_NOSLOT ? ~a.tab[s].inv : KB_CENSUS_NONE, 0u);
}

__global__ __launch_bounds__(FC_THREADS) void k_fc_lookup(FcArgs a) {
  const uint32_t i = blockIdx.x * FC_THREADS + threadIdx.x;
  if (i >= a.n) return;
  uint32_t r = KB_CENSUS_NONE, z = 0;
  if (a.run[i]) {
    const uint32_t s = fc_find(a, a.fp[i]);
    if (s != FC_NOSLOT) { r = ~a.tab[s].inv; z = a.tab[s].cnt; }
  }
  a.rep[i] = r; a.size[i] = z;
}

}  // namespace kb

// ---- host side -------------------------------------------------------------------------------------------
// the scratch of a census over n rows, laid out by fc_lay: every part 16-byte aligned
struct FcPlan {
  uint32_t n = 0, T = 0, tiles = 0;
  uint32_t* acc = nullptr; FcSlot* tab = nullptr;   // the summary words and the table: cleared before every census
  unsigned long long* cand_a = nullptr; unsigned long long* cand_b = nullptr;
  kb_fp_class* list = nullptr;
  uint32_t* rep = nullptr; uint32_t* size = nullptr; uint32_t* fp = nullptr; uint8_t* run = nullptr;
};
static bool fc_plan(size_t n, FcPlan& p) {
  if (n > (1u << 30)) return false;
  size_t T = FC_TILE;
  while (T < 2 * n) T <<= 1;
  p.n = (uint32_t)n; p.T = (uint32_t)T; p.tiles = (uint32_t)(T / FC_TILE);
  return true;
}
static void fc_lay(Carve& c, FcPlan& p) {
  c.zero_from(); p.acc = c.take<uint32_t>(FA_WORDS, 16); p.tab = c.take<FcSlot>(p.T, 16); c.zero_to();
  p.cand_a = c.take<unsigned long long>((size_t)FC_K * p.tiles, 16); p.cand_b = c.take<unsigned long long>((size_t)FC_K * ((p.tiles + 3) / 4), 16);
  p.list = c.take<kb_fp_class>(FC_K, 16);
  p.rep = c.take<uint32_t>(p.n, 16); p.size = c.take<uint32_t>(p.n, 16); p.fp = c.take<uint32_t>(p.n, 16); p.run = c.take<uint8_t>(p.n, 16);
}
static_assert(sizeof(kb_fp_class) == 16, "kb_classes.h scratch layout");

struct FcSeg { const uint32_t* src; uint32_t lo, n; };            // a shard's fingerprints: rows [lo, lo + n)

static int fc_check(const void* out, const kb_fp_class* list, size_t cap_list, const uint32_t* rep, const uint32_t* size,
                    size_t cap_rows, size_t n, const char* who) {
  if (!out) return KB_INVALID_ARGUMENT;
  if (cap_list > KB_FPC_LIST_MAX) { seterr(std::string(who) + ": cap_list is above KB_FPC_LIST_MAX"); return KB_INVALID_ARGUMENT; }
  if (cap_list && !list) { seterr(std::string(who) + ": list is NULL with cap_list > 0"); return KB_INVALID_ARGUMENT; }
  return census_caps(who, out, nullptr, 0, 0, any_of(rep, size), cap_rows, n);
}

// The census over d_fp / d_run ([n], device) in the scratch laid out in `c` by fc_lay(c, p), on stream st.  With `segs` the
// fingerprints are first gathered from the shards into the scratch (inside the timed span).
static int fc_exec(const Carve& c, const FcPlan& p, hipStream_t st, const uint32_t* d_fp, const uint8_t* d_run,
                   const std::vector<FcSeg>* segs, uint32_t true_fp, int32_t round, kb_fp_classes* out, kb_fp_class* list,
                   size_t cap_list, size_t* n_list, uint32_t* rep, uint32_t* size, double* ms) {
  FcArgs a{};
  a.n = p.n; a.acc = p.acc; a.tab = p.tab; a.mask = p.T - 1;
  a.true_fp = true_fp; a.want_list = cap_list > 0;
  a.cand = p.cand_a; a.rep = p.rep; a.size = p.size;
  a.fp = d_fp; a.run = d_run;
  CsTimer tm;
  if (!tm.start(st)) { seterr("fp_classes: events"); return KB_IO_ERROR; }
  if (segs) {
    for (const FcSeg& sg : *segs)
      if (sg.n) HIPCHK(hipMemcpyAsync(p.fp + sg.lo, sg.src, 4ull * sg.n, hipMemcpyDeviceToDevice, st));
    a.fp = p.fp;
  }
  HIPCHK(hipMemsetAsync(c.zero_ptr(), 0, c.zero_bytes(), st));
  if (p.n) k_fc_count<<<(p.n + FC_ROWS - 1) / FC_ROWS, FC_THREADS, 0, st>>>(a);
  k_fc_scan<<<p.tiles, FC_THREADS, 0, st>>>(a);
  if (cap_list) {
    unsigned long long* src = a.cand;
    unsigned long long* dst = p.cand_b;
    for (uint32_t nblk = p.tiles; nblk > 1; nblk = (nblk + 3) / 4) {
      k_fc_merge<<<(nblk + 3) / 4, FC_THREADS, 0, st>>>(src, nblk, dst);
      std::swap(src, dst);
    }
    k_fc_list<<<(uint32_t)(cap_list + 255) / 256, 256, 0, st>>>(a, src, (uint32_t)cap_list, reinterpret_cast<uint4*>(p.list));
  }
  if ((rep || size) && p.n) k_fc_lookup<<<(p.n + FC_THREADS - 1) / FC_THREADS, FC_THREADS, 0, st>>>(a);
  tm.stop(st);
  HIPCHK(hipGetLastError());
  uint32_t acc[FA_WORDS];
  std::vector<kb_fp_class> got;
  HIPCHK(hipMemcpyAsync(acc, a.acc, sizeof acc, hipMemcpyDeviceToHost, st));
  HIPCHK(fetch(got, p.list, cap_list, st));
  if (rep && p.n) HIPCHK(hipMemcpyAsync(rep, a.rep, 4ull * p.n, hipMemcpyDeviceToHost, st));
  if (size && p.n) HIPCHK(hipMemcpyAsync(size, a.size, 4ull * p.n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (ms) *ms = tm.ms();
  memset(out, 0, sizeof *out);
  out->round = round;
  out->observers = acc[FA_OBS]; out->classes = acc[FA_CLASSES]; out->largest = acc[FA_LARGEST];
  out->singletons = acc[FA_SINGLE];
  out->true_fp = true_fp;
  out->true_size = acc[FA_TRUE_HERE] ? acc[FA_TRUE_SIZE] : 0u;
  out->true_rank = acc[FA_TRUE_HERE] ? acc[FA_AHEAD] : KB_CENSUS_NONE;
  for (uint32_t k = 0; k < 32; ++k) out->size_hist[k] = acc[FA_HIST + k];
  out->listed = (uint32_t)std::min<size_t>(out->classes, cap_list);
  for (uint32_t k = 0; k < out->listed; ++k) { list[k] = got[k]; out->listed_observers += got[k].size; }
  if (n_list) *n_list = out->listed;
  return KB_OK;
}

extern "C" int kb_sim_fp_classes(kb_sim* s, kb_fp_classes* out, kb_fp_class* list, size_t cap_list, size_t* n_list,
                                 uint32_t* rep, uint32_t* size, size_t cap_rows) {
  if (!s) return KB_INVALID_ARGUMENT;
  { const int rc = fc_check(out, list, cap_list, rep, size, cap_rows, s->C, "kb_sim_fp_classes"); if (rc) return rc; }
  { const int rc = census_gate(s, "kb_sim_fp_classes", {" and a class spans ranks", nullptr, nullptr}); if (rc) return rc; }
  const bool grp = is_group(s);
  (void)hipSetDevice(s->device);
  // what kb_sim_fingerprints does first: the rows whose view changed since their fingerprint was last taken
  { const int rc = route(s, R_ALL, 0, [&](auto* e) -> int {
      const int rc = eng_refresh_fps(e);
      if (!rc && grp) HIPCHK(hipStreamSynchronize(eng_stream(e)));
      return rc;
    });
    if (rc) return rc; }
  uint32_t tfp = 0;
  { const int rc = kb_sim_true_fingerprint(s, &tfp); if (rc) return rc; }
  FcPlan p;
  if (!fc_plan(s->C, p)) { seterr("kb_sim_fp_classes: capacity above 2^30"); return KB_CAPACITY; }
  // the scratch belongs to the engine whose stream runs the census (it is released with that engine)
  auto lay = [&](Carve& c) { fc_lay(c, p); };
  { const int rc = route(s, R_FIRST, 0, [&](auto* e) { return eng_grow(e, &s->fc_buf, &s->fc_cap, carve_bytes(lay)); }); if (rc) return rc; }
  const Carve c = carve(s->fc_buf, lay);
  std::vector<FcSeg> segs;
  if (grp) route(s, R_ALL, 0, [&](auto* e) { segs.push_back(FcSeg{eng_fp(e) + e->lo, e->lo, e->R}); return KB_OK; });
  // the first shard's stream runs the census; every shard is on its device
  return route(s, R_FIRST, 0, [&](auto* e) {
    return fc_exec(c, p, eng_stream(e), eng_fp(e), eng_alive(e), grp ? &segs : nullptr, tfp, e->round, out, list, cap_list,
                   n_list, rep, size, &s->census_ms[CM_CLASSES]);
  });
}

extern "C" int kb_sim_fp_classes_device_ms(kb_sim* s, double* ms) { return census_ms_get(s, CM_CLASSES, ms); }

extern "C" int kb_fp_classes_of(int device, const uint32_t* fps, const uint8_t* running, size_t n, uint32_t true_fp,
                                kb_fp_classes* out, kb_fp_class* list, size_t cap_list, size_t* n_list,
                                uint32_t* rep, uint32_t* size, size_t cap_rows) {
  { const int rc = fc_check(out, list, cap_list, rep, size, cap_rows, n, "kb_fp_classes_of"); if (rc) return rc; }
  if (n && (!fps || !running)) return KB_INVALID_ARGUMENT;
  OfScope o;
  { const int rc = o.open(device, "kb_fp_classes_of"); if (rc) return rc; }
  FcPlan p;
  if (!fc_plan(n, p)) { seterr("kb_fp_classes_of: more than 2^30 rows"); return KB_CAPACITY; }
  auto lay = [&](Carve& c) { fc_lay(c, p); };
  { const int rc = dev_reserve(&o.buf, &o.cap, carve_bytes(lay), "fp_classes: scratch allocation failed"); if (rc) return rc; }
  const Carve c = carve(o.buf, lay);
  if (n) {
    HIPCHK(hipMemcpyAsync(p.fp, fps, 4 * n, hipMemcpyHostToDevice, o.st));
    HIPCHK(hipMemcpyAsync(p.run, running, n, hipMemcpyHostToDevice, o.st));
  }
  return fc_exec(c, p, o.st, p.fp, p.run, nullptr, true_fp, -1, out, list, cap_list, n_list, rep, size, nullptr);
}
