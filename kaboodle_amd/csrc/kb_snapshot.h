// kb_snapshot.h — snapshot and restore of a sparse-row mesh (include/kaboodle_snapshot.h).  Included
// at the end of kb_sim.hip.  kb_sim_snapshot reads the sparse engine's state and writes only its own scratch;
// kb_sim_restore creates a handle from the stored config and overwrites its tables.  Dense handles refuse.
//
// The rows' entry lists are allocated as C x ESTR words and use a small part of that, so they travel packed: an
// exclusive scan of `ne` over the handle's rows (64-bit offsets: 4M rows x 2048 entries is 2^33), then an
// ENTRY-parallel copy, thread p of the packed buffer finding its row by a binary search in the offsets.  Writes are
// contiguous over the whole grid for converged rows of 0-4 entries and for a joiner's row of ECAP entries alike,
// reads are contiguous inside a row, and no thread's work depends on a row's length.  Unpack is the inverse, and
// the thread holding a row's last entry zeroes the rest of its 16-byte group (the row kernels load rows as uint4).
// Plain kernels on the handle's stream: the scan is three launches (tile sums, the tiles' scan by one workgroup
// over a count the host passes, offsets), nothing waits on another workgroup.
#pragma once
#include "../../include/kaboodle_snapshot.h"

namespace kb {

constexpr uint32_t SN_TILE = 1024;                 // rows per scan tile

// ne summed per tile of SN_TILE rows (ne: the shard's local base)
__global__ __launch_bounds__(1024) void k_sn_tile_sums(const uint32_t* __restrict__ ne, uint32_t R, unsigned long long* __restrict__ tile) {
  const uint32_t k = blockIdx.x * SN_TILE + threadIdx.x;
  const unsigned long long t = block_sum(k < R ? ne[k] : 0u);
  if (threadIdx.x == 0) tile[blockIdx.x] = t;
}
// one workgroup: tile[0 .. nt) becomes its exclusive scan, tile[nt] the total
__global__ __launch_bounds__(1024) void k_sn_tile_scan(unsigned long long* tile, uint32_t nt) {
  __shared__ unsigned long long s[1024];
  const uint32_t t = threadIdx.x, per = (nt + 1023u) / 1024u;
  const uint32_t a = t * per, b = a + per < nt ? a + per : nt;
  unsigned long long sum = 0;
  for (uint32_t k = a; k < b; ++k) sum += tile[k];
  s[t] = sum;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {         // inclusive scan of the 1024 partial sums
    const unsigned long long x = t >= o ? s[t - o] : 0ull;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  unsigned long long run = s[t] - sum;
  for (uint32_t k = a; k < b; ++k) { const unsigned long long v = tile[k]; tile[k] = run; run += v; }
  if (t == 1023) tile[nt] = s[1023];
}
// off[k] = entries of the shard's rows before local row k, k in [0, R]; off[R] the total
__global__ __launch_bounds__(1024) void k_sn_offsets(const uint32_t* __restrict__ ne, uint32_t R, const unsigned long long* __restrict__ tile,
                                                     uint32_t nt, unsigned long long* __restrict__ off) {
  __shared__ uint32_t ws[16];
  const uint32_t k = blockIdx.x * SN_TILE + threadIdx.x, w = threadIdx.x >> 6;
  const uint32_t v = k < R ? ne[k] : 0u;
  uint32_t inc = v;                                 // a tile holds at most 1024 x 4096 entries: 32 bits inside it
  for (int o = 1; o < 64; o <<= 1) { const uint32_t x = __shfl_up(inc, o, 64); if ((threadIdx.x & 63u) >= (uint32_t)o) inc += x; }
  if ((threadIdx.x & 63u) == 63u) ws[w] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (uint32_t q = 0; q < w; ++q) base += ws[q];
  if (k < R) off[k] = tile[blockIdx.x] + base + (inc - v);
  if (k == 0) off[R] = tile[nt];
}
// the canonical fingerprint column: a stale cache entry is stored as the fold it stands for (nothing is written back)
__global__ __launch_bounds__(256) void k_sn_fp(SpDev d, uint32_t* __restrict__ out) {
  const uint32_t i = sp_gid(d);
  if (i >= d.hi) return;
  out[i - d.lo] = d.dirty[i] ? sp_fold(d, i) : d.fp[i];
}
// the local row holding packed entry p: the last k with off[k] <= p (empty rows share an offset with their successor)
__device__ inline uint32_t sn_row_of(const unsigned long long* __restrict__ off, uint32_t R, unsigned long long p) {
  uint32_t lo = 0, hi = R;                          // off[lo] <= p < off[hi]
  while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= p) lo = mid; else hi = mid; }
  return lo;
}
__global__ __launch_bounds__(256) void k_sn_pack(SpDev d, const unsigned long long* __restrict__ off, unsigned long long total,
                                                 uint32_t* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (p >= total) return;
  const uint32_t k = sn_row_of(off, d.hi - d.lo, p);
  out[p] = sp_row(d, d.lo + k)[p - off[k]];
}
// the host has checked every row's length against ECAP and the lengths' sum against `total`
__global__ __launch_bounds__(256) void k_sn_unpack(SpDev d, const unsigned long long* __restrict__ off, unsigned long long total,
                                                   const uint32_t* __restrict__ in) {
  const unsigned long long p = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (p >= total) return;
  const uint32_t k = sn_row_of(off, d.hi - d.lo, p);
  uint32_t* e = sp_row(d, d.lo + k);
  const uint32_t q = (uint32_t)(p - off[k]), n = (uint32_t)(off[k + 1] - off[k]);
  if (q >= d.ECAP) return;
  e[q] = in[p];
  if (q + 1 == n) for (uint32_t t = q + 1; t & 3u; ++t) e[t] = 0;   // ESTR is a multiple of 4: inside the row
}

}  // namespace kb

// ---- the format (little-endian; every section starts on an 8-byte boundary, padding is zero) -------------------
//   SnHdr | SnSec[SN_NSEC] | the sections in the order of SnId
// Row tables hold C rows in global id order, per-id tables C elements; payload_crc32 covers everything after SnHdr.
static const char SN_MAGIC[8] = {'K', 'B', 'S', 'N', 'A', 'P', 'L', 'E'};
struct SnHdr {
  char magic[8];
  uint32_t format_version, abi_version;
  uint32_t header_bytes, cfg_bytes;                 // sizeof(SnHdr), sizeof(kb_config)
  kb_config cfg;                                    // as created, device = -1
  int32_t round; uint32_t alive;
  uint64_t entries, bytes;
  uint32_t payload_crc32, nsect;
};
struct SnSec { uint32_t id, elem; uint64_t off, count; };
struct SnScalars {
  int32_t round; uint32_t nj, nf, pad0;             // the Join / Failed lists the next round delivers
  uint64_t bj_total, bf_total;
  uint32_t next_free, first_conv, last_conv, last_agree, last_alive, pad1;   // CtrIdx: the mesh-wide values
};
static_assert(sizeof(SnHdr) % 8 == 0 && sizeof(SnSec) == 24 && sizeof(SnScalars) == 56, "snapshot layout");
static_assert(sizeof(kb::Susp) == 16 && sizeof(kb::Cur) == 32 && sizeof(kb::BCast) == 16, "snapshot layout");
enum SnId : uint32_t {
  SN_SCALARS, SN_STATS, SN_NE, SN_BASED, SN_N, SN_FP, SN_LAST_BCAST, SN_A3CUR, SN_SUSP, SN_CUR, SN_PAQ, SN_PAQ_N,
  SN_ALIVE, SN_START_ROUND, SN_IDSET, SN_EXT, SN_IDENT, SN_IDLEN, SN_PEND, SN_PENDLEN, SN_MOVED, SN_BJOIN, SN_BFAIL,
  SN_ENTRIES, SN_NSEC
};
static void sn_layout(uint32_t C, uint32_t nj, uint32_t nf, uint64_t entries, SnSec* s, uint64_t* bytes) {
  const uint32_t elem[SN_NSEC] = {sizeof(SnScalars), 8, 4, 1, 4, 4, 4, 4, 16 * kb::SLOTS, 32 * kb::CSLOTS, 4 * kb::PAQ, 4,
                                  1, 4, 1, 1, kb::MAXID, 1, kb::MAXID, 2, 1, 16, 16, 4};
  uint64_t at = sizeof(SnHdr) + sizeof(SnSec) * SN_NSEC;
  for (uint32_t k = 0; k < SN_NSEC; ++k) {
    s[k].id = k; s[k].elem = elem[k]; s[k].off = at;
    s[k].count = k == SN_SCALARS ? 1 : k == SN_STATS ? (uint64_t)kb::NSTAT : k == SN_BJOIN ? nj : k == SN_BFAIL ? nf :
                 k == SN_ENTRIES ? entries : C;
    at = (at + s[k].elem * s[k].count + 7ull) & ~7ull;
  }
  *bytes = at;
}
static uint32_t sn_ecap(const kb_config& c) {       // sp_create's ECAP
  return c.sparse_row_cap ? std::min<uint32_t>(c.sparse_row_cap, c.capacity) : std::min<uint32_t>(c.capacity, 4096u);
}
static uint32_t sn_crc(const uint8_t* p, size_t n) { h_crc_init(); return h_crc_update(0xFFFFFFFFu, p, n) ^ 0xFFFFFFFFu; }

// the header, the checksum and the section table of a snapshot, before any device call
static int sn_parse(const void* buf, size_t len, SnHdr* h, SnSec* sec) {
  if (!buf) { seterr("snapshot: null buffer"); return KB_INVALID_ARGUMENT; }
  if (len < sizeof(SnHdr)) { seterr("snapshot: short buffer, truncated inside the header"); return KB_INVALID_ARGUMENT; }
  memcpy(h, buf, sizeof *h);
  if (memcmp(h->magic, SN_MAGIC, sizeof SN_MAGIC) != 0) { seterr("snapshot: bad magic (not a little-endian kaboodle snapshot)"); return KB_INVALID_ARGUMENT; }
  if (h->format_version != KB_SNAPSHOT_VERSION) {
    seterr("snapshot: unknown format_version " + std::to_string(h->format_version) + " (this library reads " + std::to_string(KB_SNAPSHOT_VERSION) + ")");
    return KB_INVALID_ARGUMENT;
  }
  if (h->abi_version != KB_ABI_VERSION || h->cfg_bytes != sizeof(kb_config) || h->header_bytes != sizeof(SnHdr)) {
    seterr("snapshot: written under abi_version " + std::to_string(h->abi_version) + " with sizeof(kb_config) " + std::to_string(h->cfg_bytes) +
           " (this library: " + std::to_string(KB_ABI_VERSION) + ", " + std::to_string(sizeof(kb_config)) + ")");
    return KB_INVALID_ARGUMENT;
  }
  if ((uint64_t)len < h->bytes) {
    seterr("snapshot: short buffer, truncated at " + std::to_string(len) + " of " + std::to_string(h->bytes) + " bytes");
    return KB_INVALID_ARGUMENT;
  }
  if ((uint64_t)len > h->bytes || h->bytes < sizeof(SnHdr) + sizeof(SnSec) * SN_NSEC || h->nsect != SN_NSEC) {
    seterr("snapshot: the header's length or section count does not fit the buffer"); return KB_INVALID_ARGUMENT;
  }
  const uint8_t* b = static_cast<const uint8_t*>(buf);
  if (sn_crc(b + sizeof(SnHdr), len - sizeof(SnHdr)) != h->payload_crc32) { seterr("snapshot: payload checksum mismatch"); return KB_INVALID_ARGUMENT; }
  const kb_config& c = h->cfg;
  if (c.abi_version != KB_ABI_VERSION || c.capacity == 0 || c.capacity > 7800000u || !(c.variant & KB_VARIANT_SPARSE_ROWS)) {
    seterr("snapshot: the stored config is not a sparse-row mesh of this ABI"); return KB_INVALID_ARGUMENT;
  }
  memcpy(sec, b + sizeof(SnHdr), sizeof(SnSec) * SN_NSEC);
  SnSec want[SN_NSEC];
  uint64_t total = 0;
  sn_layout(c.capacity, (uint32_t)sec[SN_BJOIN].count, (uint32_t)sec[SN_BFAIL].count, h->entries, want, &total);
  for (uint32_t k = 0; k < SN_NSEC; ++k) {
    // (counts are bounded before they are multiplied: a list holds at most C x SLOTS records, a row ECAP entries)
    const bool fits = sec[k].count <= (uint64_t)c.capacity * 4096ull && sec[k].off <= len && (uint64_t)sec[k].elem * sec[k].count <= len - sec[k].off;
    if (!fits) { seterr("snapshot: section " + std::to_string(k) + " runs past the end of the buffer"); return KB_INVALID_ARGUMENT; }
    if (sec[k].id != want[k].id || sec[k].elem != want[k].elem || sec[k].count != want[k].count || sec[k].off != want[k].off) {
      seterr("snapshot: section " + std::to_string(k) + " is not laid out as format_version 1 lays it out"); return KB_INVALID_ARGUMENT;
    }
  }
  if (total != h->bytes) { seterr("snapshot: the sections do not add up to the header's length"); return KB_INVALID_ARGUMENT; }
  return KB_OK;
}
template <class T> static const T* sn_at(const void* buf, const SnSec* sec, SnId k) {
  return reinterpret_cast<const T*>(static_cast<const uint8_t*>(buf) + sec[k].off);
}
// the values a restore hands to kernels as indices and lengths, checked on the host first
static int sn_check_values(const void* buf, const SnHdr& h, const SnSec* sec) {
  const uint32_t C = h.cfg.capacity, ECAP = sn_ecap(h.cfg);
  const auto bad = [](const char* what) { seterr(std::string("snapshot: a section holds values out of range (") + what + ")"); return KB_INVALID_ARGUMENT; };
  SnScalars sc;
  memcpy(&sc, sn_at<uint8_t>(buf, sec, SN_SCALARS), sizeof sc);
  if (sc.nj != sec[SN_BJOIN].count || sc.nf != sec[SN_BFAIL].count || sc.nj > C || sc.nf > (uint64_t)C * kb::SLOTS || sc.round < 0 ||
      sc.round != h.round || sc.next_free > C) return bad("scalars");
  const uint32_t* ne = sn_at<uint32_t>(buf, sec, SN_NE);
  uint64_t sum = 0;
  for (uint32_t i = 0; i < C; ++i) { if (ne[i] > ECAP) return bad("a row longer than sparse_row_cap"); sum += ne[i]; }
  if (sum != h.entries) return bad("the rows' lengths do not add up to the entries");
  const uint32_t* ent = sn_at<uint32_t>(buf, sec, SN_ENTRIES);
  for (uint64_t p = 0; p < h.entries; ++p) if ((ent[p] >> 9) >= C) return bad("an entry's id");
  // rows the engine never writes, which its list routines assume away: sp_lb searches a row as strictly ascending
  // ids, sp_put keeps no entry without x or a stamp, and `based` is read as a flag
  const uint8_t* based = sn_at<uint8_t>(buf, sec, SN_BASED);
  uint64_t p = 0;
  for (uint32_t i = 0; i < C; ++i) {
    if (based[i] > 1) return bad("a based flag above 1");
    for (uint32_t q = 0; q < ne[i]; ++q, ++p) {
      if (q && (ent[p] >> 9) <= (ent[p - 1] >> 9)) return bad("a row's ids are not strictly ascending");
      if (!(ent[p] & 0x1FFu)) return bad("an entry with neither x nor a stamp");
    }
  }
  const uint32_t* paq_n = sn_at<uint32_t>(buf, sec, SN_PAQ_N);
  const uint32_t* paq = sn_at<uint32_t>(buf, sec, SN_PAQ);
  const uint32_t* a3 = sn_at<uint32_t>(buf, sec, SN_A3CUR);
  const kb::Susp* su = sn_at<kb::Susp>(buf, sec, SN_SUSP);
  const kb::Cur* cu = sn_at<kb::Cur>(buf, sec, SN_CUR);
  const uint8_t* idlen = sn_at<uint8_t>(buf, sec, SN_IDLEN);
  const int16_t* pendlen = sn_at<int16_t>(buf, sec, SN_PENDLEN);
  for (uint32_t i = 0; i < C; ++i) {
    if (paq_n[i] > (uint32_t)kb::PAQ || a3[i] >= C) return bad("ping_addrs queue / A3 cursor");
    for (uint32_t q = 0; q < paq_n[i]; ++q) if (paq[(size_t)i * kb::PAQ + q] >= C) return bad("ping_addrs id");
    for (int q = 0; q < kb::SLOTS; ++q) if (su[(size_t)i * kb::SLOTS + q].kind && su[(size_t)i * kb::SLOTS + q].peer >= C) return bad("suspect slot");
    for (int q = 0; q < kb::CSLOTS; ++q) {
      const kb::Cur& x = cu[(size_t)i * kb::CSLOTS + q];
      if (!x.used) continue;
      if (x.peer >= C || x.nobs > (uint32_t)kb::NOBS) return bad("curious slot");
      for (uint32_t o = 0; o < x.nobs; ++o) if (x.obs[o] >= C) return bad("curious observer");
    }
    if (idlen[i] > kb::MAXID || pendlen[i] > kb::MAXID) return bad("identity length");
  }
  const kb::BCast* bj = sn_at<kb::BCast>(buf, sec, SN_BJOIN);
  const kb::BCast* bf = sn_at<kb::BCast>(buf, sec, SN_BFAIL);
  for (uint32_t k = 0; k < sc.nj; ++k) if (bj[k].sender >= C || bj[k].peer >= C) return bad("Join list");
  for (uint32_t k = 0; k < sc.nf; ++k) if (bf[k].sender >= C || bf[k].peer >= C) return bad("Failed list");
  return KB_OK;
}

extern "C" int kb_snapshot_info_of(const void* buf, size_t len, kb_snapshot_info* out) {
  if (!out) return KB_INVALID_ARGUMENT;
  SnHdr h;
  SnSec sec[SN_NSEC];
  { const int rc = sn_parse(buf, len, &h, sec); if (rc) return rc; }
  { const int rc = sn_check_values(buf, h, sec); if (rc) return rc; }   // as kb_sim_restore: the header's promise
  memset(out, 0, sizeof *out);
  out->format_version = h.format_version; out->abi_version = h.abi_version; out->cfg = h.cfg;
  out->round = h.round; out->alive = h.alive; out->entries = h.entries; out->bytes = h.bytes; out->payload_crc32 = h.payload_crc32;
  return KB_OK;
}

// ---- one leaf's part (route() hands every shard of a group here in turn) ----------------------------------------
static int sn_dense() { seterr("snapshot: dense rows are not answered (KB_VARIANT_SPARSE_ROWS handles are)"); return KB_INVALID_OPERATION; }
// the leaf's scratch: [R + 1] offsets, [nt + 1] tile sums, [R] canonical fingerprints
struct SnScratch { unsigned long long* off; unsigned long long* tile; uint32_t* fp; uint32_t nt; };
static int sn_scratch(SpSim* S, SnScratch* x) {
  const uint32_t R = S->R, nt = (R + kb::SN_TILE - 1) / kb::SN_TILE;
  if (!S->sn_fix && sp_alloc(S, &S->sn_fix, (size_t)R + 1 + nt + 1 + (R + 1) / 2) != hipSuccess) {
    seterr("snapshot: device allocation failed"); return KB_CAPACITY;
  }
  x->off = S->sn_fix; x->tile = x->off + R + 1; x->fp = reinterpret_cast<uint32_t*>(x->tile + nt + 1); x->nt = nt;
  return KB_OK;
}
static void sn_scan(SpSim* S, const SnScratch& x) {
  const uint32_t* ne = SL(S, S->d.ne);
  kb::k_sn_tile_sums<<<x.nt, 1024, 0, S->st>>>(ne, S->R, x.tile);
  kb::k_sn_tile_scan<<<1, 1024, 0, S->st>>>(x.tile, x.nt);
  kb::k_sn_offsets<<<x.nt, 1024, 0, S->st>>>(ne, S->R, x.tile, x.nt, x.off);
}
static uint32_t sn_grid(uint64_t total) { return (uint32_t)((total + 255ull) / 256ull); }   // <= 2^33 / 2^8 workgroups

static int sn_queued(kb_sim*) { return sn_dense(); }
static int sn_queued(SpSim* S) {
  if (!S->events.empty() || !S->probe_q.empty() || !S->inj.empty() || !S->inj_join.empty()) {
    seterr("kb_sim_snapshot: lifecycle calls, probes or injected records are queued for the next round start (step first)");
    return KB_INVALID_OPERATION;
  }
  return KB_OK;
}
// pass 1: the counters folded, the offsets of this leaf's rows, its entries counted
static int sn_measure(kb_sim*, uint64_t*, unsigned long long*) { return sn_dense(); }
static int sn_measure(SpSim* S, uint64_t* entries, unsigned long long* stats) {
  { const int rc = fold_stats(S); if (rc) return rc; }
  SnScratch x;
  { const int rc = sn_scratch(S, &x); if (rc) return rc; }
  CsTimer tm;
  if (!tm.start(S->st)) { seterr("snapshot: events"); return KB_IO_ERROR; }
  sn_scan(S, x);
  tm.stop(S->st);
  HIPCHK(hipGetLastError());
  unsigned long long total = 0, st[kb::NSTAT];
  HIPCHK(hipMemcpyAsync(&total, x.off + S->R, 8, hipMemcpyDeviceToHost, S->st));
  HIPCHK(hipMemcpyAsync(st, S->d.stats, sizeof st, hipMemcpyDeviceToHost, S->st));
  HIPCHK(hipStreamSynchronize(S->st));
  S->sn_ms = tm.ms(); S->sn_total = total;
  *entries += total;
  for (int k = 0; k < kb::NSTAT; ++k) stats[k] += st[k];
  return KB_OK;
}
// pass 2: this leaf's rows into the sections; the first leaf also writes what every shard holds alike
static int sn_gather(kb_sim*, uint8_t*, const SnSec*, uint64_t*, bool) { return sn_dense(); }
static int sn_gather(SpSim* S, uint8_t* buf, const SnSec* sec, uint64_t* ent_at, bool first) {
  const SpDev& d = S->d;
  const uint32_t C = S->C, R = S->R, lo = S->lo;
  SnScratch x;
  { const int rc = sn_scratch(S, &x); if (rc) return rc; }
  const uint64_t total = S->sn_total;
  { const int rc = sp_grow(S, &S->sn_buf, &S->sn_cap, (size_t)total); if (rc) return rc; }
  CsTimer tm;
  if (!tm.start(S->st)) { seterr("snapshot: events"); return KB_IO_ERROR; }
  kb::k_sn_fp<<<(R + 255) / 256, 256, 0, S->st>>>(d, x.fp);
  if (total) kb::k_sn_pack<<<sn_grid(total), 256, 0, S->st>>>(d, x.off, total, S->sn_buf);
  tm.stop(S->st);
  HIPCHK(hipGetLastError());
  const auto rows = [&](SnId k, const void* dev_local_base) {     // R rows of section k, from the shard's first row
    return hipMemcpyAsync(buf + sec[k].off + (uint64_t)lo * sec[k].elem, dev_local_base, (size_t)R * sec[k].elem, hipMemcpyDeviceToHost, S->st);
  };
  HIPCHK(rows(SN_NE, d.ne + lo)); HIPCHK(rows(SN_BASED, d.based + lo)); HIPCHK(rows(SN_N, d.n + lo));
  HIPCHK(rows(SN_FP, x.fp)); HIPCHK(rows(SN_LAST_BCAST, d.last_bcast + lo)); HIPCHK(rows(SN_A3CUR, d.a3cur + lo));
  HIPCHK(rows(SN_SUSP, d.susp + (size_t)lo * kb::SLOTS)); HIPCHK(rows(SN_CUR, d.cur + (size_t)lo * kb::CSLOTS));
  HIPCHK(rows(SN_PAQ, d.paq + (size_t)lo * kb::PAQ)); HIPCHK(rows(SN_PAQ_N, d.paq_n + lo));
  if (total) HIPCHK(hipMemcpyAsync(buf + sec[SN_ENTRIES].off + 4ull * *ent_at, S->sn_buf, 4ull * total, hipMemcpyDeviceToHost, S->st));
  if (first) {
    const auto ids = [&](SnId k, const void* dev) { return hipMemcpyAsync(buf + sec[k].off, dev, (size_t)C * sec[k].elem, hipMemcpyDeviceToHost, S->st); };
    HIPCHK(ids(SN_ALIVE, d.alive)); HIPCHK(ids(SN_START_ROUND, d.start_round)); HIPCHK(ids(SN_IDSET, d.idset)); HIPCHK(ids(SN_EXT, d.ext));
    if (S->nj) HIPCHK(hipMemcpyAsync(buf + sec[SN_BJOIN].off, S->bjoin, sizeof(kb::BCast) * S->nj, hipMemcpyDeviceToHost, S->st));
    if (S->nf) HIPCHK(hipMemcpyAsync(buf + sec[SN_BFAIL].off, S->bfail, sizeof(kb::BCast) * S->nf, hipMemcpyDeviceToHost, S->st));
    uint32_t ctr[kb::NCTR];
    HIPCHK(hipMemcpyAsync(ctr, d.ctr, sizeof ctr, hipMemcpyDeviceToHost, S->st));
    HIPCHK(hipStreamSynchronize(S->st));
    memcpy(buf + sec[SN_IDENT].off, S->h_ident.data(), (size_t)C * kb::MAXID);
    memcpy(buf + sec[SN_IDLEN].off, S->h_idlen.data(), C);
    memcpy(buf + sec[SN_PEND].off, S->h_pend.data(), (size_t)C * kb::MAXID);
    memcpy(buf + sec[SN_PENDLEN].off, S->h_pendlen.data(), 2ull * C);
    memcpy(buf + sec[SN_MOVED].off, S->h_moved.data(), C);
    SnScalars sc;
    memset(&sc, 0, sizeof sc);
    sc.round = S->round; sc.nj = S->nj; sc.nf = S->nf; sc.bj_total = S->bj_total; sc.bf_total = S->bf_total;
    sc.next_free = ctr[kb::C_NEXTFREE]; sc.first_conv = ctr[kb::C_FIRSTCONV]; sc.last_conv = ctr[kb::C_LASTCONV];
    sc.last_agree = ctr[kb::C_LASTAGREE]; sc.last_alive = ctr[kb::C_LASTALIVE];
    memcpy(buf + sec[SN_SCALARS].off, &sc, sizeof sc);
  } else {
    HIPCHK(hipStreamSynchronize(S->st));
  }
  S->sn_ms += tm.ms();
  *ent_at += total;
  return KB_OK;
}

extern "C" int kb_sim_snapshot(kb_sim* s, void* buf, size_t cap, uint64_t* bytes) {
  if (!s || !bytes) return KB_INVALID_ARGUMENT;
  const Kind kd = kind_of(s);
  if (kd.rank) {
    seterr("kb_sim_snapshot: a rank handle holds its own rows only (use kb_sim_create or kb_sim_create_local)");
    return KB_INVALID_OPERATION;
  }
  if (!kd.sparse) return sn_dense();
  { const int rc = route(s, R_ALL, 0, [&](auto* e) { return sn_queued(e); }); if (rc) return rc; }
  uint64_t entries = 0;
  unsigned long long stats[kb::NSTAT] = {0};
  uint32_t nj = 0, nf = 0;
  { const int rc = route(s, R_ALL, 0, [&](auto* e) { return sn_measure(e, &entries, stats); }); if (rc) return rc; }
  { const int rc = route(s, R_FIRST, 0, [&](auto* e) { nj = e->nj; nf = e->nf; return KB_OK; }); if (rc) return rc; }
  SnSec sec[SN_NSEC];
  uint64_t total = 0;
  sn_layout(s->C, nj, nf, entries, sec, &total);
  *bytes = total;
  double ms = 0;
  if (!buf || !cap) {
    route(s, R_ALL, 0, [&](auto* e) { ms += e->sn_ms; return KB_OK; });
    s->sn_ms = ms;
    return KB_OK;
  }
  if ((uint64_t)cap < total) { seterr("kb_sim_snapshot: the buffer is smaller than the snapshot"); return KB_CAPACITY; }
  uint8_t* b = static_cast<uint8_t*>(buf);
  memset(b, 0, sizeof(SnHdr) + sizeof(SnSec) * SN_NSEC);
  for (uint32_t k = 0; k < SN_NSEC; ++k) {            // the padding behind every section
    const uint64_t end = sec[k].off + (uint64_t)sec[k].elem * sec[k].count, next = k + 1 < SN_NSEC ? sec[k + 1].off : total;
    memset(b + end, 0, (size_t)(next - end));
  }
  uint64_t ent_at = 0;
  bool first = true;
  {
    const int rc = route(s, R_ALL, 0, [&](auto* e) { const int rc = sn_gather(e, b, sec, &ent_at, first); first = false; return rc; });
    if (rc) return rc;
  }
  route(s, R_ALL, 0, [&](auto* e) { ms += e->sn_ms; return KB_OK; });
  s->sn_ms = ms;
  memcpy(b + sec[SN_STATS].off, stats, sizeof stats);
  memcpy(b + sizeof(SnHdr), sec, sizeof sec);
  SnHdr h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, SN_MAGIC, sizeof SN_MAGIC);
  h.format_version = KB_SNAPSHOT_VERSION; h.abi_version = KB_ABI_VERSION;
  h.header_bytes = sizeof(SnHdr); h.cfg_bytes = sizeof(kb_config);
  route(s, R_FIRST, 0, [&](auto* e) { h.cfg = e->cfg; h.round = e->round; return KB_OK; });
  h.cfg.device = -1;                                 // where the mesh ran is no part of its state
  const uint8_t* al = b + sec[SN_ALIVE].off;
  for (uint32_t i = 0; i < s->C; ++i) h.alive += al[i] != 0;
  h.entries = entries; h.bytes = total; h.nsect = SN_NSEC;
  h.payload_crc32 = sn_crc(b + sizeof(SnHdr), (size_t)(total - sizeof(SnHdr)));
  memcpy(b, &h, sizeof h);
  return KB_OK;
}

// a created leaf takes the snapshot's state: its rows' slices, the per-id facts, the counters (shard 0: the mesh's)
static int sn_apply(kb_sim*, const void*, const SnHdr&, const SnSec*, const uint64_t*) { return sn_dense(); }
static int sn_apply(SpSim* S, const void* buf, const SnHdr& h, const SnSec* sec, const uint64_t* row_off) {
  (void)hipSetDevice(S->device);
  SpDev& d = S->d;
  const uint32_t C = S->C, R = S->R, lo = S->lo;
  const uint8_t* b = static_cast<const uint8_t*>(buf);
  const auto rows = [&](SnId k, void* dev_local_base) {
    return hipMemcpyAsync(dev_local_base, b + sec[k].off + (uint64_t)lo * sec[k].elem, (size_t)R * sec[k].elem, hipMemcpyHostToDevice, S->st);
  };
  const auto ids = [&](SnId k, void* dev) { return hipMemcpyAsync(dev, b + sec[k].off, (size_t)C * sec[k].elem, hipMemcpyHostToDevice, S->st); };
  HIPCHK(rows(SN_NE, d.ne + lo)); HIPCHK(rows(SN_BASED, d.based + lo)); HIPCHK(rows(SN_N, d.n + lo));
  HIPCHK(rows(SN_FP, d.fp + lo)); HIPCHK(rows(SN_LAST_BCAST, d.last_bcast + lo)); HIPCHK(rows(SN_A3CUR, d.a3cur + lo));
  HIPCHK(rows(SN_SUSP, d.susp + (size_t)lo * kb::SLOTS)); HIPCHK(rows(SN_CUR, d.cur + (size_t)lo * kb::CSLOTS));
  HIPCHK(rows(SN_PAQ, d.paq + (size_t)lo * kb::PAQ)); HIPCHK(rows(SN_PAQ_N, d.paq_n + lo));
  HIPCHK(hipMemsetAsync(d.dirty + lo, 0, R, S->st));   // the stored fingerprints are the rows' folds
  HIPCHK(ids(SN_ALIVE, d.alive)); HIPCHK(ids(SN_START_ROUND, d.start_round)); HIPCHK(ids(SN_IDSET, d.idset)); HIPCHK(ids(SN_EXT, d.ext));
  SnScalars sc;
  memcpy(&sc, b + sec[SN_SCALARS].off, sizeof sc);
  if (sc.nj) HIPCHK(hipMemcpyAsync(S->bjoin, b + sec[SN_BJOIN].off, sizeof(kb::BCast) * sc.nj, hipMemcpyHostToDevice, S->st));
  if (sc.nf) {
    HIPCHK(hipMemcpyAsync(S->bfail, b + sec[SN_BFAIL].off, sizeof(kb::BCast) * sc.nf, hipMemcpyHostToDevice, S->st));
    kb::k_sp_fkey<<<(sc.nf + 3 + 255) / 256, 256, 0, S->st>>>((const kb::BCast*)S->bfail, sc.nf, S->fkey);
  }
  uint32_t ctr[kb::NCTR];
  HIPCHK(hipMemcpyAsync(ctr, d.ctr, sizeof ctr, hipMemcpyDeviceToHost, S->st));
  HIPCHK(hipStreamSynchronize(S->st));
  ctr[kb::C_NEXTFREE] = sc.next_free; ctr[kb::C_FIRSTCONV] = sc.first_conv; ctr[kb::C_LASTCONV] = sc.last_conv;
  ctr[kb::C_LASTAGREE] = sc.last_agree; ctr[kb::C_LASTALIVE] = sc.last_alive;
  HIPCHK(hipMemcpyAsync(d.ctr, ctr, sizeof ctr, hipMemcpyHostToDevice, S->st));
  if (S->rank == 0) HIPCHK(hipMemcpyAsync(d.stats, b + sec[SN_STATS].off, 8ull * kb::NSTAT, hipMemcpyHostToDevice, S->st));
  S->nj = sc.nj; S->nf = sc.nf; S->bj_total = sc.bj_total; S->bf_total = sc.bf_total; S->round = sc.round;
  memcpy(S->h_ident.data(), b + sec[SN_IDENT].off, (size_t)C * kb::MAXID);
  memcpy(S->h_idlen.data(), b + sec[SN_IDLEN].off, C);
  memcpy(S->h_pend.data(), b + sec[SN_PEND].off, (size_t)C * kb::MAXID);
  memcpy(S->h_pendlen.data(), b + sec[SN_PENDLEN].off, 2ull * C);
  memcpy(S->h_moved.data(), b + sec[SN_MOVED].off, C);
  memcpy(S->h_idset.data(), b + sec[SN_IDSET].off, C);
  const uint8_t* ext = b + sec[SN_EXT].off;
  size_t n_ext = 0;
  for (uint32_t j = 0; j < C; ++j) n_ext += ext[j] != 0;
  if (n_ext) {
    S->h_ext.assign(ext, ext + C); S->n_ext = n_ext;
    HIPCHK(hipStreamSynchronize(S->st));
    { const int rc = export_alloc(S); if (rc) return rc; }
  }
  HIPCHK(hipStreamSynchronize(S->st));
  { const int rc = upload_segments(S); if (rc) return rc; }   // the segment CRCs and `uniform` of the stored identities
  // the rows' entries: this shard's run of the packed section, unpacked by the offsets of the lengths just uploaded
  const uint64_t total = row_off[S->hi] - row_off[lo];
  SnScratch x;
  { const int rc = sn_scratch(S, &x); if (rc) return rc; }
  { const int rc = sp_grow(S, &S->sn_buf, &S->sn_cap, (size_t)total); if (rc) return rc; }
  if (total) HIPCHK(hipMemcpyAsync(S->sn_buf, b + sec[SN_ENTRIES].off + 4ull * row_off[lo], 4ull * total, hipMemcpyHostToDevice, S->st));
  CsTimer tm;
  if (!tm.start(S->st)) { seterr("snapshot: events"); return KB_IO_ERROR; }
  sn_scan(S, x);
  if (total) kb::k_sn_unpack<<<sn_grid(total), 256, 0, S->st>>>(d, x.off, total, (const uint32_t*)S->sn_buf);
  tm.stop(S->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(S->st));
  S->sn_ms = tm.ms(); S->sn_total = total;
  (void)h;
  return KB_OK;
}

extern "C" int kb_sim_restore(const void* buf, size_t len, int32_t shards, int32_t device, kb_sim** out) {
  if (!out) return KB_INVALID_ARGUMENT;
  SnHdr h;
  SnSec sec[SN_NSEC];
  { const int rc = sn_parse(buf, len, &h, sec); if (rc) return rc; }
  { const int rc = sn_check_values(buf, h, sec); if (rc) return rc; }
  const uint32_t C = h.cfg.capacity, world = shards > 1 ? (uint32_t)shards : 1u;
  if (shards < 0 || shards > (int32_t)XMAX || (uint64_t)(world - 1) * ((C + world - 1) / world) >= C) {
    seterr("kb_sim_restore: the shard count is out of range or leaves a shard without rows (0..8 shards, each holding at least one row)");
    return KB_INVALID_ARGUMENT;
  }
  kb_config cfg = h.cfg;
  cfg.device = device;
  kb_sim* s = nullptr;
  { const int rc = world > 1 ? kb_sim_create_local(&cfg, (int32_t)world, &s) : kb_sim_create(&cfg, &s); if (rc) return rc; }
  std::vector<uint64_t> row_off((size_t)C + 1, 0);   // entries before global row i
  const uint32_t* ne = sn_at<uint32_t>(buf, sec, SN_NE);
  for (uint32_t i = 0; i < C; ++i) row_off[i + 1] = row_off[i] + ne[i];
  double ms = 0;
  const int rc = route(s, R_ALL, 0, [&](auto* e) { const int rc = sn_apply(e, buf, h, sec, row_off.data()); if (!rc) ms += e->sn_ms; return rc; });
  if (rc) { const std::string keep = g_err; (void)kb_sim_destroy(s); seterr(keep); return rc; }
  s->sn_ms = ms;
  *out = s;
  return KB_OK;
}

extern "C" int kb_sim_snapshot_device_ms(kb_sim* s, double* ms) {
  if (!s || !ms) return KB_INVALID_ARGUMENT;
  *ms = s->sn_ms;
  return KB_OK;
}
