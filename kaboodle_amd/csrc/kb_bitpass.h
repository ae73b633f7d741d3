// kb_bitpass.h — the device half of the censuses' frame (DESIGN.md "Host control plane"): what the passes over the
// member bits (Dev::bits, [rows][W/32]) share: the id masks, the shards' rows as one table, the bit-sliced column
// counters, a wave's row tile.  Included by kb_sim.hip after kb_censusframe.h, before the census headers.
#pragma once
#include "kb_scratch.h"

namespace kb {

// [NWR] each: the running ids, the stale class (neither running nor external; nullptr: not wanted), the valid ids (< C)
struct IdMasks { uint32_t* ab; uint32_t* sb; uint32_t* vb; };
// the running set as k_alive_bits builds it; ext == nullptr: no id is external
__global__ void k_id_masks(const uint8_t* alive, const uint8_t* ext, uint32_t C, uint32_t NWR, IdMasks m) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= NWR) return;
  uint32_t x = 0, s = 0, v = 0;
  for (uint32_t t = 0; t < 32; ++t) {
    const uint32_t j = w * 32 + t;
    if (j >= C) break;
    const bool al = alive[j] != 0, ex = ext && ext[j] != 0;       // both loads before either is used
    v |= 1u << t;
    if (al) x |= 1u << t;
    if (!al && !ex) s |= 1u << t;
  }
  m.ab[w] = x; m.vb[w] = v;
  if (m.sb) m.sb[w] = s;
}

struct BitRows {
  const uint32_t* bits[XMAX];                     // every shard's member bits (biased: indexed by global row)
  uint32_t lo[XMAX];                              // its first row; 0xFFFFFFFF for unused entries
  uint32_t C, NWR;                                // capacity, words per row
};
// row r: in the shard of the last entry whose first row is <= r (lo[] ascending, lo[0] = 0, unused 0xFFFFFFFF: bit_rows())
__device__ __attribute__((always_inline)) inline const uint32_t* bit_row(const BitRows& t, uint32_t r) {
  const uint32_t* p = t.bits[0];
#pragma unroll
  for (uint32_t k = 1; k < XMAX; ++k) if (r >= t.lo[k]) p = t.bits[k];
  return p + (size_t)r * t.NWR;
}

constexpr uint32_t BP_LOW = 5, BP_HIGH = 12;      // bit planes: 5 filled row by row, folded into 12 more
constexpr uint32_t BP_U = 8;                      // rows per batch (loads in flight per lane)
constexpr uint32_t BP_MAX_RPW = 4080;             // rows per wave (< 2^BP_HIGH; a multiple of BP_U and of CS_FOLD)

// the LDS slot of (word of the lane's group, bit, lane): consecutive lanes on consecutive banks, padded
__device__ __host__ constexpr uint32_t col_slot(uint32_t word, uint32_t bit, uint32_t lane) { return (word * 32 + bit) * 65 + lane; }
__device__ __host__ constexpr uint32_t col_lds(uint32_t nw) { return nw * 32 * 65; }   // a block's counters, NW words a lane

// the vertical counters of the NW words a lane owns (plane p: bit p of 32 counters), in registers: every loop unrolls
template <uint32_t NW> struct ColCount {
  uint32_t lo[NW][BP_LOW] = {}, hi[NW][BP_HIGH] = {};
  // x joins word q's counters: a ripple of half adders (no carry out while < 2^BP_LOW words were added since a fold)
  __device__ __attribute__((always_inline)) void add(uint32_t q, uint32_t x) {
#pragma unroll
    for (uint32_t k = 0; k < BP_LOW; ++k) { const uint32_t c = lo[q][k] & x; lo[q][k] ^= x; x = c; }
  }
  // the low planes' counters are added to the high planes' (full adders, then the carry's ripple) and cleared
  __device__ __attribute__((always_inline)) void fold() {
#pragma unroll
    for (uint32_t q = 0; q < NW; ++q) {
      uint32_t c = 0;
#pragma unroll
      for (uint32_t k = 0; k < BP_LOW; ++k) {
        const uint32_t s = hi[q][k] ^ lo[q][k];
        const uint32_t c2 = (hi[q][k] & lo[q][k]) | (s & c);
        hi[q][k] = s ^ c; c = c2; lo[q][k] = 0;
      }
#pragma unroll
      for (uint32_t k = BP_LOW; k < BP_HIGH; ++k) { const uint32_t c2 = hi[q][k] & c; hi[q][k] ^= c; c = c2; }
    }
  }
  // lane l's 32 NW counters out of the high planes, added to the block's LDS counters
  __device__ __attribute__((always_inline)) void readout(uint32_t* cnt, uint32_t l) const {
    for (uint32_t c = 0; c < 32; ++c) {
#pragma unroll
      for (uint32_t q = 0; q < NW; ++q) {
        uint32_t n = 0;
#pragma unroll
        for (uint32_t p = 0; p < BP_HIGH; ++p) n |= ((hi[q][p] >> c) & 1u) << p;
        if (n) atomicAdd(&cnt[col_slot(q, c, l)], n);
      }
    }
  }
};
// the inverse walk: a block's nonzero counters are added to its 64 x 32 NW columns of the [W] result (256 threads)
template <uint32_t NW> __device__ __attribute__((always_inline)) inline void col_flush(const uint32_t* cnt, uint32_t* out) {
  for (uint32_t k = threadIdx.x; k < 64 * 32 * NW; k += 256) {
    const uint32_t n = cnt[col_slot((k >> 5) % NW, k & 31u, k / (32 * NW))];   // column k: lane k / (32 NW), word, bit
    if (n) atomicAdd(&out[k], n);
  }
}

// rows [r0, r1) of [lo, hi): the tile of wave wv (0..3) of the workgroup at row-tile index `tile`, rpw rows a wave
__device__ __attribute__((always_inline)) inline void wave_rows(uint32_t lo, uint32_t hi, uint32_t tile, uint32_t wv, uint32_t rpw,
                                                                uint32_t& r0, uint32_t& r1) {
  const uint64_t first = (uint64_t)lo + (uint64_t)(tile * 4 + wv) * rpw;
  r0 = first < hi ? (uint32_t)first : hi;
  r1 = hi - r0 > rpw ? r0 + rpw : hi;
}

}  // namespace kb

// ---- host side -------------------------------------------------------------------------------------------
// the masks' place in a scratch layout: 16-byte aligned, for the passes' uint4 loads of them
static kb::IdMasks carve_masks(Carve& c, uint32_t NWR, bool stale) {
  uint32_t* ab = c.take<uint32_t>(NWR, 16); uint32_t* vb = c.take<uint32_t>(NWR, 16);
  return kb::IdMasks{ab, stale ? c.take<uint32_t>(NWR, 16) : nullptr, vb};
}
static void id_masks(const uint8_t* alive, const uint8_t* ext, uint32_t C, uint32_t NWR, const kb::IdMasks& m, hipStream_t st) {
  kb::k_id_masks<<<(NWR + 255) / 256, 256, 0, st>>>(alive, ext, C, NWR, m);
}

// one table of C rows, NWR words each
static void bit_rows(const uint32_t* bits, uint32_t C, uint32_t NWR, kb::BitRows& t) {
  for (uint32_t k = 0; k < kb::XMAX; ++k) { t.bits[k] = bits; t.lo[k] = 0xFFFFFFFFu; }
  t.lo[0] = 0; t.C = C; t.NWR = NWR;
}
// The table of a handle or an in-process group, for the census `who`.  *owner owns the scratch and the stream (every
// shard is on its device, made current); the shards' streams are synchronised and bit_row's precondition is checked.
static int bit_rows(kb_sim* s, const char* who, kb::BitRows& t, kb_sim** owner) {
  kb_sim* h = *owner = is_group(s) ? s->shards[0] : s;
  (void)hipSetDevice(h->device);
  bit_rows(h->d.bits, s->C, h->d.NWR, t);
  if (!is_group(s)) return KB_OK;
  { const int rc = route(s, R_ALL, 0, [](auto* e) -> int { HIPCHK(hipStreamSynchronize(eng_stream(e))); return KB_OK; }); if (rc) return rc; }
  const size_t ns = s->shards.size();
  bool ok = ns >= 1 && ns <= kb::XMAX && s->shards[0]->lo == 0 && s->shards[ns - 1]->hi == s->C;
  for (size_t k = 0; ok && k < ns; ++k) {
    t.bits[k] = s->shards[k]->d.bits; t.lo[k] = s->shards[k]->lo;
    ok = k == 0 || (t.lo[k] == s->shards[k - 1]->hi && t.lo[k] > t.lo[k - 1]);
  }
  if (!ok) { seterr(std::string(who) + ": the group's shards are not contiguous in row order"); return KB_INVALID_OPERATION; }
  return KB_OK;
}
