// kb_recip.h — the reciprocity census (include/kaboodle_reciprocity.h): for every running row the
// number of running peers it lacks that lack it too (mutual), that still hold it (lacks), and that it holds while
// they lack it (lacked_by).  Included at the end of kb_sim.hip; reads the dense engine's member bits, writes only
// its own scratch.
//
// The question is about the member-bit matrix B ([rows][W/32], Dev::bits) and its transpose.  The matrix is cut
// into square blocks of 512 x 512 bits.  A workgroup takes one unordered pair of blocks (I <= J): it stages
// block (I, J) and its mirror (J, I) in LDS (every row segment read from HBM is 64 contiguous bytes), so each
// block is read once and the pass moves R·W/8 bytes.  Wave w owns the 64 rows of tile w of block I and walks the
// 8 column tiles: a lane holds one 64-bit row word x of the block and one row word y of the mirror, the mirror's
// 64 x 64 tile is transposed inside the wave (six exchange stages), and
//     ~x & ~yT   mutual gaps      ~x & yT   i lacks j, j holds i      x & ~yT   i holds j, j lacks i
// are counted per row under the running masks of the rows and the columns.  The mirror's rows get their counts
// from the same two words with the block's tile transposed instead (lacks and lacked_by swap).  A tile pair
// whose running rows hold every running column in both directions has nothing to count and skips both
// transposes: that is almost every tile of a mesh near agreement.  Counts go to zeroed [C] arrays by integer
// atomics: order-free, so the result is deterministic.  Rows that are not running are never read (their LDS
// image is zero and their mask bit is clear), so a stopped id's stale row counts neither as a row nor as a column.
//
// The pair list is a second launch over the block pairs the first pass flagged as holding a mutual gap; it
// appends (i, j), i < j, to a buffer sized for the known total, and the host sorts it.
#pragma once
#include "../../include/kaboodle_reciprocity.h"

namespace kb {

constexpr uint32_t RC_B = 512;                    // ids per block side
constexpr uint32_t RC_T = RC_B / 64;              // 64-id tiles per block side = waves per workgroup
constexpr uint32_t RC_LD = RC_T + 1;              // u64 per staged row: 72-byte rows, so the 32 lanes of a
                                                  // ds_read_b64 half fall on 32 distinct bank pairs
constexpr uint32_t RC_THREADS = 64 * RC_T;

struct RcArgs {
  BitRows rows;                                   // the member bits of rows.C ids (kb_bitpass.h)
  uint32_t nb;                                    // blocks per side
  const uint32_t* ab;                             // [W/32] running ids (k_id_masks)
  uint32_t* cnt;                                  // [3][C] mutual, lacks, lacked_by (zeroed)
  uint32_t* flag;                                 // [nb][nb] block pair (I, J) holds a mutual gap (zeroed)
  uint2* pairs; unsigned long long* npairs;       // the pair pass: its buffer, entries appended (zeroed)
  unsigned long long cap;                         // entries the buffer holds
};

// the running rows' 64-byte segments of rows [rb*512, +512) x columns [cb*512, +512): a thread's four loads
__device__ __attribute__((always_inline)) inline void rc_load(const RcArgs& a, uint32_t rb, uint32_t cb, uint4 (&v)[4]) {
#pragma unroll
  for (uint32_t p = 0; p < 4; ++p) {
    const uint32_t row = rb * RC_B + p * 128 + (threadIdx.x >> 2);
    const bool on = row < a.rows.C && ((a.ab[row >> 5] >> (row & 31u)) & 1u);
    v[p] = on ? *reinterpret_cast<const uint4*>(bit_row(a.rows, row) + cb * (RC_B / 32) + (threadIdx.x & 3u) * 4)
              : uint4{0, 0, 0, 0};
  }
}
__device__ __attribute__((always_inline)) inline void rc_store(uint64_t* dst, const uint4 (&v)[4]) {
#pragma unroll
  for (uint32_t p = 0; p < 4; ++p) {
    uint64_t* q = dst + (p * 128 + (threadIdx.x >> 2)) * RC_LD + (threadIdx.x & 3u) * 2;
    q[0] = (uint64_t)v[p].x | ((uint64_t)v[p].y << 32);
    q[1] = (uint64_t)v[p].z | ((uint64_t)v[p].w << 32);
  }
}

// One stage of the in-wave transpose of a 64 x 64 bit tile (lane = row, bit = column): the off-diagonal S x S
// sub-blocks of every 2S x 2S block change places, element (r, c) with (r, c) ^ (S, S).
template <uint32_t S> __device__ __attribute__((always_inline)) inline uint64_t rc_tstage(uint64_t x, uint32_t l) {
  constexpr uint64_t M = S == 1 ? 0x5555555555555555ull : S == 2 ? 0x3333333333333333ull
                       : S == 4 ? 0x0F0F0F0F0F0F0F0Full : S == 8 ? 0x00FF00FF00FF00FFull : 0x0000FFFF0000FFFFull;
  const uint32_t ylo = shfl_xor_c<S>((uint32_t)x), yhi = shfl_xor_c<S>((uint32_t)(x >> 32));
  const uint64_t y = ((uint64_t)yhi << 32) | ylo;
  return (l & S) ? (x & ~M) | ((y & ~M) >> S) : (x & M) | ((y & M) << S);
}
// lane l ends with bit c = bit l of lane c's x
__device__ __attribute__((always_inline)) inline uint64_t rc_transpose(uint64_t x, uint32_t l) {
  {                                               // S = 32: whole halves change places, one exchange
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    const uint32_t got = shfl_xor_c<32>((l & 32u) ? lo : hi);
    x = (l & 32u) ? ((uint64_t)hi << 32) | got : ((uint64_t)got << 32) | lo;
  }
  x = rc_tstage<16>(x, l); x = rc_tstage<8>(x, l); x = rc_tstage<4>(x, l);
  x = rc_tstage<2>(x, l); x = rc_tstage<1>(x, l);
  return x;
}

// grid (nb, nb): block pair (I, J) = (blockIdx.x, blockIdx.y), I <= J; 512 threads = 8 waves, wave w = row tile w
__global__ __launch_bounds__(RC_THREADS) void k_rc_count(RcArgs a) {
  const uint32_t BI = blockIdx.x, BJ = blockIdx.y;
  if (BI > BJ) return;
  __shared__ uint64_t sA[RC_B * RC_LD], sB[RC_B * RC_LD];
  __shared__ uint32_t cj[3 * RC_B];               // the mirror's rows: their counts from all 8 waves
  const bool diag = BI == BJ;
  {
    uint4 va[4], vb[4];
    rc_load(a, BI, BJ, va);
    if (!diag) rc_load(a, BJ, BI, vb);            // every load before the first LDS write
    rc_store(sA, va);
    if (!diag) rc_store(sB, vb);
  }
  for (uint32_t k = threadIdx.x; k < 3 * RC_B; k += RC_THREADS) cj[k] = 0;
  __syncthreads();
  const uint64_t* sM = diag ? sA : sB;            // the mirror block
  const uint32_t l = lane();
  const uint32_t ti = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t* ab64 = reinterpret_cast<const uint64_t*>(a.ab);
  const uint64_t runI = ab64[BI * RC_T + ti];     // this tile's running rows (wave-uniform)
  const bool rowI = (runI >> l) & 1ull;
  uint32_t nm = 0, nl = 0, nh = 0;
  bool any = false;
  if (runI) {
    for (uint32_t tj = 0; tj < RC_T; ++tj) {
      const uint64_t runJ = ab64[BJ * RC_T + tj];
      if (!runJ) continue;
      const bool rowJ = (runJ >> l) & 1ull;
      const uint64_t x = sA[(ti * 64 + l) * RC_LD + tj];        // row i = tile ti's l-th, columns of tile tj
      const uint64_t y = sM[(tj * 64 + l) * RC_LD + ti];        // row j = tile tj's l-th, columns of tile ti
      // nothing lacked in either direction (the diagonal bit aside: a view holds its own id): nothing to count
      if (!__ballot((rowI && (~x & runJ)) || (rowJ && (~y & runI)))) continue;
      const uint64_t yt = rc_transpose(y, l);                   // bit c: j = tile tj's c-th holds i
      uint64_t cm = runJ;
      if (diag && ti == tj) cm &= ~(1ull << l);                 // i != j
      if (!rowI) cm = 0;
      const uint64_t gm = ~x & ~yt & cm;
      nm += (uint32_t)__popcll(gm); nl += (uint32_t)__popcll(~x & yt & cm); nh += (uint32_t)__popcll(x & ~yt & cm);
      any |= gm != 0;
      if (!diag) {                                              // the same pairs seen from the mirror's rows
        const uint64_t xt = rc_transpose(x, l);                 // bit c: i = tile ti's c-th holds j
        const uint64_t rm = rowJ ? runI : 0ull;
        const uint32_t jm = (uint32_t)__popcll(~y & ~xt & rm), jl = (uint32_t)__popcll(~y & xt & rm),
                       jb = (uint32_t)__popcll(y & ~xt & rm);
        if (jm) atomicAdd(&cj[tj * 64 + l], jm);
        if (jl) atomicAdd(&cj[RC_B + tj * 64 + l], jl);
        if (jb) atomicAdd(&cj[2 * RC_B + tj * 64 + l], jb);
      }
    }
  }
  const uint32_t i = BI * RC_B + ti * 64 + l;
  if (i < a.rows.C) {
    if (nm) atomicAdd(&a.cnt[i], nm);
    if (nl) atomicAdd(&a.cnt[(size_t)a.rows.C + i], nl);
    if (nh) atomicAdd(&a.cnt[2 * (size_t)a.rows.C + i], nh);
  }
  if (__ballot(any) && l == 0) a.flag[(size_t)BI * a.nb + BJ] = 1;
  if (diag) return;                               // workgroup-uniform
  __syncthreads();
  const uint32_t j = BJ * RC_B + threadIdx.x;
  if (j < a.rows.C) {
#pragma unroll
    for (uint32_t q = 0; q < 3; ++q) {
      const uint32_t n = cj[q * RC_B + threadIdx.x];
      if (n) atomicAdd(&a.cnt[q * (size_t)a.rows.C + j], n);
    }
  }
}

// the mutual pairs (i, j), i < j, of the flagged block pairs, appended in no particular order (the host sorts)
__global__ __launch_bounds__(RC_THREADS) void k_rc_pairs(RcArgs a) {
  const uint32_t BI = blockIdx.x, BJ = blockIdx.y;
  if (BI > BJ || !a.flag[(size_t)BI * a.nb + BJ]) return;
  __shared__ uint64_t sA[RC_B * RC_LD], sB[RC_B * RC_LD];
  const bool diag = BI == BJ;
  {
    uint4 va[4], vb[4];
    rc_load(a, BI, BJ, va);
    if (!diag) rc_load(a, BJ, BI, vb);
    rc_store(sA, va);
    if (!diag) rc_store(sB, vb);
  }
  __syncthreads();
  const uint64_t* sM = diag ? sA : sB;
  const uint32_t l = lane();
  const uint32_t ti = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t* ab64 = reinterpret_cast<const uint64_t*>(a.ab);
  const uint64_t runI = ab64[BI * RC_T + ti];
  if (!runI) return;
  const bool rowI = (runI >> l) & 1ull;
  for (uint32_t tj = diag ? ti : 0; tj < RC_T; ++tj) {          // a diagonal block: the tiles on and above its diagonal
    const uint64_t runJ = ab64[BJ * RC_T + tj];
    if (!runJ) continue;
    const uint64_t x = sA[(ti * 64 + l) * RC_LD + tj];
    const uint64_t y = sM[(tj * 64 + l) * RC_LD + ti];
    if (!__ballot((rowI && (~x & runJ)) || (((runJ >> l) & 1ull) && (~y & runI)))) continue;
    const uint64_t yt = rc_transpose(y, l);
    uint64_t cm = rowI ? runJ : 0ull;
    if (diag && ti == tj) cm &= ~((2ull << l) - 1ull);          // j > i
    uint64_t gm = ~x & ~yt & cm;
    if (gm) {                                                   // lanes diverge here only: the exchanges are behind us
      unsigned long long at = atomicAdd(a.npairs, (unsigned long long)__popcll(gm));
      const uint32_t i = BI * RC_B + ti * 64 + l;
      for (; gm; gm &= gm - 1, ++at)
        if (at < a.cap) a.pairs[at] = make_uint2(i, BJ * RC_B + tj * 64 + (uint32_t)__builtin_ctzll(gm));
    }
  }
}

}  // namespace kb

// ---- host side -------------------------------------------------------------------------------------------
extern "C" int kb_sim_reciprocity(kb_sim* s, kb_reciprocity* out, uint32_t* mutual, uint32_t* lacks, uint32_t* lacked_by,
                                  size_t cap_rows, uint32_t* pairs, size_t cap_pairs) {
  if (!s || !out) return KB_INVALID_ARGUMENT;
  { const int rc = census_gate(s, "kb_sim_reciprocity", {"; the census needs every rank's", "need an O(entries) algorithm of their own (not built yet)", nullptr});
    if (rc) return rc; }
  { const int rc = census_caps("kb_sim_reciprocity", out, nullptr, 0, 0, any_of(mutual, lacks, lacked_by), cap_rows, s->C); if (rc) return rc; }
  RcArgs a{};
  kb_sim* h = nullptr;
  { const int rc = bit_rows(s, "kb_sim_reciprocity", a.rows, &h); if (rc) return rc; }
  const Dev& d = h->d;
  const uint32_t C = s->C, nb = (C + RC_B - 1) / RC_B;
  a.nb = nb;
  IdMasks m{};
  auto lay = [&](Carve& c) {                      // the masks (8-byte loads of ab), then, cleared every call, the pair
    m = carve_masks(c, d.NWR, false);             // counter, the counts and the flags
    c.zero_from(); a.npairs = c.take<unsigned long long>(1); a.cnt = c.take<uint32_t>(3ull * C); a.flag = c.take<uint32_t>((size_t)nb * nb); c.zero_to();
  };
  if (!h->rc_buf) HIPCHK(talloc(h, &h->rc_buf, carve_bytes(lay) / 4));
  const Carve c = carve(h->rc_buf, lay);
  a.ab = m.ab;
  CsTimer tm;
  if (!tm.start(h->st)) { seterr("reciprocity: events"); return KB_IO_ERROR; }
  HIPCHK(hipMemsetAsync(c.zero_ptr(), 0, c.zero_bytes(), h->st));
  id_masks(d.alive, nullptr, C, d.NWR, m, h->st);
  k_rc_count<<<dim3(nb, nb), RC_THREADS, 0, h->st>>>(a);
  tm.stop(h->st);
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> cnt;
  std::vector<uint8_t> alive;
  HIPCHK(fetch(cnt, a.cnt, 3ull * C, h->st));
  HIPCHK(fetch(alive, d.alive, C, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  s->census_ms[CM_RECIP] = tm.ms();
  memset(out, 0, sizeof *out);
  out->round = h->round;
  out->max_mutual_row = KB_CENSUS_NONE;
  uint64_t msum = 0;
  for (uint32_t i = 0; i < C; ++i) {
    const uint32_t mu = cnt[i], lk = cnt[(size_t)C + i];
    out->observers += alive[i] != 0;
    msum += mu; out->oneway_pairs += lk;
    out->rows_mutual += mu > 0; out->rows_oneway += lk > 0;
    if (mu > out->max_mutual) { out->max_mutual = mu; out->max_mutual_row = i; }
  }
  out->mutual_pairs = msum / 2;
  deliver(mutual, cnt.data(), C);
  deliver(lacks, cnt.data() + C, C);
  deliver(lacked_by, cnt.data() + 2ull * C, C);
  if (!pairs || !out->mutual_pairs || out->mutual_pairs > cap_pairs) return KB_OK;
  // the pair list: a device buffer and a host vector for exactly the known total (8 bytes each per pair), grown when
  // a later call needs more; the total is at most cap_pairs, so the caller's own 8 * cap_pairs buffer bounds both
  const uint64_t np = out->mutual_pairs;
  { const int rc = eng_grow(h, &h->rc_pairs, &h->rc_pairs_cap, (size_t)np); if (rc) return rc; }
  a.pairs = h->rc_pairs; a.cap = np;
  CsTimer tp;
  if (!tp.start(h->st)) { seterr("reciprocity: events"); return KB_IO_ERROR; }
  k_rc_pairs<<<dim3(nb, nb), RC_THREADS, 0, h->st>>>(a);
  tp.stop(h->st);
  HIPCHK(hipGetLastError());
  std::vector<uint64_t> pl;
  unsigned long long got = 0;
  HIPCHK(hipMemcpyAsync(&got, a.npairs, 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(fetch(pl, a.pairs, np, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  s->census_ms[CM_RECIP] += tp.ms();
  if (got != np) { seterr("reciprocity: the pair pass and the counts disagree"); return KB_IO_ERROR; }
  for (uint64_t& v : pl) v = (v << 32) | (v >> 32);              // uint2 (i, j) in memory = j << 32 | i: sort by (i, j)
  std::sort(pl.begin(), pl.end());
  for (uint64_t k = 0; k < np; ++k) { pairs[2 * k] = (uint32_t)(pl[k] >> 32); pairs[2 * k + 1] = (uint32_t)pl[k]; }
  out->pairs_listed = np;
  return KB_OK;
}

extern "C" int kb_sim_reciprocity_device_ms(kb_sim* s, double* ms) { return census_ms_get(s, CM_RECIP, ms); }
