// kb_delta.h — the view-delta census (include/kaboodle_delta.h): what every view gained and lost
// since a mark.  Included at the end of kb_sim.hip beside the other censuses; stands on the frame of
// kb_censusframe.h and kb_bitpass.h (the id masks, the column counters, the row tiles and their plan).
//
// A baseline is a copy of the member bits of a handle's rows ([rows][W/32]) and of the running set, taken by
// kb_sim_delta_mark.  The census is ONE streaming pass over the current bits and the baseline, shaped like
// k_cs_dense: the grid is column blocks x row tiles, a lane owns one 8-byte column group (2 words = 64 ids) and
// walks down its tile, so each row read is 512 B contiguous per wave and table; every load of a batch of 8 rows is
// issued before the first use.  Whether a row is continuing (running at the mark and now) is a scalar decision, and
// only continuing rows are read.  g = now & ~base & valid and l = base & ~now & valid go into two sets of bit-sliced
// vertical counters (5 low planes, folded into 12 high planes before they can overflow).  A row whose g | l is zero
// in every lane of the wave skips the adds, the popcounts and the row's reduction: a delta between consecutive
// rounds touches a few columns of a block only.  A workgroup's 4 waves combine their counters in LDS and add the
// nonzero ones to the [W] results with integer atomics: order-free, so the result is deterministic.  Under
// KB_DELTA_ADVANCE the same pass stores the column groups that differ into the baseline and copies the rows that
// began to run; the running-set copy is refreshed after the pass.
//
// The kernel takes DlArgs and does not reach into Dev, so kb_delta_of runs it on host arrays.
#pragma once
#include "../../include/kaboodle_delta.h"

namespace kb {

constexpr uint32_t DL_COLS = 4096;                // ids per column block: 64 lanes x 64
constexpr uint32_t DL_LOW_MAX = (1u << BP_LOW) - 1;   // rows the low planes hold between folds

struct DlArgs {
  const uint32_t* now;                            // [R][NWR] the rows' member bits (row 0 is id lo)
  uint32_t* base;                                 // [R][NWR] the baseline; written under advance only
  const uint8_t* run_now;                         // [C] running now, per id
  const uint8_t* run_base;                        // [C] running at the mark, per id
  IdMasks m;                                      // k_id_masks over run_now: ab and vb
  uint32_t* gby; uint32_t* lby;                   // [W] gained_by, lost_by (zeroed)
  uint32_t* rowc;                                 // [3][R] gained, lost, lost_live (zeroed)
  uint32_t C, NWR, lo, R;
  uint32_t rpw;                                   // rows per wave: a multiple of BP_U, <= BP_MAX_RPW
  uint32_t advance;                               // baseline := now in the same pass
};

// grid (W / 4096 column blocks, row tiles of 4 x rpw rows), 256 threads
__global__ __launch_bounds__(256) void k_delta(DlArgs a) {
  __shared__ uint32_t cnt[2][col_lds(2)];
  for (uint32_t k = threadIdx.x; k < 2 * col_lds(2); k += 256) (&cnt[0][0])[k] = 0;
  __syncthreads();
  const uint32_t l = lane();
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t nw2 = a.NWR / 2;
  const uint32_t cg = blockIdx.x * 64 + l;                       // this lane's column group (< nw2: the grid is exact)
  const uint2 ab = reinterpret_cast<const uint2*>(a.m.ab)[cg];
  const uint2 vb = reinterpret_cast<const uint2*>(a.m.vb)[cg];
  uint32_t r0, r1;                                               // local rows [r0, r1) of [0, R)
  wave_rows(0, a.R, blockIdx.y, wv, a.rpw, r0, r1);
  const uint2* now = reinterpret_cast<const uint2*>(a.now);
  uint2* base = reinterpret_cast<uint2*>(a.base);
  ColCount<2> gain, loss;                                        // the columns' gained_by and lost_by
  uint32_t nlow = 0;                                             // rows in the low planes: wave-uniform
  for (uint32_t r = r0; r < r1; r += BP_U) {
    uint32_t cm = 0, nm = 0;                                     // the batch's continuing rows, new rows: scalar masks
#pragma unroll
    for (uint32_t u = 0; u < BP_U; ++u) {
      if (r + u >= r1) continue;
      const bool rn = a.run_now[a.lo + r + u] != 0, rb = a.run_base[a.lo + r + u] != 0;
      if (rn && rb) cm |= 1u << u;
      if (rn && !rb) nm |= 1u << u;
    }
    cm = (uint32_t)__builtin_amdgcn_readfirstlane((int)cm);
    nm = (uint32_t)__builtin_amdgcn_readfirstlane((int)nm);
    if (a.advance && nm) {                                       // a row that began to run: its bits become its baseline
#pragma unroll
      for (uint32_t u = 0; u < BP_U; ++u)
        if ((nm >> u) & 1u) base[(size_t)(r + u) * nw2 + cg] = now[(size_t)(r + u) * nw2 + cg];
    }
    if (!cm) continue;                                           // no continuing row: nothing is read
    uint2 vn[BP_U], vo[BP_U];
#pragma unroll
    for (uint32_t u = 0; u < BP_U; ++u) {                        // every load of the batch before its first use
      vn[u] = vo[u] = make_uint2(0u, 0u);
      if ((cm >> u) & 1u) {                                      // a scalar branch: other rows are not read
        vn[u] = now[(size_t)(r + u) * nw2 + cg];
        vo[u] = base[(size_t)(r + u) * nw2 + cg];
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < BP_U; ++u) {
      if (!((cm >> u) & 1u)) continue;
      const uint32_t d0 = vn[u].x ^ vo[u].x, d1 = vn[u].y ^ vo[u].y;
      if (a.advance && (d0 | d1)) base[(size_t)(r + u) * nw2 + cg] = vn[u];   // only the groups that differ
      const uint32_t g0 = d0 & vn[u].x & vb.x, g1 = d1 & vn[u].y & vb.y;
      const uint32_t l0 = d0 & vo[u].x & vb.x, l1 = d1 & vo[u].y & vb.y;
      if (__ballot((g0 | g1 | l0 | l1) != 0u) == 0ull) continue;  // wave-uniform: the row changed nothing in this block
      gain.add(0, g0); gain.add(1, g1); loss.add(0, l0); loss.add(1, l1);
      const uint32_t ng = __popc(g0) + __popc(g1), nl = __popc(l0) + __popc(l1);
      const uint32_t nv = __popc(l0 & ab.x) + __popc(l1 & ab.y);
      const uint32_t t0 = wave_sum(ng | (nl << 16));             // <= 4096 each per wave: 16 bits hold them
      const uint32_t t1 = wave_sum(nv);
      if (l == 0) {
        const size_t k = r + u;
        if (t0 & 0xFFFFu) atomicAdd(&a.rowc[k], t0 & 0xFFFFu);
        if (t0 >> 16) atomicAdd(&a.rowc[(size_t)a.R + k], t0 >> 16);
        if (t1) atomicAdd(&a.rowc[2 * (size_t)a.R + k], t1);
      }
      if (++nlow == DL_LOW_MAX) { gain.fold(); loss.fold(); nlow = 0; }
    }
  }
  gain.fold(); loss.fold();
  gain.readout(cnt[0], l);
  loss.readout(cnt[1], l);
  __syncthreads();
  col_flush<2>(cnt[0], a.gby + (size_t)blockIdx.x * DL_COLS);
  col_flush<2>(cnt[1], a.lby + (size_t)blockIdx.x * DL_COLS);
}

}  // namespace kb

// ---- host side -------------------------------------------------------------------------------------------
// what the parts of a delta census add up to: the per-id counts over all ids, the rows' counts at the rows' ids
struct DlPart {
  std::vector<uint32_t> gby, lby, gained, lost, live;   // [C] each (rows no part held: 0)
  std::vector<uint8_t> alive, ext;                      // [C] the running and external sets now (replicated facts)
  uint32_t continuing = 0, new_rows = 0, ended_rows = 0;
  double ms = 0;
};
static void dl_part_init(DlPart& p, size_t C) {
  p.gby.assign(C, 0); p.lby.assign(C, 0); p.gained.assign(C, 0); p.lost.assign(C, 0); p.live.assign(C, 0);
}
// the pass's scratch (a.R, a.NWR set): the results, cleared before every pass, then the masks; the rows per wave
static void dl_lay(Carve& c, kb::DlArgs& a, uint32_t W, uint32_t ncu, uint64_t want_rpw) {
  c.zero_from(); a.gby = c.take<uint32_t>(W); a.lby = c.take<uint32_t>(W); a.rowc = c.take<uint32_t>(3ull * a.R); c.zero_to();
  a.m = carve_masks(c, a.NWR, false);
  a.rpw = rows_per_wave(a.R, W / kb::DL_COLS, ncu, want_rpw, kb::BP_U, kb::BP_MAX_RPW);
}

// The pass over a.now / a.base with the running sets a.run_now / a.run_base, scratch laid out in `c` by dl_lay, on
// stream st; its results join `p`, the rows' at index a.lo onwards.
static int dl_exec(const Carve& c, const kb::DlArgs& a, uint32_t W, hipStream_t st, DlPart& p) {
  const uint32_t C = a.C, R = a.R;
  CsTimer tm;
  if (!tm.start(st)) { seterr("delta census: events"); return KB_IO_ERROR; }
  HIPCHK(hipMemsetAsync(c.zero_ptr(), 0, c.zero_bytes(), st));
  id_masks(a.run_now, nullptr, C, a.NWR, a.m, st);
  if (R) k_delta<<<dim3(W / kb::DL_COLS, row_tiles(R, a.rpw)), 256, 0, st>>>(a);
  tm.stop(st);
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> gby(C), lby(C), rc(3ull * R);            // sized before the first copy waits for the kernels
  std::vector<uint8_t> rb;
  p.alive.resize(C);
  HIPCHK(fetch(gby, a.gby, C, st));
  HIPCHK(fetch(lby, a.lby, C, st));
  HIPCHK(fetch(rc, a.rowc, 3ull * R, st));
  HIPCHK(fetch(p.alive, a.run_now, C, st));
  HIPCHK(fetch(rb, a.run_base, C, st));
  HIPCHK(hipStreamSynchronize(st));
  p.ms += tm.ms();
  for (uint32_t j = 0; j < C; ++j) { p.gby[j] += gby[j]; p.lby[j] += lby[j]; }
  for (uint32_t k = 0; k < R; ++k) {
    const uint32_t i = a.lo + k;
    const bool rn = p.alive[i] != 0, was = rb[i] != 0;
    p.continuing += rn && was; p.new_rows += rn && !was; p.ended_rows += !rn && was;
    p.gained[i] = rc[k]; p.lost[i] = rc[(size_t)R + k]; p.live[i] = rc[2ull * R + k];
  }
  return KB_OK;
}

// the O(ids) reductions of the summary, on the host
static void dl_summary(const DlPart& p, int32_t round_base, int32_t round, kb_delta* out) {
  memset(out, 0, sizeof *out);
  out->round_base = round_base; out->round = round;
  out->continuing = p.continuing; out->new_rows = p.new_rows; out->ended_rows = p.ended_rows;
  out->top_false_drop = KB_CENSUS_NONE;
  for (size_t j = 0; j < p.gby.size(); ++j) {
    const uint32_t g = p.gby[j], l = p.lby[j];
    out->changed_rows += p.gained[j] + p.lost[j] > 0;
    out->changed_ids += g + l > 0;
    if (p.alive[j]) {
      out->learned += g; out->false_drops += l;
      if (l > out->top_false_drop_by) { out->top_false_drop = (uint32_t)j; out->top_false_drop_by = l; }
    } else if (p.ext[j]) { out->ext_gained += g; out->ext_lost += l; }
    else { out->ghost_adds += g; out->detections += l; }
  }
}
static void dl_deliver(const DlPart& p, uint32_t* gained_by, uint32_t* lost_by, uint32_t* gained, uint32_t* lost, uint32_t* lost_live) {
  deliver(gained_by, p.gby); deliver(lost_by, p.lby); deliver(gained, p.gained); deliver(lost, p.lost); deliver(lost_live, p.live);
}

// ---- the baseline of one leaf (route() hands every shard of a group here in turn) -----------------------------
static void dl_drop(kb_sim* s) {
  (void)hipSetDevice(s->device);
  for (void* p : {(void*)s->dl_base, (void*)s->dl_run}) {
    if (!p) continue;
    (void)hipFree(p);
    s->allocs.erase(std::remove(s->allocs.begin(), s->allocs.end(), p), s->allocs.end());
  }
  s->dl_base = nullptr; s->dl_run = nullptr;
}
static void dl_drop(SpSim*) {}
static int dl_mark(kb_sim* s) {
  (void)hipSetDevice(s->device);
  const size_t bytes = 4ull * s->R * s->d.NWR;                   // rows x W/8
  if (!s->dl_base) {
    void* b = nullptr; void* r = nullptr;
    if (hipMalloc(&b, bytes ? bytes : 4) != hipSuccess || hipMalloc(&r, s->C) != hipSuccess) {
      if (b) (void)hipFree(b);
      (void)hipGetLastError();
      seterr("kb_sim_delta_mark: the device cannot hold a baseline of " + std::to_string(bytes) + " bytes (rows x W/8)");
      return KB_CAPACITY;
    }
    s->dl_base = static_cast<uint32_t*>(b); s->dl_run = static_cast<uint8_t*>(r);
    s->allocs.push_back(b); s->allocs.push_back(r);
  }
  HIPCHK(hipMemcpyAsync(s->dl_base, s->d.bits + (size_t)s->lo * s->d.NWR, bytes, hipMemcpyDeviceToDevice, s->st));   // d.bits is biased by -lo rows
  HIPCHK(hipMemcpyAsync(s->dl_run, s->d.alive, s->C, hipMemcpyDeviceToDevice, s->st));
  HIPCHK(hipStreamSynchronize(s->st));
  s->dl_round = s->round;
  return KB_OK;
}
static int dl_mark(SpSim*) { return KB_INVALID_OPERATION; }     // not reached: census_gate refuses sparse rows
static bool dl_marked(kb_sim* s) { return s->dl_base != nullptr; }
static bool dl_marked(SpSim*) { return false; }

// one leaf's pass
static int dl_leaf(kb_sim* s, bool advance, int32_t* round_base, DlPart& p) {
  (void)hipSetDevice(s->device);
  const Dev& d = s->d;
  kb::DlArgs a{};
  a.now = d.bits + (size_t)s->lo * d.NWR; a.base = s->dl_base; a.run_now = d.alive; a.run_base = s->dl_run;
  a.C = s->C; a.NWR = d.NWR; a.lo = s->lo; a.R = s->R; a.advance = advance;
  // env KB_DELTA_RPW overrides the rows per wave (tools/delta_census_cost.py records its value)
  auto lay = [&](Carve& c) { dl_lay(c, a, s->W, s->ncu, rpw_env("KB_DELTA_RPW")); };
  if (!s->dl_buf) HIPCHK(talloc(s, &s->dl_buf, carve_bytes(lay) / 4));
  const Carve c = carve(s->dl_buf, lay);
  *round_base = s->dl_round;
  const int rc = dl_exec(c, a, s->W, s->st, p);
  if (rc) return rc;
  if (p.ext.empty()) {                                           // replicated: the first leaf's copy
    HIPCHK(fetch(p.ext, d.ext, s->C, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
  }
  if (advance) {                                                 // the pass stored the bits: the running set follows
    HIPCHK(hipMemcpyAsync(s->dl_run, d.alive, s->C, hipMemcpyDeviceToDevice, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    s->dl_round = s->round;
  }
  return KB_OK;
}
static int dl_leaf(SpSim*, bool, int32_t*, DlPart&) { return KB_INVALID_OPERATION; }   // not reached

static const Refuse DL_REFUSE = {" and a baseline of the whole mesh spans ranks", "keep no member bits to take a baseline of", nullptr};

extern "C" int kb_sim_delta_mark(kb_sim* s) {
  if (!s) return KB_INVALID_ARGUMENT;
  { const int rc = census_gate(s, "kb_sim_delta_mark", DL_REFUSE); if (rc) return rc; }
  const int rc = route(s, R_ALL, 0, [](auto* e) { return dl_mark(e); });
  if (rc) route(s, R_ALL, 0, [](auto* e) { dl_drop(e); return KB_OK; });   // no shard keeps half a baseline
  return rc;
}

extern "C" int kb_sim_delta_release(kb_sim* s) {
  if (!s) return KB_INVALID_ARGUMENT;
  { const int rc = census_gate(s, "kb_sim_delta_release", DL_REFUSE); if (rc) return rc; }
  return route(s, R_ALL, 0, [](auto* e) { dl_drop(e); return KB_OK; });
}

extern "C" int kb_sim_delta_census(kb_sim* s, kb_delta* out, uint32_t* gained_by, uint32_t* lost_by, size_t cap_ids,
                                   uint32_t* gained, uint32_t* lost, uint32_t* lost_live, size_t cap_rows, uint32_t flags) {
  if (!s) return KB_INVALID_ARGUMENT;
  { const int rc = census_caps("kb_sim_delta_census", out, any_of(gained_by, lost_by), cap_ids, s->C,
                               any_of(gained, lost, lost_live), cap_rows, s->C); if (rc) return rc; }
  if (flags & ~KB_DELTA_ADVANCE) { seterr("kb_sim_delta_census: unknown flags"); return KB_INVALID_ARGUMENT; }
  { const int rc = census_gate(s, "kb_sim_delta_census", DL_REFUSE); if (rc) return rc; }
  bool marked = true;
  route(s, R_ALL, 0, [&](auto* e) { marked = marked && dl_marked(e); return KB_OK; });
  if (!marked) { seterr("kb_sim_delta_census: no baseline (kb_sim_delta_mark takes one)"); return KB_INVALID_OPERATION; }
  DlPart p;
  dl_part_init(p, s->C);
  int32_t round = 0, round_base = 0;
  { const int rc = route(s, R_FIRST, 0, [&](auto* e) { round = e->round; return KB_OK; }); if (rc) return rc; }
  { const int rc = route(s, R_ALL, 0, [&](auto* e) { return dl_leaf(e, (flags & KB_DELTA_ADVANCE) != 0, &round_base, p); }); if (rc) return rc; }
  s->census_ms[CM_DELTA] = p.ms;
  dl_summary(p, round_base, round, out);
  dl_deliver(p, gained_by, lost_by, gained, lost, lost_live);
  return KB_OK;
}

extern "C" int kb_sim_delta_device_ms(kb_sim* s, double* ms) { return census_ms_get(s, CM_DELTA, ms); }

extern "C" int kb_delta_of(int device, const uint32_t* bits_base, const uint8_t* run_base, const uint32_t* bits_now,
                           const uint8_t* run_now, const uint8_t* external, size_t capacity, size_t row_lo, size_t rows,
                           uint32_t rpw, kb_delta* out, uint32_t* gained_by, uint32_t* lost_by, size_t cap_ids,
                           uint32_t* gained, uint32_t* lost, uint32_t* lost_live, size_t cap_rows) {
  { const int rc = census_caps("kb_delta_of", out, any_of(gained_by, lost_by), cap_ids, capacity,
                               any_of(gained, lost, lost_live), cap_rows, capacity); if (rc) return rc; }
  if (capacity == 0 || capacity > (1u << 24)) { seterr("kb_delta_of: capacity outside 1 .. 2^24"); return KB_CAPACITY; }
  if (row_lo > capacity || rows > capacity - row_lo) { seterr("kb_delta_of: the rows are ids below the capacity"); return KB_INVALID_ARGUMENT; }
  if (!run_base || !run_now || !external || (rows && (!bits_base || !bits_now))) return KB_INVALID_ARGUMENT;
  OfScope o;
  { const int rc = o.open(device, "kb_delta_of"); if (rc) return rc; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { seterr("kb_delta_of: hipGetDeviceProperties failed"); return KB_NO_DEVICE; }
  const uint32_t C = (uint32_t)capacity, R = (uint32_t)rows, W = (C + 8191) / 8192 * 8192, NWR = W / 32;
  kb::DlArgs a{};
  a.C = C; a.NWR = NWR; a.lo = (uint32_t)row_lo; a.R = R; a.advance = 0;
  const size_t bits_n = (size_t)R * NWR;
  uint32_t* now = nullptr; uint8_t* rn = nullptr; uint8_t* rb = nullptr;
  auto lay = [&](Carve& c) {                      // the scratch, the two bit tables (8-byte loads), the flags
    dl_lay(c, a, W, (uint32_t)prop.multiProcessorCount, rpw);
    now = c.take<uint32_t>(bits_n, 8); a.base = c.take<uint32_t>(bits_n, 8); rn = c.take<uint8_t>(C); rb = c.take<uint8_t>(C);
  };
  { const int rc = dev_reserve(&o.buf, &o.cap, carve_bytes(lay), "kb_delta_of: device allocation failed"); if (rc) return rc; }
  const Carve c = carve(o.buf, lay);
  a.now = now; a.run_now = rn; a.run_base = rb;
  if (bits_n) {
    HIPCHK(hipMemcpyAsync(now, bits_now, 4 * bits_n, hipMemcpyHostToDevice, o.st));
    HIPCHK(hipMemcpyAsync(a.base, bits_base, 4 * bits_n, hipMemcpyHostToDevice, o.st));
  }
  HIPCHK(hipMemcpyAsync(rn, run_now, C, hipMemcpyHostToDevice, o.st));
  HIPCHK(hipMemcpyAsync(rb, run_base, C, hipMemcpyHostToDevice, o.st));
  DlPart p;
  dl_part_init(p, C);
  { const int rc = dl_exec(c, a, W, o.st, p); if (rc) return rc; }
  p.ext.assign(external, external + C);
  dl_summary(p, -1, -1, out);
  dl_deliver(p, gained_by, lost_by, gained, lost, lost_live);
  return KB_OK;
}
