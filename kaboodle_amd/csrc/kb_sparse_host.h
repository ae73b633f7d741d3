// kb_sparse_host.h — host side of the sparse-row engine (kb_sparse.h): one handle per mesh, the round's
// launch sequence, and the C-ABI surface of include/kaboodle_sim.h for handles created with
// KB_VARIANT_SPARSE_ROWS.  Included by kb_sim.hip after its host helpers (seterr, HIPCHK, the scan, the CRC
// tables, kb_format_addr, default_identity).
#pragma once
#include <algorithm>
#include <array>
#include <string>
#include <vector>

namespace kb {

enum SpKId : int {
  SPK_REBASE, SPK_EVENTS, SPK_CHURN, SPK_BCAST, SPK_BOUND0, SPK_JRESP, SPK_TRUEFP, SPK_TICK, SPK_BCAST_WRITE, SPK_SCAN,
  SPK_COMPACT, SPK_ROUTE, SPK_PAYBOUND, SPK_SCATTER, SPK_HANDLE, SPK_WINDOW, SPK_ROUND_END, SPK_BFAIL_SF, SPK_N
};
static const char* const SPK_NAME[SPK_N] = {
  "k_sp_rebase", "k_sp_events", "k_sp_churn", "k_sp_bcast", "k_sp_bound0", "k_sp_jresp", "k_sp_truefp", "k_sp_tick",
  "k_sp_bcast_write", "k_sp_scan", "k_sp_compact", "k_sp_route", "k_sp_paybound", "k_sp_scatter", "k_sp_handle",
  "k_sp_window", "k_sp_round_end", "k_sp_bfail_sf"};

struct SpSim {
  kb_config cfg;
  SpDev d;
  int device = 0;
  hipStream_t st = nullptr;
  uint32_t C = 0;
  // row shard: rows [lo, hi) of the mesh, RS rows per rank; xf null = unsharded
  int rank = 0, world = 1;
  uint32_t lo = 0, hi = 0, R = 0, RS = 0;
  Xfer* xf = nullptr;
  bool in_group = false;                            // a shard of a kb_sim_create_local group (the façade sums)
  SpX x;                                            // the waves' send side
  size_t smsg_cap = 0, spay_cap = 0;
  Msg* rmsg = nullptr; uint32_t* rpay = nullptr; uint8_t* rstat = nullptr;
  size_t rmsg_cap = 0, rpay_cap = 0, rstat_cap = 0;
  uint32_t* xall = nullptr;                         // all-gathered counts
  std::vector<uint32_t> h_xall;
  BCast* bjoin_loc = nullptr; BCast* bfail_loc = nullptr;   // this shard's broadcast lists before the all-gather
  uint32_t* rpack = nullptr; uint32_t* rpack_in = nullptr;  // a restart's packed row (send / receive)
  unsigned long long* xstats = nullptr;             // ranks: the counters summed over the mesh
  int32_t round = 0;
  std::vector<void*> allocs;
  std::vector<uint8_t> h_ident, h_idlen, h_pend, h_moved, h_idset;
  std::vector<int16_t> h_pendlen;
  std::vector<uint32_t> h_bbits;
  std::vector<Event> events;
  Event* d_events = nullptr; size_t events_cap = 0;
  std::vector<kb_wire_addr> probe_q, probes;
  std::vector<kb_probe_response> presp;
  uint2* d_presp = nullptr; uint32_t* d_presp_n = nullptr; size_t presp_cap = 0;
  BCast* bjoin = nullptr; BCast* bfail = nullptr;
  uint32_t* fkey = nullptr;                         // the Failed list packed for k_sp_bfail_sf (padded to 4)
  uint32_t nj = 0, nf = 0;
  uint64_t bj_total = 0, bf_total = 0;
  uint32_t* jnew = nullptr; uint32_t* jresp = nullptr; size_t jw_cap = 0;
  uint32_t* jr_n = nullptr; uint32_t* jr_pay = nullptr;
  SpTickOut bo;
  uint32_t* joff = nullptr; uint32_t* foff = nullptr;
  Msg* out[2] = {nullptr, nullptr}; size_t out_cap[2] = {0, 0};
  Msg* stage = nullptr; size_t stage_cap = 0;
  uint32_t* pool[2] = {nullptr, nullptr}; size_t pool_cap[2] = {0, 0};
  uint32_t* inbox = nullptr; size_t inbox_cap = 0;
  uint8_t* status = nullptr; size_t status_cap = 0;
  uint32_t *icnt = nullptr, *icur = nullptr, *ebound = nullptr, *kprc = nullptr, *pb = nullptr;
  uint32_t *ioff = nullptr, *eoff = nullptr, *poff = nullptr, *en = nullptr, *ooff = nullptr;
  uint32_t* scan_tiles = nullptr; uint32_t* scan_tot = nullptr;
  uint2* tfpart = nullptr; uint32_t* tfp = nullptr;
  std::vector<uint32_t> watch_node, watch_fp;
  std::vector<std::vector<uint8_t>> watch_snap;
  // profile: with prof_level > 0 every launch carries start/stop events on its own dispatch packet
  int prof_level = 0;
  struct Rec { int kid; hipEvent_t a, b; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> ev_free;
  double k_ms[SPK_N] = {};
  uint64_t k_n[SPK_N] = {};
  double round_ms = 0; uint64_t round_n = 0;
  uint64_t host_syncs = 0;
  uint32_t* cs_buf = nullptr;                       // the census's scratch (kb_census.h), allocated by the first census
  uint32_t* ag_buf = nullptr;                       // the contact-age census's scratch (kb_agecensus.h), allocated by its first call
  // external peers
  std::vector<uint8_t> h_ext;
  size_t n_ext = 0;
  std::vector<XRec> inj; std::vector<uint32_t> inj_ids;
  std::vector<uint32_t> inj_join;                    // external peers' Join broadcasts for the next round
  XRec* d_inj = nullptr; uint32_t* d_inj_ids = nullptr; size_t d_inj_cap = 0, d_inj_ids_cap = 0;
  std::vector<kb_unicast> xq; std::vector<uint32_t> xq_ids;
  // snapshot and restore (kb_snapshot.h): the scratch is allocated by the first call
  unsigned long long* sn_fix = nullptr;             // the rows' entry offsets, the scan's tile sums, the canonical fingerprints
  uint32_t* sn_buf = nullptr; size_t sn_cap = 0;    // the packed entries, grown on demand
  uint64_t sn_total = 0;                            // entries of this handle's rows at the last scan
  double sn_ms = 0;                                 // device time of the last pack or unpack
};

static int sp_err_status(uint32_t e) {
  if (!e) return KB_OK;
  const char* what[] = {"", "suspect slots exhausted", "outbox region overflow", "payload pool overflow", "?", "inbox overflow",
                        "Join response member count mismatch", "?", "indirect-ping candidate out of range", "?",
                        "a row's entry list exceeded kb_config.sparse_row_cap", "export buffer overflow"};
  seterr(std::string("device capacity error: ") + (e <= 11 ? what[e] : "?"));
  return KB_CAPACITY;
}
// zeroed device memory.  The zeroing is complete on return: hipMemset runs on the null stream, which does not
// order with the simulator's non-blocking stream, so a kernel enqueued next could otherwise run before it
template <class T> static hipError_t sp_alloc(SpSim* S, T** p, size_t n) {
  hipError_t e = hipMalloc((void**)p, sizeof(T) * (n ? n : 1));
  if (e == hipSuccess) e = hipMemset(*p, 0, sizeof(T) * (n ? n : 1));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) S->allocs.push_back((void*)*p);
  return e;
}
// a row table: per_row elements for each of the shard's rows, the pointer biased by -lo rows (kernels index it
// with global ids); SL gives the local base of a one-per-row table
template <class T> static hipError_t sp_ralloc(SpSim* S, T** p, size_t per_row) {
  T* base = nullptr;
  const hipError_t e = sp_alloc(S, &base, per_row * S->R);
  *p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) - sizeof(T) * per_row * S->lo);
  return e;
}
template <class T> static T* SL(const SpSim* S, T* p) { return p + S->lo; }
template <class T> static hipError_t eng_alloc(SpSim* S, T** p, size_t n) { return sp_alloc(S, p, n); }   // kb_roundframe.h's hooks
static const char* eng_alloc_what(SpSim*) { return "sparse engine: device allocation failed: "; }
// a dynamic buffer of at least `need` elements (contents are not kept), grown with a quarter's slack
template <class T> static int sp_grow(SpSim* S, T** p, size_t* cap, size_t need) {
  if (need <= *cap && *p) return KB_OK;
  return eng_grow(S, p, cap, std::max<size_t>(need + need / 4, 1024));
}
static void sp_prof(SpSim* S, int kid, hipEvent_t* a, hipEvent_t* b) {
  *a = *b = nullptr;
  if (S->prof_level <= 0) return;
  hipEvent_t e[2];
  for (int k = 0; k < 2; ++k) {
    if (!S->ev_free.empty()) { e[k] = S->ev_free.back(); S->ev_free.pop_back(); }
    else if (hipEventCreate(&e[k]) != hipSuccess) { if (k) S->ev_free.push_back(e[0]); return; }
  }
  *a = e[0]; *b = e[1];
  S->recs.push_back(SpSim::Rec{kid, e[0], e[1]});
}
template <typename F, typename... Args>
static void sp_launch(SpSim* S, int kid, F kern, uint32_t grid, uint32_t block, Args... args) {
  if (!grid) return;
  hipEvent_t a, b;
  sp_prof(S, kid, &a, &b);
  hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, S->st, a, b, 0, args...);
}
static void sp_prof_resolve(SpSim* S) {
  for (const auto& q : S->recs) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, q.a, q.b) == hipSuccess) {
      if (q.kid == SPK_N) { S->round_ms += ms; S->round_n++; }
      else { S->k_ms[q.kid] += ms; S->k_n[q.kid]++; }
    }
    S->ev_free.push_back(q.a); S->ev_free.push_back(q.b);
  }
  S->recs.clear();
}
static hipError_t sp_sync(SpSim* S) { S->host_syncs++; return hipStreamSynchronize(S->st); }
// exclusive scans of up to 4 arrays of n elements (the shard's rows: local bases), totals into scan_tot[t0..]
static void sp_scan(SpSim* S, uint32_t n, int narr, const uint32_t* const* in, uint32_t* const* out, uint32_t t0) {
  ScanArgs a;
  memset(&a, 0, sizeof a);
  a.n = n; a.narr = narr; a.totals = S->scan_tot + t0; a.tiles = S->scan_tiles; a.ntiles = (n + 1023) / 1024;
  for (int q = 0; q < narr; ++q) { a.in[q] = in[q]; a.out[q] = out[q]; }
  sp_launch(S, SPK_SCAN, k_scan_tiles, a.ntiles, 1024, a);
  sp_launch(S, SPK_SCAN, k_scan_apply, a.ntiles, 1024, a);
}

// per-id segment CRCs and uniformity (identity changes), on the host tables
static int upload_segments(SpSim* S) {
  const uint32_t C = S->C;
  std::vector<uint32_t> cseg(C), segmul(C), seglen(C);
  bool uniform = true;
  uint32_t xp[ADDR_LEN + MAXID + 1];                 // x^(8 len) per segment length
  for (uint32_t l = 0; l <= ADDR_LEN + MAXID; ++l) xp[l] = h_xpow8(l);
  for (uint32_t j = 0; j < C; ++j) {
    char a[32]; kb_format_addr(j, a, sizeof a);
    uint32_t reg = h_crc_update(0, (const uint8_t*)a, ADDR_LEN);
    reg = h_crc_update(reg, &S->h_ident[(size_t)j * MAXID], S->h_idlen[j]);
    cseg[j] = reg; seglen[j] = ADDR_LEN + S->h_idlen[j]; segmul[j] = xp[seglen[j]];
    if (S->h_idlen[j] != S->cfg.id_len) uniform = false;
  }
  S->d.uniform = uniform ? 1 : 0;
  HIPCHK(hipMemcpy(S->d.cseg, cseg.data(), 4ull * C, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(S->d.segmul, segmul.data(), 4ull * C, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(S->d.seglen, seglen.data(), 4ull * C, hipMemcpyHostToDevice));
  return KB_OK;
}

static void sp_destroy(SpSim* S) {
  if (!S) return;
  (void)hipSetDevice(S->device);
  if (S->st) (void)hipStreamSynchronize(S->st);
  for (void* p : S->allocs) (void)hipFree(p);
  for (auto& q : S->recs) { (void)hipEventDestroy(q.a); (void)hipEventDestroy(q.b); }
  for (hipEvent_t e : S->ev_free) (void)hipEventDestroy(e);
  if (S->st) (void)hipStreamDestroy(S->st);
  delete S->xf;
  delete S;
}

// kb_sim_create with KB_VARIANT_SPARSE_ROWS: the whole mesh (xf null), or rank `rank` of `world` row shards
// exchanging over xf (kb_sim_create_local / kb_sim_create_rank; the handle owns xf)
static int sp_create(const kb_config* cfg, int rank, int world, Xfer* xf, SpSim** out) {
  h_crc_init();
  if (cfg->variant != KB_VARIANT_SPARSE_ROWS) { seterr("the sparse rows take no other semantic variant"); delete xf; return KB_INVALID_ARGUMENT; }
  if (cfg->track_latency) { seterr("sparse rows keep no latency table"); delete xf; return KB_INVALID_ARGUMENT; }
  if (cfg->stat_flags & ~(uint32_t)KB_STAT_NO_SF_FAILED_DROPS) { seterr("unknown kb_config.stat_flags"); delete xf; return KB_INVALID_ARGUMENT; }
  const uint32_t C = cfg->capacity;
  const uint32_t RS = (C + (uint32_t)world - 1) / (uint32_t)world;
  if (world < 1 || world > (int)XMAX || rank < 0 || rank >= world || (uint64_t)(world - 1) * RS >= C) {
    seterr("shard layout out of range (1..8 shards, each holding at least one row)"); delete xf; return KB_INVALID_ARGUMENT;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { seterr("no HIP device"); delete xf; return KB_NO_DEVICE; }
  SpSim* S = new SpSim();
  memset((void*)&S->d, 0, sizeof S->d);
  memset((void*)&S->x, 0, sizeof S->x);
  S->cfg = *cfg;
  S->xf = xf;
  S->rank = rank; S->world = world; S->RS = RS;
  S->lo = (uint32_t)rank * RS; S->hi = std::min<uint32_t>(C, S->lo + RS); S->R = S->hi - S->lo;
  S->device = cfg->device >= 0 ? cfg->device : 0;
  if (cfg->device < 0) (void)hipGetDevice(&S->device);
  if (hipSetDevice(S->device) != hipSuccess) { sp_destroy(S); seterr("hipSetDevice failed"); return KB_NO_DEVICE; }
  S->C = C;
  const uint32_t R = S->R;
  SpDev& d = S->d;
  d.C = C; d.lo = S->lo; d.hi = S->hi; d.rank0 = rank == 0 ? 1u : 0u;
  d.ECAP = cfg->sparse_row_cap ? std::min<uint32_t>(cfg->sparse_row_cap, C) : std::min<uint32_t>(C, 4096u);
  d.ESTR = (d.ECAP + 3u) & ~3u;
  d.nb = cfg->init_mode == KB_INIT_CONVERGED ? cfg->initial_nodes : 0u;
  d.k0 = (uint32_t)cfg->seed; d.k1 = (uint32_t)(cfg->seed >> 32);
  d.loss_thr = cfg->loss_threshold; d.churn_thr = cfg->churn_threshold; d.fault_end = cfg->fault_end_round;
  d.failed_mode = cfg->failed_mode; d.pgroups = cfg->partition_groups; d.pstart = cfg->partition_start; d.pend = cfg->partition_end;
  const uint32_t Lid = cfg->id_len;
  d.L = ADDR_LEN + Lid;
  d.capk = (BUFSZ - 20 - Lid) / (18 + Lid);             // KPR reply: 20 + L + k(18+L) <= 10240
  d.capj = (BUFSZ - 20 - Lid - 1) / (18 + Lid);         // Join response: 20 + L + k(18+L) < 10240
  S->h_ident.assign((size_t)C * MAXID, 0); S->h_idlen.assign(C, (uint8_t)Lid);
  S->h_pend.assign((size_t)C * MAXID, 0); S->h_pendlen.assign(C, (int16_t)-1); S->h_moved.assign(C, 0);
  S->h_idset.assign(C, 0);
  for (uint32_t j = 0; j < C; ++j) default_identity(j, Lid, &S->h_ident[(size_t)j * MAXID]);
  hipError_t e = hipSuccess;
#define SA(ptr, n) if (e == hipSuccess) e = sp_alloc(S, &(ptr), (n))     // per-id and global tables
#define SR(ptr, n) if (e == hipSuccess) e = sp_ralloc(S, &(ptr), (n))    // row tables: n per local row
  SR(d.ent, d.ESTR); SR(d.ne, 1); SR(d.based, 1); SR(d.n, 1); SR(d.fp, 1); SR(d.dirty, 1);
  SR(d.last_bcast, 1); SR(d.a3cur, 1); SR(d.susp, SLOTS); SR(d.cur, CSLOTS);
  SR(d.paq, PAQ); SR(d.paq_n, 1); SA(d.alive, C); SA(d.start_round, C); SA(d.idset, C); SA(d.ext, C);
  SA(d.cseg, C); SA(d.segmul, C); SA(d.seglen, C); SA(d.bbits, C / 32 + 1); SA(d.bcnt, (size_t)C + 1);
  SA(d.bpre, (size_t)C + 1); SA(d.zpow, (size_t)C + 2); SA(d.stats, NSTAT); SA(d.sacc, (size_t)SP_ACC * NSTAT);
  SA(d.ctr, NCTR); SA(d.tacc, 2 * SP_ACC);
  SA(S->bjoin, C); SA(S->bfail, (size_t)C * SLOTS); SA(S->fkey, (size_t)C * SLOTS + 4); SR(S->jr_n, 1); SR(S->jr_pay, 1);
  SR(S->bo.bj, 1); SR(S->bo.bnf, 1); SR(S->bo.bfp, SLOTS); SR(S->joff, 1); SR(S->foff, 1);
  SR(S->icnt, 1); SR(S->icur, 1); SR(S->ebound, 1); SR(S->kprc, 1); SR(S->pb, 1);
  SR(S->ioff, 1); SR(S->eoff, 1); SR(S->poff, 1); SR(S->en, 1); SR(S->ooff, 1);
  SA(S->scan_tiles, 5 * ((std::max<size_t>(C, (size_t)world * R) + 1023) / 1024) + 5); SA(S->scan_tot, 32);
  SA(S->tfpart, SP_TFP); SA(S->tfp, 1);
  if (xf) {
    SpX& x = S->x;
    x.world = (uint32_t)world; x.R = R; x.S = RS;
    SA(x.xcnt, (size_t)world * R); SA(x.xpay, (size_t)world * R); SA(x.xoff, (size_t)world * R); SA(x.xpoff, (size_t)world * R);
    SA(x.xb, 2 * world); SA(S->xall, 2 * world * world); SA(S->xstats, NSTAT);
    SA(S->bjoin_loc, R); SA(S->bfail_loc, (size_t)R * SLOTS);
    S->h_xall.assign(2 * world * world, 0);
  }
#undef SA
#undef SR
  if (e != hipSuccess) { seterr(std::string("sparse engine: device allocation failed: ") + hipGetErrorString(e)); sp_destroy(S); return KB_CAPACITY; }
  if (hipStreamCreateWithFlags(&S->st, hipStreamNonBlocking) != hipSuccess) { sp_destroy(S); seterr("stream"); return KB_IO_ERROR; }
  if (const char* pv = getenv("KB_PROF")) S->prof_level = atoi(pv);
  { const int rc = upload_segments(S); if (rc) { sp_destroy(S); return rc; } }
  // the base (the initial members of a converged start) with its prefix counts and prefix folds, and Z^k
  {
    const uint32_t nb = d.nb;
    S->h_bbits.assign(C / 32 + 1, 0);
    for (uint32_t j = 0; j < nb; ++j) S->h_bbits[j >> 5] |= 1u << (j & 31);
    std::vector<uint32_t> bcnt((size_t)C + 1), bpre((size_t)C + 1), zpow((size_t)C + 2), cseg(C);
    if (hipMemcpy(cseg.data(), d.cseg, 4ull * C, hipMemcpyDeviceToHost) != hipSuccess) { sp_destroy(S); seterr("cseg"); return KB_IO_ERROR; }
    const uint32_t Z = h_xpow8(d.L);
    zpow[0] = 0x80000000u;
    for (size_t k = 1; k < zpow.size(); ++k) zpow[k] = multmodp(Z, zpow[k - 1]);
    uint32_t raw = 0, c = 0;
    for (uint32_t j = 0; j <= C; ++j) {
      bcnt[j] = c; bpre[j] = raw;
      if (j < C && j < nb) { raw = multmodp(Z, raw) ^ cseg[j]; c++; }
    }
    if (hipMemcpy(d.bbits, S->h_bbits.data(), 4ull * S->h_bbits.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d.bcnt, bcnt.data(), 4ull * bcnt.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d.bpre, bpre.data(), 4ull * bpre.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d.zpow, zpow.data(), 4ull * zpow.size(), hipMemcpyHostToDevice) != hipSuccess) {
      sp_destroy(S); seterr("base tables"); return KB_IO_ERROR;
    }
  }
  uint32_t ctr0[NCTR] = {0};
  ctr0[C_NEXTFREE] = cfg->initial_nodes;
  ctr0[C_FIRSTCONV] = 0xFFFFFFFFu; ctr0[C_LASTCONV] = 0xFFFFFFFFu;
  if (hipMemcpy(d.ctr, ctr0, sizeof ctr0, hipMemcpyHostToDevice) != hipSuccess) { sp_destroy(S); seterr("ctr upload"); return KB_IO_ERROR; }
  k_sp_init<<<(C + 255) / 256, 256, 0, S->st>>>(d, cfg->initial_nodes, cfg->init_mode == KB_INIT_CONVERGED ? 1u : 0u);
  if (hipStreamSynchronize(S->st) != hipSuccess) { sp_destroy(S); seterr("init failed"); return KB_IO_ERROR; }
  *out = S;
  return KB_OK;
}

static int read_row(SpSim* S, uint32_t node, std::vector<uint8_t>& rw);
static int sp_xfail(SpSim* S) { seterr(S->xf->error()); return KB_IO_ERROR; }
// one all-to-all-v pair (records + ids, or two lists) as one group; an opened group is always closed
static int sp_a2a2(SpSim* S, const void* s1, const size_t* sc1, const size_t* sd1, void* r1, const size_t* rc1, const size_t* rd1,
                   size_t e1, const void* s2, const size_t* sc2, const size_t* sd2, void* r2, const size_t* rc2, const size_t* rd2,
                   size_t e2) {
  if (!S->xf->group_begin()) return sp_xfail(S);
  const bool sent = S->xf->alltoallv(s1, sc1, sd1, r1, rc1, rd1, e1, S->st) && (!s2 || S->xf->alltoallv(s2, sc2, sd2, r2, rc2, rd2, e2, S->st));
  const std::string err = sent ? std::string() : S->xf->error();
  if (!S->xf->group_end() || !sent) { seterr(sent ? S->xf->error() : err); return KB_IO_ERROR; }
  return KB_OK;
}

// A restart's map across shards: the old address's row, packed on the shard holding it,
// moves to the shard holding the fresh address (an all-to-all-v with one non-empty pair, on every rank); the
// instance's event observer moves with it (the map and its observer belong to the Kaboodle, src/lib.rs:104).
// *snap_after: an observer attached to the fresh address before this round takes its snapshot once the restart
// has applied (the instance had none)
static int sp_move_row(SpSim* S, uint32_t from, uint32_t to, bool* snap_after) {
  *snap_after = false;
  const uint32_t nw = (S->C + 31) / 32, ext0 = SP_PACK_HDR + S->d.ESTR;
  const size_t words = (size_t)ext0 + 2 + nw;           // row, then [watched, fp, snapshot bits]
  if (!S->rpack) { HIPCHK(sp_alloc(S, &S->rpack, words)); HIPCHK(sp_alloc(S, &S->rpack_in, words)); }
  const bool have = from >= S->lo && from < S->hi, take = to >= S->lo && to < S->hi;
  if (have) {
    k_sp_row_pack<<<8, 256, 0, S->st>>>(S->d, from, S->rpack);
    std::vector<uint32_t> ext(2 + nw, 0);
    size_t kf = 0;
    while (kf < S->watch_node.size() && S->watch_node[kf] != from) ++kf;
    if (kf < S->watch_node.size()) {
      ext[0] = 1; ext[1] = S->watch_fp[kf];
      for (uint32_t j = 0; j < S->C; ++j) if (S->watch_snap[kf][j]) ext[2 + (j >> 5)] |= 1u << (j & 31);
      S->watch_node.erase(S->watch_node.begin() + kf); S->watch_fp.erase(S->watch_fp.begin() + kf);
      S->watch_snap.erase(S->watch_snap.begin() + kf);
    }
    HIPCHK(hipMemcpyAsync(S->rpack + ext0, ext.data(), 4 * ext.size(), hipMemcpyHostToDevice, S->st));
    HIPCHK(sp_sync(S));
  }
  size_t sc[XMAX] = {}, sd[XMAX] = {}, rc[XMAX] = {}, rd[XMAX] = {};
  const int ofrom = (int)(from / S->RS), oto = (int)(to / S->RS);
  if (S->rank == ofrom) sc[oto] = words;
  if (S->rank == oto) rc[ofrom] = words;
  { const int rc2 = sp_a2a2(S, S->rpack, sc, sd, S->rpack_in, rc, rd, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0); if (rc2) return rc2; }
  if (!take) return KB_OK;
  k_sp_row_unpack<<<8, 256, 0, S->st>>>(S->d, to, S->rpack_in);
  std::vector<uint32_t> ext(2 + nw);
  HIPCHK(hipMemcpyAsync(ext.data(), S->rpack_in + ext0, 4 * ext.size(), hipMemcpyDeviceToHost, S->st));
  HIPCHK(sp_sync(S));
  size_t kt = 0;
  while (kt < S->watch_node.size() && S->watch_node[kt] != to) ++kt;
  if (ext[0]) {
    if (kt == S->watch_node.size()) { S->watch_node.push_back(to); S->watch_fp.push_back(0); S->watch_snap.emplace_back(S->C, 0); }
    S->watch_fp[kt] = ext[1];
    for (uint32_t j = 0; j < S->C; ++j) S->watch_snap[kt][j] = (uint8_t)((ext[2 + (j >> 5)] >> (j & 31)) & 1u);
  } else if (kt < S->watch_node.size()) {
    *snap_after = true;
  }
  return KB_OK;
}

// API events in call order (src/lib.rs:136-183); a restart moves the map to its fresh address
static int sp_apply_events(SpSim* S, int32_t r) {
  SpDev& d = S->d;
  const uint32_t C = S->C;
  if (S->events.empty()) return KB_OK;
  if (S->xf) for (Event& ev : S->events) if (ev.kind == EV_RESTART) ev.kind = EV_START_MOVED;   // the row moves on the host
  { const int rc = round_upload_events(S); if (rc) return rc; }
  size_t k0 = 0;
  for (size_t k = 0; k < S->events.size(); ++k) {
    const Event& ev = S->events[k];
    if (ev.kind == EV_START_MOVED) {                   // sharded restart: events before it, the row move, its start
      if (k > k0) sp_launch(S, SPK_EVENTS, k_sp_events, 1, 1, d, (const Event*)S->d_events + k0, (uint32_t)(k - k0), r);
      bool snap_after = false;
      { const int rc = sp_move_row(S, ev.src, ev.node, &snap_after); if (rc) return rc; }
      sp_launch(S, SPK_EVENTS, k_sp_events, 1, 1, d, (const Event*)S->d_events + k, 1u, r);
      k0 = k + 1;
      if (snap_after) {
        std::vector<uint8_t> rw;
        HIPCHK(sp_sync(S));
        const int rc = read_row(S, ev.node, rw);
        if (rc) return rc;
        for (size_t q = 0; q < S->watch_node.size(); ++q)
          if (S->watch_node[q] == ev.node) for (uint32_t j = 0; j < C; ++j) S->watch_snap[q][j] = rw[j] != 0;
      }
      continue;
    }
    if (ev.kind != EV_RESTART) continue;
    // unsharded: the map's observer follows the instance.  An observer attached to the new address before this
    // round gives way to the instance's own, or (the instance had none) starts from the row the restart leaves,
    // so it reports only later changes
    size_t kf = S->watch_node.size(), kt = S->watch_node.size();
    for (size_t q = 0; q < S->watch_node.size(); ++q) { if (S->watch_node[q] == ev.src) kf = q; if (S->watch_node[q] == ev.node) kt = q; }
    if (kf < S->watch_node.size()) {
      if (kt < S->watch_node.size()) {
        S->watch_node.erase(S->watch_node.begin() + kt); S->watch_fp.erase(S->watch_fp.begin() + kt);
        S->watch_snap.erase(S->watch_snap.begin() + kt);
        if (kf > kt) kf--;
      }
      S->watch_node[kf] = ev.node;
    } else if (kt < S->watch_node.size()) {
      sp_launch(S, SPK_EVENTS, k_sp_events, 1, 1, d, (const Event*)S->d_events + k0, (uint32_t)(k + 1 - k0), r);
      k0 = k + 1;
      std::vector<uint8_t> rw;
      HIPCHK(sp_sync(S));
      const int rc = read_row(S, ev.node, rw);
      if (rc) return rc;
      for (uint32_t j = 0; j < C; ++j) S->watch_snap[kt][j] = rw[j] != 0;
    }
  }
  if (k0 < S->events.size())
    sp_launch(S, SPK_EVENTS, k_sp_events, 1, 1, d, (const Event*)S->d_events + k0, (uint32_t)(S->events.size() - k0), r);
  HIPCHK(sp_sync(S));
  S->events.clear();
  return KB_OK;
}

// sharded: every shard's broadcast lists, concatenated in rank order = sender order (one all-gather of the counts,
// then each shard's lists to every rank)
static int sp_gather_bcasts(SpSim* S, uint32_t nj_loc, uint32_t nf_loc, uint32_t* nj, uint32_t* nf) {
  const int W = S->world;
  if (!S->xf->allgather_u32(S->scan_tot + 2, S->xall, 2, S->st)) return sp_xfail(S);
  HIPCHK(hipMemcpyAsync(S->h_xall.data(), S->xall, 8ull * W, hipMemcpyDeviceToHost, S->st));
  HIPCHK(sp_sync(S));
  size_t sc[XMAX], sd[XMAX], rc[XMAX], rd[XMAX], fsc[XMAX], frc[XMAX], frd[XMAX];
  size_t oj = 0, of = 0;
  for (int k = 0; k < W; ++k) {
    rc[k] = S->h_xall[2 * k]; frc[k] = S->h_xall[2 * k + 1];
    rd[k] = oj; oj += rc[k]; frd[k] = of; of += frc[k];
    sc[k] = nj_loc; fsc[k] = nf_loc; sd[k] = 0;
  }
  const int rc2 = sp_a2a2(S, S->bjoin_loc, sc, sd, S->bjoin, rc, rd, sizeof(BCast), S->bfail_loc, fsc, sd, S->bfail, frc, frd, sizeof(BCast));
  if (rc2) return rc2;
  *nj = (uint32_t)oj; *nf = (uint32_t)of;
  return KB_OK;
}

// sharded: route this shard's M records of out[cur], move the delivered ones to the shards holding their
// destinations' rows, and count them there.  *nrecv = records received; *any = some rank delivered a record
static int sp_exchange_wave(SpSim* S, uint32_t M, int cur, int32_t r, uint32_t w, uint32_t* nrecv, bool* any) {
  SpDev& d = S->d;
  const int W = S->world, me = S->rank;
  const uint32_t R = S->R;
  hipStream_t st = S->st;
  SpX& x = S->x;
  HIPCHK(hipMemsetAsync(x.xcnt, 0, 4ull * W * R, st));
  HIPCHK(hipMemsetAsync(x.xpay, 0, 4ull * W * R, st));
  { const int rc = sp_grow(S, &S->status, &S->status_cap, M); if (rc) return rc; }
  SpRoute rt;
  memset(&rt, 0, sizeof rt);
  rt.msgs = S->out[cur]; rt.M = M; rt.status = S->status; rt.pay = S->pool[cur];
  if (M) sp_launch(S, SPK_ROUTE, k_sp_route_x, (M + 255) / 256, 256, d, rt, x, r, w);
  {
    const uint32_t* in[2] = {x.xcnt, x.xpay};
    uint32_t* out[2] = {x.xoff, x.xpoff};
    sp_scan(S, (uint32_t)W * R, 2, in, out, 16);
  }
  sp_launch(S, SPK_ROUTE, k_sp_xbound, 1, 64, x, (const uint32_t*)S->scan_tot + 16);
  if (!S->xf->allgather_u32(x.xb, S->xall, 2 * W, st)) return sp_xfail(S);
  HIPCHK(hipMemcpyAsync(S->h_xall.data(), S->xall, 4ull * 2 * W * W, hipMemcpyDeviceToHost, st));
  HIPCHK(sp_sync(S));
  size_t sc[XMAX], sd[XMAX], rc[XMAX], rd[XMAX], psc[XMAX], psd[XMAX], prc[XMAX], prd[XMAX];
  size_t so = 0, pso = 0, ro = 0, pro = 0;
  uint64_t total = 0;
  for (int k = 0; k < W * W; ++k) total += S->h_xall[(size_t)(k / W) * 2 * W + (k % W)];
  *any = total != 0;
  *nrecv = 0;
  if (!*any) return KB_OK;
  for (int k = 0; k < W; ++k) {
    sc[k] = S->h_xall[(size_t)me * 2 * W + k]; psc[k] = S->h_xall[(size_t)me * 2 * W + W + k];
    rc[k] = S->h_xall[(size_t)k * 2 * W + me]; prc[k] = S->h_xall[(size_t)k * 2 * W + W + me];
    sd[k] = so; so += sc[k]; psd[k] = pso; pso += psc[k];
    rd[k] = ro; ro += rc[k]; prd[k] = pro; pro += prc[k];
  }
  { const int rc2 = sp_grow(S, &x.smsg, &S->smsg_cap, so); if (rc2) return rc2; }
  { const int rc2 = sp_grow(S, &x.spay, &S->spay_cap, pso); if (rc2) return rc2; }
  { const int rc2 = sp_grow(S, &S->rmsg, &S->rmsg_cap, ro); if (rc2) return rc2; }
  { const int rc2 = sp_grow(S, &S->rpay, &S->rpay_cap, pro); if (rc2) return rc2; }
  { const int rc2 = sp_grow(S, &S->rstat, &S->rstat_cap, ro); if (rc2) return rc2; }
  if (M) sp_launch(S, SPK_ROUTE, k_sp_pack, (R + 255) / 256, 256, d, x, (const Msg*)S->out[cur], (const uint8_t*)S->status,
                   (const uint32_t*)S->pool[cur], (const uint32_t*)S->ooff, (const uint32_t*)S->en);
  { const int rc2 = sp_a2a2(S, x.smsg, sc, sd, S->rmsg, rc, rd, sizeof(Msg), x.spay, psc, psd, S->rpay, prc, prd, 4); if (rc2) return rc2; }
  SpRecvBlocks rb;
  memset(&rb, 0, sizeof rb);
  for (int k = 0; k < W; ++k) rb.p0[k] = (uint32_t)prd[k];
  SpRoute rr;
  memset(&rr, 0, sizeof rr);
  rr.msgs = S->rmsg; rr.M = (uint32_t)ro; rr.status = S->rstat; rr.pay = S->rpay;
  rr.icnt = S->icnt; rr.ebound = S->ebound; rr.kprc = S->kprc;
  if (ro) sp_launch(S, SPK_ROUTE, k_sp_recv, (uint32_t)((ro + 255) / 256), 256, rr, x, rb);
  *nrecv = (uint32_t)ro;
  return KB_OK;
}

static int sp_step_round(SpSim* S) {
  SpDev& d = S->d;
  const int32_t r = S->round;
  const uint32_t C = S->C, R = S->R, tb = 256, g = (R + tb - 1) / tb, gc = (C + tb - 1) / tb;
  const bool sh = S->xf != nullptr;
  hipStream_t st = S->st;
  hipEvent_t er[2] = {nullptr, nullptr};
  if (S->prof_level > 0) {
    for (int k = 0; k < 2; ++k) {
      if (!S->ev_free.empty()) { er[k] = S->ev_free.back(); S->ev_free.pop_back(); }
      else (void)hipEventCreate(&er[k]);
    }
    (void)hipEventRecord(er[0], st);
  }
  // 0. stamp window
  if (r > 0 && r % EPOCH == 0) sp_launch(S, SPK_REBASE, k_sp_rebase, g, tb, d);
  // 1. lifecycle: API events in call order (a restart moves the map to its fresh address), then churn; every
  // shard replays them over all ids (the per-id facts are replicated), rows change on the shard holding them
  { const int rc = sp_apply_events(S, r); if (rc) return rc; }
  if ((S->cfg.fault_end_round < 0 || r < S->cfg.fault_end_round) && S->cfg.churn_threshold) {
    sp_launch(S, SPK_CHURN, k_sp_churn_leave, gc, tb, d, r);
    sp_launch(S, SPK_CHURN, k_sp_churn_join, 1, 1, d, r);
  }
  // 2. broadcasts of round r-1 (Failed, Join with the external peers' Joins), and the Probes queued since the last round
  if (!S->inj_join.empty()) {
    const int rc = merge_ext_joins(S->st, S->bjoin, &S->nj, S->inj_join, S->cfg.partition_groups, C);
    if (rc) return rc;
  }
  uint32_t np = 0;
  { const int rc = round_take_probes(S, R, &np); if (rc) return rc; }
  SpBc bc;
  memset(&bc, 0, sizeof bc);
  bc.bfail = S->bfail; bc.nf = S->nf; bc.bjoin = S->bjoin; bc.nj = S->nj; bc.JW = (S->nj + 31) / 32;
  if (bc.JW) {
    const size_t words = (size_t)R * bc.JW;
    if (words > S->jw_cap) {
      int rc = KB_OK;
      size_t c1 = S->jw_cap, c2 = S->jw_cap;
      rc = sp_grow(S, &S->jnew, &c1, words);
      if (!rc) rc = sp_grow(S, &S->jresp, &c2, words);
      if (rc) return rc;
      S->jw_cap = std::min(c1, c2);
    }
    HIPCHK(hipMemsetAsync(S->jnew, 0, 4 * words, st));
    HIPCHK(hipMemsetAsync(S->jresp, 0, 4 * words, st));
  }
  bc.jnew = S->jnew; bc.jresp = S->jresp; bc.jr_n = S->jr_n; bc.jr_pay = S->jr_pay;
  bc.np = np; bc.presp = S->d_presp; bc.presp_n = S->d_presp_n; bc.presp_cap = (uint32_t)std::min<size_t>(S->presp_cap, 0xFFFFFFFFu);
  if (S->nf && S->cfg.failed_mode == KB_FAILED_SOCKET_FAITHFUL && (S->cfg.stat_flags & KB_STAT_NO_SF_FAILED_DROPS)) {
    bc.fcounted = 1;                                   // no state effect, and their drops are not counted
  } else if (S->nf && S->cfg.failed_mode == KB_FAILED_SOCKET_FAITHFUL && S->cfg.partition_groups <= 255) {
    sp_launch(S, SPK_BFAIL_SF, k_sp_bfail_sf, g, tb, d, (const uint4*)S->fkey, S->nf, r);
    bc.fcounted = 1;
  }
  sp_launch(S, SPK_BCAST, k_sp_bcast, g, tb, d, bc, r);
  // wave-0 regions: Join responses first, then the tick's emissions; the external peers' injected records (the
  // shard holding the external id's row injects them)
  sp_launch(S, SPK_BOUND0, k_sp_bound0, g, tb, d, (const uint32_t*)S->jr_n, S->ebound);
  std::vector<XRec> inj;
  for (const XRec& q : S->inj) if (q.sender >= S->lo && q.sender < S->hi) inj.push_back(q);
  const uint32_t ninj = (uint32_t)inj.size();
  if (ninj) {
    { const int rc = sp_grow(S, &S->d_inj, &S->d_inj_cap, ninj); if (rc) return rc; }
    { const int rc = sp_grow(S, &S->d_inj_ids, &S->d_inj_ids_cap, S->inj_ids.size() + 1); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(S->d_inj, inj.data(), sizeof(XRec) * ninj, hipMemcpyHostToDevice, st));
    if (!S->inj_ids.empty()) HIPCHK(hipMemcpyAsync(S->d_inj_ids, S->inj_ids.data(), 4 * S->inj_ids.size(), hipMemcpyHostToDevice, st));
    sp_launch(S, SPK_EVENTS, k_sp_inject_prep, 1, 1, d, (const XRec*)S->d_inj, ninj, S->ebound, S->jr_pay);
  }
  {
    const uint32_t* in[2] = {SL(S, S->ebound), SL(S, S->jr_pay)};
    uint32_t* out[2] = {SL(S, S->eoff), SL(S, S->poff)};
    sp_scan(S, R, 2, in, out, 0);
  }
  uint32_t tot[8];
  HIPCHK(hipMemcpyAsync(tot, S->scan_tot, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(sp_sync(S));
  { const int rc = sp_grow(S, &S->stage, &S->stage_cap, tot[0]); if (rc) return rc; }
  { const int rc = sp_grow(S, &S->pool[0], &S->pool_cap[0], tot[1]); if (rc) return rc; }
  if (S->n_ext) { const int rc = round_size_exports(S, tot[0], tot[1]); if (rc) return rc; }   // wave 0's totals + the later waves' allowance
  SpOut o0;
  o0.stage = S->stage; o0.eoff = S->eoff; o0.ecap = S->ebound; o0.pay = S->pool[0]; o0.poff = S->poff; o0.pcap = S->jr_pay;
  o0.en = S->en;
  if (S->nj) sp_launch(S, SPK_JRESP, k_sp_jresp, g, tb, d, bc, o0, r);
  // 3. tick, against the running set's fingerprint
  sp_launch(S, SPK_TRUEFP, k_sp_truefp_part, SP_TFP / 256, 256, d, S->tfpart);
  sp_launch(S, SPK_TRUEFP, k_sp_truefp_fin, 1, 64, d, (const uint2*)S->tfpart, S->tfp);
  sp_launch(S, SPK_TICK, k_sp_tick, g, tb, d, o0, (const uint32_t*)S->jr_n, S->bo, (const uint32_t*)S->tfp, r);
  if (ninj) sp_launch(S, SPK_EVENTS, k_sp_inject, 1, 1, d, o0, (const XRec*)S->d_inj, ninj, (const uint32_t*)S->d_inj_ids);
  S->inj.clear(); S->inj_ids.clear();
  {
    const uint32_t* in[3] = {SL(S, S->bo.bj), SL(S, S->bo.bnf), SL(S, S->en)};
    uint32_t* out[3] = {SL(S, S->joff), SL(S, S->foff), SL(S, S->ooff)};
    sp_scan(S, R, 3, in, out, 2);
  }
  sp_launch(S, SPK_BCAST_WRITE, k_sp_bcast_write, g, tb, d, S->bo, (const uint32_t*)S->joff, (const uint32_t*)S->foff,
            sh ? S->bjoin_loc : S->bjoin, sh ? S->bfail_loc : S->bfail);
  HIPCHK(hipMemcpyAsync(tot + 2, S->scan_tot + 2, 12, hipMemcpyDeviceToHost, st));
  HIPCHK(sp_sync(S));
  uint32_t nj_next = tot[2], nf_next = tot[3];
  uint32_t M = tot[4];
  if (sh) { const int rc = sp_gather_bcasts(S, tot[2], tot[3], &nj_next, &nf_next); if (rc) return rc; }
  if (nf_next) sp_launch(S, SPK_BCAST_WRITE, k_sp_fkey, (nf_next + 3 + 255) / 256, 256, (const BCast*)S->bfail, nf_next, S->fkey);
  { const int rc = sp_grow(S, &S->out[0], &S->out_cap[0], M); if (rc) return rc; }
  sp_launch(S, SPK_COMPACT, k_sp_compact, g, tb, d, o0, (const uint32_t*)S->ooff, S->out[0]);
  // 4. receive window: delivery waves (sharded: routed on the senders' shards, exchanged, handled on the receivers')
  int cur = 0;
  for (uint32_t w = 0; w < S->cfg.max_waves && (M || sh); ++w) {
    HIPCHK(hipMemsetAsync(SL(S, S->icnt), 0, 4ull * R, st));
    HIPCHK(hipMemsetAsync(SL(S, S->icur), 0, 4ull * R, st));
    HIPCHK(hipMemsetAsync(SL(S, S->ebound), 0, 4ull * R, st));
    HIPCHK(hipMemsetAsync(SL(S, S->kprc), 0, 4ull * R, st));
    SpRoute rt;
    memset(&rt, 0, sizeof rt);
    const Msg* in_msgs = S->out[cur];
    const uint32_t* in_pay = S->pool[cur];
    uint32_t nin = M;
    if (!sh) {
      { const int rc = sp_grow(S, &S->status, &S->status_cap, M); if (rc) return rc; }
      rt.msgs = S->out[cur]; rt.M = M; rt.status = S->status; rt.icnt = S->icnt; rt.ebound = S->ebound; rt.kprc = S->kprc;
      rt.pay = S->pool[cur];
      sp_launch(S, SPK_ROUTE, k_sp_route, (M + 255) / 256, 256, d, rt, r, w);
    } else {
      bool any = false;
      { const int rc = sp_exchange_wave(S, M, cur, r, w, &nin, &any); if (rc) return rc; }
      if (!any) { M = 0; break; }                      // no record delivered anywhere: every later wave is empty
      rt.msgs = S->rmsg; rt.M = nin; rt.status = S->rstat; rt.pay = S->rpay;
      in_msgs = S->rmsg; in_pay = S->rpay;
    }
    sp_launch(S, SPK_PAYBOUND, k_sp_paybound, g, tb, d, (const uint32_t*)S->kprc, (const uint32_t*)S->icnt, S->pb);
    {
      const uint32_t* in[3] = {SL(S, S->icnt), SL(S, S->ebound), SL(S, S->pb)};
      uint32_t* out[3] = {SL(S, S->ioff), SL(S, S->eoff), SL(S, S->poff)};
      sp_scan(S, R, 3, in, out, 8);
    }
    HIPCHK(hipMemcpyAsync(tot, S->scan_tot + 8, 12, hipMemcpyDeviceToHost, st));
    HIPCHK(sp_sync(S));
    { const int rc = sp_grow(S, &S->inbox, &S->inbox_cap, tot[0]); if (rc) return rc; }
    { const int rc = sp_grow(S, &S->stage, &S->stage_cap, tot[1]); if (rc) return rc; }
    { const int rc = sp_grow(S, &S->pool[cur ^ 1], &S->pool_cap[cur ^ 1], tot[2]); if (rc) return rc; }
    if (nin) sp_launch(S, SPK_SCATTER, k_sp_scatter, (nin + 255) / 256, 256, rt, (const uint32_t*)S->ioff, S->icur, S->inbox);
    SpWave v;
    v.in = in_msgs; v.pay_in = in_pay; v.inbox = S->inbox; v.ioff = S->ioff; v.icnt = S->icnt;
    SpOut o;
    o.stage = S->stage; o.eoff = S->eoff; o.ecap = S->ebound; o.pay = S->pool[cur ^ 1]; o.poff = S->poff; o.pcap = S->pb;
    o.en = S->en;
    sp_launch(S, SPK_HANDLE, k_sp_handle, g, tb, d, v, o, r);
    {
      const uint32_t* in[1] = {SL(S, S->en)};
      uint32_t* out[1] = {SL(S, S->ooff)};
      sp_scan(S, R, 1, in, out, 12);
    }
    HIPCHK(hipMemcpyAsync(tot, S->scan_tot + 12, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(sp_sync(S));
    M = tot[0];
    { const int rc = sp_grow(S, &S->out[cur ^ 1], &S->out_cap[cur ^ 1], M); if (rc) return rc; }
    sp_launch(S, SPK_COMPACT, k_sp_compact, g, tb, d, o, (const uint32_t*)S->ooff, S->out[cur ^ 1]);
    cur ^= 1;
  }
  if (M) sp_launch(S, SPK_WINDOW, k_sp_window, (M + 255) / 256, 256, d, (const Msg*)S->out[cur], M);   // missed the window
  sp_launch(S, SPK_ROUND_END, k_sp_round_end, 1, 1024, d, r);
  if (sh) {                                          // the mesh's agreement and running counts, and any rank's error
    if (!S->xf->allreduce_sum_u32(d.ctr + C_LASTAGREE, 2, st)) return sp_xfail(S);
    if (!S->xf->allreduce_max_u32(d.ctr + C_ERR, 1, st)) return sp_xfail(S);
  }
  sp_launch(S, SPK_ROUND_END, k_sp_round_conv, 1, 64, d, r);
  if (er[1] || S->prof_level > 0) {
    if (!er[1] && !S->ev_free.empty()) { er[1] = S->ev_free.back(); S->ev_free.pop_back(); }
    if (!er[1]) (void)hipEventCreate(&er[1]);
    (void)hipEventRecord(er[1], st);
    S->recs.push_back(SpSim::Rec{SPK_N, er[0], er[1]});
  }
  uint32_t err = 0;
  HIPCHK(hipMemcpyAsync(&err, d.ctr + C_ERR, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(sp_sync(S));
  if (S->prof_level > 0) sp_prof_resolve(S);
  S->nj = nj_next; S->nf = nf_next;
  S->bj_total += nj_next; S->bf_total += nf_next;
  { const int rc = round_drain_exports(S); if (rc) return rc; }
  { const int rc = round_drain_probes(S, np, r); if (rc) return rc; }
  S->round = r + 1;
  return sp_err_status(err);
}
static int sp_step(SpSim* S, uint32_t rounds) {
  (void)hipSetDevice(S->device);
  for (uint32_t k = 0; k < rounds; ++k) { const int rc = sp_step_round(S); if (rc) return rc; }
  return KB_OK;
}

// ---- inspection: a row materialised from base Δ x and its entries -----------------------------------
// row inspection is answered by the shard holding the row (KB_INVALID_ARGUMENT on the others)
static int sp_chk_row(SpSim* S, uint32_t node) {
  if (node < S->lo || node >= S->hi) { seterr("the node's row is held by another shard"); return KB_INVALID_ARGUMENT; }
  return KB_OK;
}
static int sp_entries(SpSim* S, uint32_t node, std::vector<uint32_t>& e, uint8_t* based) {
  { const int rc = sp_chk_row(S, node); if (rc) return rc; }
  uint32_t n = 0;
  HIPCHK(hipMemcpy(&n, S->d.ne + node, 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(based, S->d.based + node, 1, hipMemcpyDeviceToHost));
  e.resize(n);
  if (n) HIPCHK(hipMemcpy(e.data(), S->d.ent + (size_t)node * S->d.ESTR, 4ull * n, hipMemcpyDeviceToHost));
  return KB_OK;
}
static int read_row(SpSim* S, uint32_t node, std::vector<uint8_t>& rw) {   // canonical bytes (0 = not a member)
  std::vector<uint32_t> e;
  uint8_t based = 0;
  const int rc = sp_entries(S, node, e, &based);
  if (rc) return rc;
  rw.assign(S->C, 0);
  if (based) for (uint32_t j = 0; j < S->C; ++j) if ((S->h_bbits[j >> 5] >> (j & 31)) & 1u) rw[j] = ST_ANCIENT;
  for (uint32_t x : e) {
    const uint32_t j = x >> 9, b = x & 255u;
    const bool mem = (based && ((S->h_bbits[j >> 5] >> (j & 31)) & 1u)) != ((x & SP_XF) != 0);
    rw[j] = mem ? (uint8_t)(b ? b : ST_ANCIENT) : ST_UNKNOWN;
  }
  return KB_OK;
}
// ---- the control plane's hooks (kb_ctl.h) ---------------------------------------------------------------
static int mark_all_dirty(SpSim* S) {
  k_sp_mark_dirty<<<(S->R + 255) / 256, 256, 0, S->st>>>(S->d);
  HIPCHK(hipStreamSynchronize(S->st));
  return KB_OK;
}
static int export_alloc(SpSim* S) {
  S->d.xrec_cap = XREC_MIN; S->d.xids_cap = XIDS_MIN;   // grown per round (round_size_exports)
  HIPCHK(sp_alloc(S, &S->d.xrec, S->d.xrec_cap)); HIPCHK(sp_alloc(S, &S->d.xids, S->d.xids_cap));
  return KB_OK;
}
static void window_stale(SpSim*) {}                  // no captured receive window
static int lat_column(SpSim*, uint32_t, std::vector<uint16_t>&) { return KB_OK; }   // no latency table
static int row_fp(SpSim* S, uint32_t node, uint32_t* fp) {
  { const int rc = sp_chk_row(S, node); if (rc) return rc; }
  k_sp_fp_one<<<1, 64, 0, S->st>>>(S->d, node);
  HIPCHK(hipMemcpyAsync(fp, S->d.fp + node, 4, hipMemcpyDeviceToHost, S->st));
  HIPCHK(hipStreamSynchronize(S->st));
  return KB_OK;
}
// the census frame's hooks (kb_ctl.h)
static hipStream_t eng_stream(SpSim* S) { return S->st; }
static const uint32_t* eng_fp(SpSim* S) { return S->d.fp; }
static const uint8_t* eng_alive(SpSim* S) { return S->d.alive; }
static int eng_refresh_fps(SpSim* S) {
  if (S->R) k_sp_fp_all<<<(S->R + 255) / 256, 256, 0, S->st>>>(S->d);
  HIPCHK(hipGetLastError());
  return KB_OK;
}
// all ids; 0 for non-running ids and for rows held by other shards
static int eng_fingerprints(SpSim* S, uint32_t* fps) {
  k_sp_fp_all<<<(S->R + 255) / 256, 256, 0, S->st>>>(S->d);
  std::vector<uint8_t> al(S->C);
  memset(fps, 0, 4ull * S->C);
  HIPCHK(hipMemcpyAsync(fps + S->lo, S->d.fp + S->lo, 4ull * S->R, hipMemcpyDeviceToHost, S->st));
  HIPCHK(hipMemcpyAsync(al.data(), S->d.alive, S->C, hipMemcpyDeviceToHost, S->st));
  HIPCHK(hipStreamSynchronize(S->st));
  for (uint32_t i = 0; i < S->C; ++i) if (!al[i]) fps[i] = 0;
  return KB_OK;
}
static int eng_true_fingerprint(SpSim* S, uint32_t* fp) {
  k_sp_truefp_part<<<SP_TFP / 256, 256, 0, S->st>>>(S->d, S->tfpart);
  k_sp_truefp_fin<<<1, 64, 0, S->st>>>(S->d, (const uint2*)S->tfpart, S->tfp);
  HIPCHK(hipMemcpyAsync(fp, S->tfp, 4, hipMemcpyDeviceToHost, S->st));
  HIPCHK(hipStreamSynchronize(S->st));
  return KB_OK;
}
static int eng_watch(SpSim* S, uint32_t node) {
  { const int rc = sp_chk_row(S, node); if (rc) return rc; }
  for (uint32_t w : S->watch_node) if (w == node) return KB_OK;
  S->watch_node.push_back(node); S->watch_fp.push_back(0); S->watch_snap.emplace_back(S->C, 0);   // attached empty
  return KB_OK;
}
static int eng_events(SpSim* S, uint32_t node, uint32_t* discovered, size_t cap_d, size_t* n_d, uint32_t* departed, size_t cap_p,
                     size_t* n_p, uint32_t* fp, int* fp_changed) {
  size_t k = 0;
  while (k < S->watch_node.size() && S->watch_node[k] != node) ++k;
  if (k == S->watch_node.size()) { seterr("node is not watched (kb_sim_watch)"); return KB_INVALID_OPERATION; }
  std::vector<uint8_t> rw;
  { const int rc = read_row(S, node, rw); if (rc) return rc; }
  { const int rc = row_fp(S, node, fp); if (rc) return rc; }
  std::vector<uint8_t>& snap = S->watch_snap[k];
  size_t a = 0, rm = 0, known = 0;
  for (uint32_t j = 0; j < S->C; ++j) {
    const bool now = rw[j] != 0, then = snap[j] != 0;
    known += now; a += now && !then; rm += then && !now;
  }
  *n_d = a; *n_p = rm;
  *fp_changed = known > 0 && *fp != S->watch_fp[k];
  const bool fit = (!a || (discovered && cap_d >= a)) && (!rm || (departed && cap_p >= rm));
  if (!fit) {
    if (discovered || departed) { seterr("event buffer too small"); return KB_CAPACITY; }
    return KB_OK;
  }
  a = rm = 0;
  for (uint32_t j = 0; j < S->C; ++j) {
    const bool now = rw[j] != 0, then = snap[j] != 0;
    if (now && !then) discovered[a++] = j;
    if (then && !now) departed[rm++] = j;
    snap[j] = (uint8_t)now;
  }
  if (*fp_changed) S->watch_fp[k] = *fp;
  return KB_OK;
}
static int fold_stats(SpSim* S) {
  (void)hipSetDevice(S->device);
  k_sp_stats_fold<<<NSTAT, 256, 0, S->st>>>(S->d);
  HIPCHK(hipStreamSynchronize(S->st));
  return KB_OK;
}
// kb_sim_kernel_time kinds: the whole round; the tick (KB_KT_ROWPASS's place: the per-row pass of the round);
// the in-order handlers (KB_KT_PROC)
static int eng_kernel_time(SpSim* S, int kind, double* ms, uint64_t* launches) {
  (void)hipStreamSynchronize(S->st);
  sp_prof_resolve(S);
  const int k = kind == KB_KT_ROUND ? SPK_N : kind == KB_KT_ROWPASS ? SPK_TICK : kind == KB_KT_PROC ? SPK_HANDLE : -1;
  if (k < 0) return KB_INVALID_ARGUMENT;
  if (k == SPK_N) { *ms = S->round_ms; *launches = S->round_n; }
  else { *ms = S->k_ms[k]; *launches = S->k_n[k]; }
  return KB_OK;
}
static int eng_reset_kernel_time(SpSim* S) {
  (void)hipStreamSynchronize(S->st);
  sp_prof_resolve(S);
  S->round_ms = 0; S->round_n = 0;
  memset(S->k_ms, 0, sizeof S->k_ms); memset(S->k_n, 0, sizeof S->k_n);
  return KB_OK;
}
static int eng_kernel_breakdown(SpSim* S, kb_kernel_time* out, size_t cap, size_t* n) {
  (void)hipStreamSynchronize(S->st);
  sp_prof_resolve(S);
  size_t c = 0;
  for (int k = 0; k < SPK_N; ++k) {
    if (!S->k_n[k]) continue;
    if (out && c < cap) {
      kb_kernel_time& o = out[c];
      memset(&o, 0, sizeof o);
      snprintf(o.name, sizeof o.name, "%s", SPK_NAME[k]);
      o.ms = S->k_ms[k]; o.launches = S->k_n[k];
    }
    c++;
  }
  *n = c;
  return (out && cap < c) ? KB_CAPACITY : KB_OK;
}
// the sparse layout's footprint (test surface): [rows based, exceptions, explicit stamps, entries of the
// largest row, bytes (4 per entry), rows], the oracle's kbo_sparse_footprint in this layout
static int eng_footprint(SpSim* S, uint64_t* out, size_t cap) {   // over the rows this handle holds
  if (cap < 6) return KB_INVALID_ARGUMENT;
  const uint32_t lo = S->lo, hi = S->hi, R = S->R;
  std::vector<uint32_t> ne(R);
  std::vector<uint8_t> based(R);
  HIPCHK(hipMemcpy(ne.data(), SL(S, S->d.ne), 4ull * R, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(based.data(), SL(S, S->d.based), R, hipMemcpyDeviceToHost));
  uint64_t nb = 0, tot = 0, mx = 0;
  for (uint32_t k = 0; k < R; ++k) { nb += based[k]; tot += ne[k]; mx = std::max<uint64_t>(mx, ne[k]); }
  out[0] = nb; out[1] = 0; out[2] = 0; out[3] = mx; out[4] = 4 * tot; out[5] = R;
  // exceptions / explicit stamps: counted exactly on the host in chunks
  const size_t chunk = std::max<size_t>(1, (size_t)(256u << 20) / (4ull * S->d.ESTR));
  std::vector<uint32_t> buf;
  for (uint32_t i0 = lo; i0 < hi; i0 += (uint32_t)chunk) {
    const uint32_t i1 = (uint32_t)std::min<size_t>(hi, i0 + chunk);
    buf.resize((size_t)(i1 - i0) * S->d.ESTR);
    HIPCHK(hipMemcpy(buf.data(), S->d.ent + (size_t)i0 * S->d.ESTR, 4ull * buf.size(), hipMemcpyDeviceToHost));
    for (uint32_t i = i0; i < i1; ++i)
      for (uint32_t q = 0; q < ne[i - lo]; ++q) {
        const uint32_t x = buf[(size_t)(i - i0) * S->d.ESTR + q];
        out[1] += (x & SP_XF) != 0; out[2] += (x & 255u) != 0;
      }
  }
  return KB_OK;
}

}  // namespace kb
