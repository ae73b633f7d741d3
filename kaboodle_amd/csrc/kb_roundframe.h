// kb_roundframe.h — the host steps of a round that both engines take (DESIGN.md "Host control plane", Round frame),
// written once.  E is the engine: kb_sim as a dense shard, or SpSim.  The templates read the fields both structs name
// alike (allocs, st, events / d_events / events_cap, probe_q / probes / presp / d_presp / d_presp_n / presp_cap,
// n_ext / xq / xq_ids, h_ident / h_idlen; d.ctr, d.xrec / d.xids and their capacities).  What differs sits behind
// hooks overloaded on the engine pointer, each defined next to its engine:
//   eng_alloc(e, &p, n)           n zeroed elements, tracked in e->allocs, the zeroing complete on return (talloc / sp_alloc)
//   eng_alloc_what(e)             the head of the engine's allocation-failure message
//   window_stale(e)               a captured receive window holds the old buffers (kb_ctl.h's hook)
// The engines keep what really differs: a restart's row move and the observers (device snapshots / host vectors), the
// sparse engine's filter of injected records by shard, the wave loops, and the error tables (err_status and
// sp_err_status number their codes differently).
// Included by kb_sim.hip after kb_sim and its allocator, before kb_sparse_host.h.
#pragma once

static void window_stale(kb_sim* s);
namespace kb { static void window_stale(SpSim* S); }

// The one growth routine of a handle's dynamic device buffers (contents are not kept).  A buffer that holds `need`
// elements stays.  Otherwise the old block is released through e->allocs and pointer and capacity are cleared BEFORE
// the allocation, so a failure leaves {nullptr, 0}: nothing dangles, and the next call allocates again.  The capacity
// is set on success only.  The slack is the call site's: `need` is the size allocated.  Every block is in e->allocs,
// which is all the handle's destruction walks.
template <class E, class T> static int eng_grow(E* e, T** p, size_t* cap, size_t need) {
  if (*p && need <= *cap) return KB_OK;
  if (*p) {
    const auto at = std::find(e->allocs.begin(), e->allocs.end(), (void*)*p);
    if (at != e->allocs.end()) e->allocs.erase(at);
    (void)hipFree(*p);
  }
  *p = nullptr; *cap = 0;
  const hipError_t err = eng_alloc(e, p, need);
  if (err != hipSuccess) { *p = nullptr; seterr(std::string(eng_alloc_what(e)) + hipGetErrorString(err)); return KB_CAPACITY; }
  *cap = need;
  return KB_OK;
}
// a capacity a kernel reads (32 bits; the call site keeps `need` below 2^32)
template <class E, class T> static int eng_grow(E* e, T** p, uint32_t* cap, size_t need) {
  size_t c = *cap;
  const int rc = eng_grow(e, p, &c, need);
  *cap = (uint32_t)c;
  return rc;
}
// Several buffers under one capacity: each re-allocated at n elements.  The capacity is zero from the first release
// on and becomes `value` (what the kernels are told; n may add a reserve to it) only when every one succeeded, so
// after a failure the next call regrows the whole group.
template <class E, class C, class... T> static int eng_grow_group(E* e, C* cap, size_t value, size_t n, T**... p) {
  *cap = 0;
  int rc = KB_OK;
  size_t c;
  ((rc = rc ? rc : (c = 0, eng_grow(e, p, &c, n))), ...);
  if (!rc) *cap = (C)value;
  return rc;
}

// the round's lifecycle events on the device, in call order (the engine launches over them)
template <class E> static int round_upload_events(E* e) {
  const size_t n = e->events.size();
  if (n > e->events_cap) { const int rc = eng_grow(e, &e->d_events, &e->events_cap, 2 * n); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(e->d_events, e->events.data(), sizeof(Event) * n, hipMemcpyHostToDevice, e->st));
  return KB_OK;
}

// The Probes queued since the last round travel with this round's broadcasts: *np of them, with room for a response
// of each of the R rows to each (presp_cap, the bound the kernel is given, is at least np * R: grown to exactly that,
// and kept from a larger round) and the counter at zero.
template <class E> static int round_take_probes(E* e, uint32_t R, uint32_t* np) {
  e->probes.swap(e->probe_q);
  e->probe_q.clear();
  *np = (uint32_t)e->probes.size();
  if (!*np) return KB_OK;
  { const int rc = eng_grow(e, &e->d_presp, &e->presp_cap, (size_t)*np * R); if (rc) return rc; }
  if (!e->d_presp_n) { size_t one = 0; const int rc = eng_grow(e, &e->d_presp_n, &one, 1); if (rc) return rc; }
  HIPCHK(hipMemsetAsync(e->d_presp_n, 0, 4, e->st));
  return KB_OK;
}

// External peers' export buffers hold every record a round routes to them.  A real instance's Join
// (kb_sim_inject KB_WIRE_JOIN) draws KnownPeers responses from ~1 % of the running peers, capj ids each
// (src/kaboodle.rs:284-304, :356-392): so before the window the buffers grow to the wave-0 totals (all Join
// responses and injected payloads, an upper bound of what wave 0 can export) plus a fixed allowance for the
// later waves' replies.  They are empty at a round's start (drained after every round), so nothing is copied.
constexpr uint32_t XREC_MIN = 1u << 16, XIDS_MIN = 1u << 22;
template <class E> static int round_size_exports(E* e, uint64_t recs, uint64_t ids) {
  const uint64_t nr = recs + XREC_MIN, ni = ids + XIDS_MIN, lim = 0xFFFFFFFFull;
  if (nr > lim || ni > lim) { seterr("export buffer beyond 2^32 entries"); return KB_CAPACITY; }
  if (nr > e->d.xrec_cap) { const int rc = eng_grow(e, &e->d.xrec, &e->d.xrec_cap, (size_t)std::min(nr + nr / 4, lim)); window_stale(e); if (rc) return rc; }
  if (ni > e->d.xids_cap) { const int rc = eng_grow(e, &e->d.xids, &e->d.xids_cap, (size_t)std::min(ni + ni / 4, lim)); window_stale(e); if (rc) return rc; }
  return KB_OK;
}

// the exported records in (wave, sender, seq) order: what a mesh of one shard and of several hand out alike
static void xrec_order(std::vector<XRec>& v) {
  std::sort(v.begin(), v.end(), [](const XRec& a, const XRec& b) {
    return a.wave != b.wave ? a.wave < b.wave : a.sender != b.sender ? a.sender < b.sender : a.seq < b.seq; });
}
// ... appended to the host queue, their payload offsets rebased onto the queue's ids (`base` ids were there before)
static void xrec_enqueue(const std::vector<XRec>& v, size_t base, std::vector<kb_unicast>& xq) {
  for (const XRec& x : v) {
    kb_unicast u;
    memcpy(&u, &x, sizeof u);
    u.pay_off = (uint32_t)(base + x.pay_off);
    xq.push_back(u);
  }
}
// the round's records to external peers, to the host queue (kb_sim_exported); the device's buffers are empty again
template <class E> static int round_drain_exports(E* e) {
  if (!e->n_ext) return KB_OK;
  uint32_t c[2];
  HIPCHK(hipMemcpy(c, e->d.ctr + C_XREC, 8, hipMemcpyDeviceToHost));
  const uint32_t nrec = std::min(c[0], e->d.xrec_cap), nid = std::min(c[1], e->d.xids_cap);
  std::vector<XRec> v(nrec);
  const size_t base = e->xq_ids.size();
  e->xq_ids.resize(base + nid);
  if (nrec) HIPCHK(hipMemcpy(v.data(), e->d.xrec, sizeof(XRec) * nrec, hipMemcpyDeviceToHost));
  if (nid) HIPCHK(hipMemcpy(e->xq_ids.data() + base, e->d.xids, 4ull * nid, hipMemcpyDeviceToHost));
  xrec_order(v);
  xrec_enqueue(v, base, e->xq);
  const uint32_t z[2] = {0, 0};
  HIPCHK(hipMemcpy(e->d.ctr + C_XREC, z, 8, hipMemcpyHostToDevice));
  return KB_OK;
}

// the ProbeResponses in (responder, probe) order
static void presp_order(std::vector<uint2>& v) {
  std::sort(v.begin(), v.end(), [](const uint2& a, const uint2& b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
}
// the round's ProbeResponses, with the responders' identities, to the host queue (kb_sim_probe_responses)
template <class E> static int round_drain_probes(E* e, uint32_t np, int32_t r) {
  if (!np) return KB_OK;
  uint32_t k = 0;
  HIPCHK(hipMemcpy(&k, e->d_presp_n, 4, hipMemcpyDeviceToHost));
  k = (uint32_t)std::min<size_t>(k, e->presp_cap);
  std::vector<uint2> v(k);
  if (k) HIPCHK(hipMemcpy(v.data(), e->d_presp, sizeof(uint2) * k, hipMemcpyDeviceToHost));
  presp_order(v);
  for (const uint2& q : v) {
    kb_probe_response o;
    memset(&o, 0, sizeof o);
    o.responder = q.x; o.probe = q.y; o.round = r; o.prober = e->probes[q.y];
    o.identity_len = e->h_idlen[q.x];
    memcpy(o.identity, &e->h_ident[(size_t)q.x * MAXID], o.identity_len);
    e->presp.push_back(o);
  }
  return KB_OK;
}
