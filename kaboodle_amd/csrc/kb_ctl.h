// kb_ctl.h — the host control plane of the C ABI (DESIGN.md "Host control plane"), written once for both engines.
// E is the engine: kb_sim as a dense shard, or SpSim.  The templates read the host state and the device tables
// that both structs name alike (events, h_ident .. inj, xq; d.alive, d.ctr, d.paq, d.susp, d.cur ..).  What differs
// sits behind hooks overloaded on the engine pointer, each defined next to its engine:
//   upload_segments(e)            per-id segment CRCs after an identity change
//   mark_all_dirty(e)             every row's fingerprint is stale
//   export_alloc(e)               the first allocation of the export buffers
//   window_stale(e)               a captured receive window holds the old buffers (dense; nothing for sparse rows)
//   read_row(e, node, rw)         a row as canonical bytes (0 = not a member)
//   row_fp(e, node, fp)           one row's fingerprint
//   lat_column(e, node, lat)      the latency column (dense with track_latency; else left empty)
//   fold_stats(e)                 the per-workgroup partial counters folded into d.stats
//   eng_stream(e)                 the engine's stream (the census frame, kb_censusframe.h, and the three below)
//   eng_fp(e), eng_alive(e)       the device's fingerprints and running flags, per id
//   eng_refresh_fps(e)            the launch that refolds the rows whose fingerprint is stale
// Included by kb_sim.hip after both engines, before the API surface.
#pragma once

// row inspection is answered by the shard holding the row (KB_INVALID_ARGUMENT on the others)
template <class E> static int ctl_chk_row(E* e, uint32_t node) {
  if (node < e->lo || node >= e->hi) { seterr("the node's row is held by another shard"); return KB_INVALID_ARGUMENT; }
  return KB_OK;
}
// the device's alive (not the queue)
template <class E> static int ctl_is_running(E* e, uint32_t node, int* running) {
  uint8_t a = 0;
  HIPCHK(hipMemcpy(&a, e->d.alive + node, 1, hipMemcpyDeviceToHost));
  *running = a;
  return KB_OK;
}
// running as the API sees it: the last lifecycle call queued for the node since the last step (they take
// effect at the next round start), else its current state; a queued restart moves the instance away
template <class E> static int ctl_running(E* e, uint32_t node, int* run) {
  for (size_t k = e->events.size(); k-- > 0;) {
    if (e->events[k].node == node) { *run = e->events[k].kind != EV_STOP; return KB_OK; }
    if (e->events[k].kind == EV_RESTART && e->events[k].src == node) { *run = 0; return KB_OK; }
  }
  return ctl_is_running(e, node, run);
}
// the address has been bound by an instance: it ran (start_round, replicated), or a start of it is queued
template <class E> static int ctl_ever_bound(E* e, uint32_t node, int* ever) {
  for (const Event& ev : e->events) if (ev.node == node && ev.kind != EV_STOP) { *ever = 1; return KB_OK; }
  int32_t sr = 0;
  HIPCHK(hipMemcpy(&sr, e->d.start_round + node, 4, hipMemcpyDeviceToHost));
  *ever = sr != NONE_ROUND;
  return KB_OK;
}
template <class E> static int ctl_facts(E* e, uint32_t node, int* run, int* ever) {
  const int rc = ctl_running(e, node, run);
  return rc ? rc : ctl_ever_bound(e, node, ever);
}
template <class E> static int ctl_start_node(E* e, uint32_t node) {
  int run = 0, ever = 0;
  { const int rc = ctl_facts(e, node, &run, &ever); if (rc) return rc; }
  if (!run && ever) { seterr("a stopped instance restarts at a fresh address (kb_sim_restart_node)"); return KB_INVALID_OPERATION; }
  e->events.push_back(Event{node, EV_START, node, 0});
  return KB_OK;
}
template <class E> static int ctl_stop_node(E* e, uint32_t node) { e->events.push_back(Event{node, EV_STOP, node, 0}); return KB_OK; }
// Kaboodle::start of the instance at `node` (include/kaboodle_sim.h): a stopped instance that ran comes
// back at the next fresh id, allocated now (the churn reserve's counter, replicated on every shard)
template <class E> static int ctl_restart_node(E* e, uint32_t node, uint32_t* new_node) {
  if (e->h_moved[node]) { seterr("the instance bound here restarted at a fresh address"); return KB_INVALID_OPERATION; }
  int run = 0, ever = 0;
  { const int rc = ctl_facts(e, node, &run, &ever); if (rc) return rc; }
  if (run) { *new_node = node; return KB_OK; }
  if (!ever) { *new_node = node; e->events.push_back(Event{node, EV_START, node, 0}); return KB_OK; }
  uint32_t to = 0;
  HIPCHK(hipMemcpy(&to, e->d.ctr + C_NEXTFREE, 4, hipMemcpyDeviceToHost));
  for (; to < e->C; ++to) {                          // the next fresh id: never bound, no identity set
    int ev = 0;
    const int rc = ctl_ever_bound(e, to, &ev);
    if (rc) return rc;
    if (!ev && !e->h_idset[to]) break;
  }
  if (to >= e->C) { seterr("no fresh address left for the restart (capacity)"); return KB_CAPACITY; }
  const int pl = e->h_pendlen[node];
  const uint8_t* src = pl >= 0 ? &e->h_pend[(size_t)node * MAXID] : &e->h_ident[(size_t)node * MAXID];
  const uint32_t len = pl >= 0 ? (uint32_t)pl : e->h_idlen[node];
  memmove(&e->h_ident[(size_t)to * MAXID], src, len);
  e->h_idlen[to] = (uint8_t)len;
  e->h_pendlen[node] = -1; e->h_pendlen[to] = -1;
  { const int rc = upload_segments(e); if (rc) return rc; }
  window_stale(e);                                   // (uniform)
  const uint32_t nf = to + 1;
  HIPCHK(hipMemcpy(e->d.ctr + C_NEXTFREE, &nf, 4, hipMemcpyHostToDevice));
  e->events.push_back(Event{to, EV_RESTART, node, 0});
  e->h_moved[node] = 1;
  *new_node = to;
  return KB_OK;
}
// validated on every shard, queued by the one holding the row
template <class E> static int ctl_ping_addrs(E* e, uint32_t node, const uint32_t* peers, size_t n) {
  for (size_t k = 0; k < n; ++k) if (peers[k] >= e->C) return KB_INVALID_ARGUMENT;
  int run = 0;
  { const int rc = ctl_is_running(e, node, &run); if (rc) return rc; }
  if (!run) { seterr("Cannot ping while we are not started"); return KB_INVALID_OPERATION; }
  if (node < e->lo || node >= e->hi) return KB_OK;
  uint32_t qn = 0;
  HIPCHK(hipMemcpy(&qn, e->d.paq_n + node, 4, hipMemcpyDeviceToHost));
  std::vector<uint32_t> q(PAQ);
  HIPCHK(hipMemcpy(q.data(), e->d.paq + (size_t)node * PAQ, 4 * PAQ, hipMemcpyDeviceToHost));
  std::vector<uint8_t> rw;
  { const int rc = read_row(e, node, rw); if (rc) return rc; }
  for (size_t k = 0; k < n; ++k) {
    if (rw[peers[k]]) continue;                      // already known: skipped (src/lib.rs:277-282)
    if (qn == PAQ) { seterr("ping_addrs queue full"); return KB_CAPACITY; }
    q[qn++] = peers[k];
  }
  HIPCHK(hipMemcpy(e->d.paq + (size_t)node * PAQ, q.data(), 4 * PAQ, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->d.paq_n + node, &qn, 4, hipMemcpyHostToDevice));
  return KB_OK;
}
template <class E> static int ctl_set_identity(E* e, uint32_t node, const uint8_t* identity, size_t len) {
  if (e->h_moved[node]) { seterr("the instance bound here restarted at a fresh address"); return KB_INVALID_OPERATION; }
  int run = 0, ever = 0;
  { const int rc = ctl_facts(e, node, &run, &ever); if (rc) return rc; }
  if (run) { seterr("Cannot change identity while the mesh is running; call .stop first"); return KB_INVALID_OPERATION; }
  if (len != e->cfg.id_len && e->C > 200) { seterr("non-uniform identity length needs capacity <= 200"); return KB_INVALID_ARGUMENT; }
  if (ever) {                                      // views keep what the address announced; the instance's
    memcpy(&e->h_pend[(size_t)node * MAXID], identity, len);   // next address takes the new bytes
    e->h_pendlen[node] = (int16_t)len;
    return KB_OK;
  }
  memcpy(&e->h_ident[(size_t)node * MAXID], identity, len);
  e->h_idlen[node] = (uint8_t)len;
  e->h_idset[node] = 1;                            // no longer a fresh id for churn joins and restarts
  { const uint8_t one = 1; HIPCHK(hipMemcpy(e->d.idset + node, &one, 1, hipMemcpyHostToDevice)); }
  { const int rc = upload_segments(e); if (rc) return rc; }
  window_stale(e);                                 // (uniform, L)
  return mark_all_dirty(e);
}
template <class E> static int ctl_identity(E* e, uint32_t node, uint8_t* buf, size_t cap, size_t* len) {
  *len = e->h_idlen[node];
  if (!buf) return KB_OK;
  if (cap < *len) return KB_CAPACITY;
  memcpy(buf, &e->h_ident[(size_t)node * MAXID], *len);
  return KB_OK;
}
// the last round's Join / Failed broadcasts (whole mesh; sender order, a node's Join before its Failed)
template <class E> static int ctl_broadcasts(E* e, kb_broadcast* out, size_t cap, size_t* n) {
  std::vector<BCast> j(e->nj), f(e->nf);
  if (e->nj) HIPCHK(hipMemcpy(j.data(), e->bjoin, sizeof(BCast) * e->nj, hipMemcpyDeviceToHost));
  if (e->nf) HIPCHK(hipMemcpy(f.data(), e->bfail, sizeof(BCast) * e->nf, hipMemcpyDeviceToHost));
  size_t c = 0, a = 0, b = 0;
  while (a < j.size() || b < f.size()) {
    const bool tj = b == f.size() || (a < j.size() && j[a].sender <= f[b].sender);
    if (out && c < cap) {
      kb_broadcast& o = out[c];
      memset(&o, 0, sizeof o);
      if (tj) { o.kind = KB_WIRE_JOIN; o.sender = j[a].sender; o.peer = j[a].peer; }
      else { o.kind = KB_WIRE_FAILED; o.sender = f[b].sender; o.peer = f[b].peer; }
    }
    if (tj) a++; else b++;
    c++;
  }
  *n = c;
  return (out && cap < c) ? KB_CAPACITY : KB_OK;
}
template <class E> static int ctl_peers(E* e, uint32_t node, uint32_t* peers, size_t cap, size_t* n) {
  std::vector<uint8_t> rw;
  { const int rc = ctl_chk_row(e, node); if (rc) return rc; }
  { const int rc = read_row(e, node, rw); if (rc) return rc; }
  size_t c = 0;
  for (uint32_t j = 0; j < e->C; ++j) if (rw[j]) { if (peers && c < cap) peers[c] = j; c++; }
  *n = c;
  return (peers && cap < c) ? KB_CAPACITY : KB_OK;
}
template <class E> static int ctl_peer_states(E* e, uint32_t node, kb_peer_state* out, size_t cap, size_t* n) {
  { const int rc = ctl_chk_row(e, node); if (rc) return rc; }
  std::vector<uint8_t> rw;
  { const int rc = read_row(e, node, rw); if (rc) return rc; }
  Susp sl[SLOTS];
  HIPCHK(hipMemcpy(sl, e->d.susp + (size_t)node * SLOTS, sizeof sl, hipMemcpyDeviceToHost));
  std::vector<uint16_t> lat;
  { const int rc = lat_column(e, node, lat); if (rc) return rc; }
  const int32_t E0 = epoch_base(e->round > 0 ? e->round - 1 : 0);
  size_t c = 0;
  for (uint32_t j = 0; j < e->C; ++j) {
    if (!rw[j]) continue;
    if (out && c < cap) {
      kb_peer_state& o = out[c];
      memset(&o, 0, sizeof o);
      o.peer = j;
      o.identity_len = e->h_idlen[j];
      memcpy(o.identity, &e->h_ident[(size_t)j * MAXID], e->h_idlen[j]);
      o.latency_ms = !lat.empty() && lat[j] != LAT_NONE ? lat[j] : KB_LATENCY_NONE;
      if (rw[j] == ST_SUSPECT) {
        const Susp* q = nullptr;
        for (auto& x : sl) if (x.kind && x.peer == j) q = &x;
        o.state = q && q->kind == SK_WFIP ? KB_STATE_WAITING_FOR_INDIRECT_PING : KB_STATE_WAITING_FOR_PING;
        o.since = q ? q->since : 0;
      } else {
        o.state = KB_STATE_KNOWN;
        o.since = rw[j] == ST_ANCIENT ? INT32_MIN : (int32_t)rw[j] + E0 - EOFF;
      }
    }
    c++;
  }
  *n = c;
  return (out && cap < c) ? KB_CAPACITY : KB_OK;
}
// this shard's counters (ranks of kb_sim_create_rank: summed over the mesh, a collective)
template <class E> static int ctl_read_stats(E* e, unsigned long long* st) {
  { const int rc = fold_stats(e); if (rc) return rc; }
  if (e->xf && !e->in_group) {
    HIPCHK(hipMemcpyAsync(e->xstats, e->d.stats, 8ull * NSTAT, hipMemcpyDeviceToDevice, e->st));
    if (!e->xf->allreduce_sum_u64(e->xstats, NSTAT, e->st)) { seterr(e->xf->error()); return KB_IO_ERROR; }
    HIPCHK(hipMemcpyAsync(st, e->xstats, 8ull * NSTAT, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    return KB_OK;
  }
  HIPCHK(hipMemcpy(st, e->d.stats, 8ull * NSTAT, hipMemcpyDeviceToHost));
  return KB_OK;
}
// kb_stats from the mesh's counters `st` and this shard's replicated facts
template <class E> static int ctl_stats_fill(E* e, const unsigned long long* st, kb_stats* out) {
  uint32_t ctr[NCTR];
  HIPCHK(hipMemcpy(ctr, e->d.ctr, sizeof ctr, hipMemcpyDeviceToHost));
  std::vector<uint8_t> al(e->C);
  HIPCHK(hipMemcpy(al.data(), e->d.alive, e->C, hipMemcpyDeviceToHost));
  memset(out, 0, sizeof *out);
  out->round = e->round;
  uint32_t a = 0;
  for (uint8_t x : al) a += x;
  out->alive = a;
  out->agree = ctr[C_LASTAGREE];
  out->first_converged_round = (int32_t)ctr[C_FIRSTCONV];
  out->last_converged_round = (int32_t)ctr[C_LASTCONV];
  out->next_free_id = ctr[C_NEXTFREE];
  out->sent_ping = st[S_PING]; out->sent_ping_req = st[S_PINGREQ]; out->sent_ack = st[S_ACK];
  out->sent_known_peers = st[S_KP]; out->sent_kpr = st[S_KPR];
  out->bcast_join = e->bj_total; out->bcast_failed = e->bf_total;
  out->drop_dead = st[S_DEAD]; out->drop_loss = st[S_LOSS]; out->drop_window = st[S_WINDOW];
  out->drop_oversize = st[S_OVERSIZE]; out->drop_partition = st[S_PART]; out->drop_bcast = st[S_BDROP];
  out->removed_timeout = st[S_RMTIMEOUT]; out->removed_failed = st[S_RMFAILED]; out->join_responses = st[S_JRESP];
  out->curious_overflow = st[S_CUROVF]; out->churn_leaves = st[S_CLEAVE]; out->churn_joins = st[S_CJOIN];
  out->sent_kp_ids = st[S_KPIDS];
  out->alive_rounds = st[S_ALIVER];
  out->probe_responses = st[S_PROBERESP];
  out->exported = st[S_EXPORT];
  return KB_OK;
}
// per id: alive, n, last_bcast, start_round; n and last_bcast only for the rows this engine holds
template <class E> static int ctl_dump_scalars(E* e, int32_t* out) {
  const uint32_t C = e->C, R = e->R;
  std::vector<uint8_t> al(C);
  std::vector<uint32_t> n(R);
  std::vector<int32_t> lb(R), sr(C);
  HIPCHK(hipMemcpy(al.data(), e->d.alive, C, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(n.data(), e->d.n + e->lo, 4ull * R, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(lb.data(), e->d.last_bcast + e->lo, 4ull * R, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(sr.data(), e->d.start_round, 4ull * C, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < C; ++i) {
    const bool loc = i >= e->lo && i < e->hi;
    out[4 * i] = al[i]; out[4 * i + 1] = loc ? (int32_t)n[i - e->lo] : 0;
    out[4 * i + 2] = loc ? lb[i - e->lo] : 0; out[4 * i + 3] = sr[i];
  }
  return KB_OK;
}
template <class E> static int ctl_dump_suspects(E* e, uint32_t node, int32_t* out, size_t cap, size_t* n) {
  { const int rc = ctl_chk_row(e, node); if (rc) return rc; }
  Susp sl[SLOTS];
  HIPCHK(hipMemcpy(sl, e->d.susp + (size_t)node * SLOTS, sizeof sl, hipMemcpyDeviceToHost));
  std::vector<std::array<int32_t, 3>> v;
  for (auto& x : sl) if (x.kind) v.push_back({(int32_t)x.peer, x.kind, x.since});
  std::sort(v.begin(), v.end());
  *n = v.size();
  if (out) { if (cap < 3 * v.size()) return KB_CAPACITY; for (size_t k = 0; k < v.size(); ++k) memcpy(out + 3 * k, v[k].data(), 12); }
  return KB_OK;
}
template <class E> static int ctl_dump_curious(E* e, uint32_t node, int32_t* out, size_t cap, size_t* n) {
  { const int rc = ctl_chk_row(e, node); if (rc) return rc; }
  Cur cu[CSLOTS];
  HIPCHK(hipMemcpy(cu, e->d.cur + (size_t)node * CSLOTS, sizeof cu, hipMemcpyDeviceToHost));
  std::vector<std::array<int32_t, 6>> v;
  for (auto& x : cu) if (x.used) {
    std::array<int32_t, 6> q{(int32_t)x.peer, (int32_t)x.nobs, -1, -1, -1, -1};
    for (uint32_t k = 0; k < x.nobs && k < NOBS; ++k) q[2 + k] = (int32_t)x.obs[k];
    v.push_back(q);
  }
  std::sort(v.begin(), v.end(), [](const std::array<int32_t, 6>& a, const std::array<int32_t, 6>& b) { return a[0] < b[0]; });
  *n = v.size();
  if (out) { if (cap < 6 * v.size()) return KB_CAPACITY; for (size_t k = 0; k < v.size(); ++k) memcpy(out + 6 * k, v[k].data(), 24); }
  return KB_OK;
}
// ---- external peers ------------------------------------------------------------------------
template <class E> static int ctl_set_external(E* e, uint32_t node) {
  if (e->h_ext.empty()) e->h_ext.assign(e->C, 0);
  if (e->h_ext[node]) return KB_OK;
  int ever = 0;
  { const int rc = ctl_ever_bound(e, node, &ever); if (rc) return rc; }
  if (ever) { seterr("an external peer takes an address no instance has bound"); return KB_INVALID_OPERATION; }
  e->h_ext[node] = 1; e->n_ext++;
  e->h_idset[node] = 1;                            // not a fresh id: churn joins and restarts skip it
  const uint8_t o = 1;
  HIPCHK(hipMemcpy(e->d.ext + node, &o, 1, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->d.idset + node, &o, 1, hipMemcpyHostToDevice));
  return e->d.xrec ? KB_OK : export_alloc(e);      // grown per round afterwards
}
template <class E> static int ctl_inject(E* e, const kb_unicast* m, const uint32_t* ids) {
  if (m->sender >= e->C || m->dest >= e->C || (m->kind > K_KPR && m->kind != KB_WIRE_JOIN) || (m->pay_len && !ids))
    return KB_INVALID_ARGUMENT;
  if (e->h_ext.empty() || !e->h_ext[m->sender]) { seterr("kb_sim_inject: the sender is not an external peer"); return KB_INVALID_OPERATION; }
  if (m->kind == KB_WIRE_JOIN) {                       // a Join broadcast: the next round's Join list
    if (std::find(e->inj_join.begin(), e->inj_join.end(), m->sender) != e->inj_join.end()) {
      seterr("kb_sim_inject: one Join per external peer per round"); return KB_CAPACITY;
    }
    e->inj_join.push_back(m->sender);
    return KB_OK;
  }
  if ((m->kind == K_PINGREQ || m->kind == K_ACK) && m->a >= e->C) return KB_INVALID_ARGUMENT;
  for (uint32_t k = 0; k < m->pay_len; ++k) if (ids[k] >= e->C) return KB_INVALID_ARGUMENT;
  uint32_t per = 0, rel = 0;
  for (const XRec& x : e->inj) if (x.sender == m->sender) { per++; if (x.kind == K_KP) rel += x.pay_len; }
  if (per >= (uint32_t)TICK_MAX) { seterr("kb_sim_inject: 33 records per external peer per round"); return KB_CAPACITY; }
  XRec x{0, 0, m->sender, m->dest, 0, m->kind, m->kind == K_KP ? 0u : m->a, m->fp, m->n, (uint32_t)e->inj_ids.size(),
         m->kind == K_KP ? m->pay_len : 0u, rel};
  if (m->kind == K_KP) e->inj_ids.insert(e->inj_ids.end(), ids, ids + m->pay_len);
  e->inj.push_back(x);
  return KB_OK;
}
