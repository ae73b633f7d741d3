// kb_rounddbg.h — the dense round's diagnostics (env KB_DEBUG_WAVES, with KB_DEV's bits choosing the device-side
// timers): the counter clears, the read-backs and the reports, each behind its own condition, so that step_round and
// launch_waves read as launches only.  Each is called at the point of the stream its numbers belong to; with
// KB_DEBUG_WAVES unset every one returns at its first line (no wait, no copy).  Included by kb_sim.hip before
// launch_waves, after RowPlan.
#pragma once

// ---- the receive window (launch_waves) -----------------------------------------------------------------------
// inbox sizes per wave
static int dbg_wave_inboxes(kb_sim* s, int32_t r, uint32_t w) {
  if (!s->debug_waves) return KB_OK;
  const uint32_t R = s->R;
  std::vector<uint32_t> c1(R);
  HIPCHK(hipMemcpyAsync(c1.data(), L(s, s->wc.cnt1), 4ull * R, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipStreamSynchronize(s->st));
  uint64_t sum = 0; uint32_t mx = 0, arg = 0, big = 0;
  for (uint32_t k = 0; k < R; ++k) { sum += c1[k]; if (c1[k] > mx) { mx = c1[k]; arg = s->lo + k; } big += c1[k] > 64; }
  fprintf(stderr, "[kb] round %d wave %u: in-order msgs %llu, max inbox %u (node %u), inboxes > 64: %u\n", r, w,
          (unsigned long long)sum, mx, arg, big);
  return KB_OK;
}
// the handlers' counters, cleared ahead of the wave's KnownPeers groups and handlers ...
static int dbg_proc_clear(kb_sim* s) {
  if (!s->debug_waves) return KB_OK;
  HIPCHK(hipMemsetAsync(s->d.ctr + C_DBG_INS, 0, 52, s->st));
  HIPCHK(hipMemsetAsync(s->d.ctr + C_DBG_SLOW_LONG, 0, 20, s->st));
  return KB_OK;
}
// ... and read back behind them
static int dbg_proc_report(kb_sim* s, int32_t r, uint32_t w) {
  if (!s->debug_waves) return KB_OK;
  const Dev& d = s->d;
  uint32_t dbg[13], slow = 0;
  HIPCHK(hipMemcpyAsync(dbg, d.ctr + C_DBG_INS, 52, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipMemcpyAsync(&slow, d.ctr + C_SLOW, 4, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipStreamSynchronize(s->st));
  fprintf(stderr, "[kb] round %d wave %u: k_proc nodes %u, prologue inserts %u, fingerprint refreshes %u (max per "
          "node %u), KPR scans %u (log entries %u), incremental bases %u\n", r, w, slow, dbg[0], dbg[1], dbg[2], dbg[3],
          dbg[4], dbg[5]);
  if (d.dev & 256) {
    uint32_t why[5];
    HIPCHK(hipMemcpy(why, d.ctr + C_DBG_SLOW_LONG, 20, hipMemcpyDeviceToHost));
    fprintf(stderr, "[kb] round %d wave %u: to k_proc because inbox > %u: %u, sender not a member: %u, fingerprint stale: %u, "
            "KPR not proven oversize: %u, other: %u\n", r, w, FAST_MAX, why[0], why[1], why[2], why[3], why[4]);
  }
  if (d.dev & 128)
    fprintf(stderr, "[kb] round %d wave %u: k_kp_group BIG workgroup-destinations %u, messages %u: stage+arms %.1f us, "
            "prologues %.1f, write-back+refold %.1f (sums), max total %.1f\n", r, w, dbg[10], dbg[12], dbg[6] * 0.01,
            dbg[8] * 0.01, dbg[9] * 0.01, dbg[7] * 0.01);
  if (d.dev & 64)
    fprintf(stderr, "[kb] round %d wave %u: k_proc node time sum %.1f us (max %.1f), take_base %.1f, insertions %.1f, "
            "start %.1f, end %.1f, messages %u\n", r, w, dbg[6] * 0.01, dbg[7] * 0.01, dbg[8] * 0.01, dbg[9] * 0.01,
            dbg[10] * 0.01, dbg[11] * 0.01, dbg[12]);
  return KB_OK;
}

// ---- the round (step_round's phases) -------------------------------------------------------------------------
// broadcast list shape, behind the Failed list's preparation
static int dbg_bcast_shape(kb_sim* s, int32_t r) {
  if (!s->debug_waves || !s->nf) return KB_OK;
  std::vector<uint8_t> dep(s->nf);
  HIPCHK(hipMemcpyAsync(dep.data(), s->bf_dep, s->nf, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipStreamSynchronize(s->st));
  size_t nd = 0;
  for (uint8_t x : dep) nd += x != 0;
  fprintf(stderr, "[kb] round %d broadcasts: Failed %u (sender named earlier: %zu), Join %u\n", r, s->nf, nd, s->nj);
  return KB_OK;
}
// KB_DEV=2048: the row pass's phases, summed over its waves
static bool dbg_rowpass_on(const kb_sim* s) { return s->debug_waves && (s->d.dev & 2048); }
static int dbg_rowpass_begin(kb_sim* s, int32_t r, const RowPlan& p) {
  if (s->debug_waves && r == 2)
    fprintf(stderr, "[kb] row pass: %u waves/workgroup, %zu B LDS, %u workgroups/CU (lds_per_cu %zu), %u workgroups\n", p.wpb,
            p.lds, p.per_cu, (size_t)s->lds_per_cu, p.blocks);
  if (dbg_rowpass_on(s)) HIPCHK(hipMemsetAsync(s->d.ctr + C_DBG_TNODE, 0, 4 * (C_DBG_MSGS - C_DBG_TNODE), s->st));
  return KB_OK;
}
static int dbg_rowpass_shares(kb_sim* s, int32_t r, const RowPlan& p) {
  if (!dbg_rowpass_on(s)) return KB_OK;
  const uint32_t blocks = p.blocks, wpb = p.wpb;
  uint32_t t[13];
  HIPCHK(hipMemcpy(t, s->d.ctr + C_DBG_INS, 52, hipMemcpyDeviceToHost));
  const double u = 100.0 / ((double)blocks * wpb);   // shares of the summed wall-clock ticks
  double tot = 0;
  for (int k = C_DBG_TNODE; k <= C_DBG_TEND; ++k) if (k != C_DBG_TMAX) tot += t[k - C_DBG_INS];
  const double sc = tot > 0 ? (double)blocks * wpb / tot : 0;   // -> percent
  fprintf(stderr, "[kb] round %d row pass time shares: stage %.1f %%, Failed %.1f %%, Join %.1f %%, A3 %.1f %%, write-back "
          "%.1f %% (%u rows, %u waves)\n", r, t[C_DBG_TSTART - C_DBG_INS] * u * sc, t[C_DBG_TBASE - C_DBG_INS] * u * sc,
          t[C_DBG_TINS - C_DBG_INS] * u * sc, t[C_DBG_TNODE - C_DBG_INS] * u * sc, t[C_DBG_TEND - C_DBG_INS] * u * sc, s->R,
          blocks * wpb);
  return KB_OK;
}
// KB_DEV=512: the Join-response wave path's phases (the counters cleared ahead of it under KB_DEBUG_WAVES alone)
static int dbg_resp_clear(kb_sim* s) {
  if (s->debug_waves) HIPCHK(hipMemsetAsync(s->d.ctr + C_DBG_INS, 0, 52, s->st));
  return KB_OK;
}
static int dbg_resp_report(kb_sim* s, int32_t r) {
  if (!s->debug_waves || !(s->d.dev & 512)) return KB_OK;
  uint32_t dbg[13];
  HIPCHK(hipMemcpyAsync(dbg, s->d.ctr + C_DBG_INS, 52, hipMemcpyDeviceToHost, s->st));
  HIPCHK(hipStreamSynchronize(s->st));
  fprintf(stderr, "[kb] round %d k_resp_wave: responders %u, responses %u: row staging %.1f us, joiners %.1f, prefix %.1f, "
          "fills %.1f (sums over waves)\n", r, dbg[10], dbg[12], dbg[11] * 0.01, dbg[8] * 0.01, dbg[6] * 0.01, dbg[9] * 0.01);
  return KB_OK;
}
