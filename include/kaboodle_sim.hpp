// kaboodle_sim.hpp — thin header-only C++ wrapper over the C ABI (include/kaboodle_sim.h) with the
// shape of the reference's `Kaboodle` surface (src/lib.rs:65-369): a `Mesh` owns one simulated mesh
// on one GPU, `Mesh::Peer` is the per-instance view (start/stop/ping_addrs/fingerprint/peers/...).
// Errors become `kb::Error` (status code + kb_last_error text), mirroring KaboodleError
// (src/errors.rs:8-24).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "kaboodle_sim.h"
#include "kaboodle_census.h"
#include "kaboodle_reciprocity.h"
#include "kaboodle_classes.h"
#include "kaboodle_latency.h"
#include "kaboodle_age.h"
#include "kaboodle_delta.h"
#include "kaboodle_islands.h"
#include "kaboodle_gaps.h"

namespace kb {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc, const char* fn) {
  if (rc != KB_OK) {
    const char* e = kb_last_error();
    throw Error(rc, std::string(fn) + ": " + (e ? e : ""));
  }
}

inline std::string format_addr(uint32_t id) {                 // canonical simulated SocketAddr
  char buf[32];
  check(kb_format_addr(id, buf, sizeof buf), "kb_format_addr");
  return buf;
}

class Mesh {
 public:
  explicit Mesh(const kb_config& cfg) : capacity_(cfg.capacity) { check(kb_sim_create(&cfg, &h_), "kb_sim_create"); }
  static kb_config defaults() { kb_config c; kb_config_default(&c); return c; }
  ~Mesh() { if (h_) kb_sim_destroy(h_); }
  Mesh(const Mesh&) = delete;
  Mesh& operator=(const Mesh&) = delete;
  Mesh(Mesh&& o) noexcept : h_(std::exchange(o.h_, nullptr)), capacity_(o.capacity_) {}

  void step(uint32_t rounds = 1) { check(kb_sim_step(h_, rounds), "kb_sim_step"); }
  kb_stats stats() const { kb_stats s; check(kb_sim_stats(h_, &s), "kb_sim_stats"); return s; }
  uint32_t true_fingerprint() const { uint32_t f; check(kb_sim_true_fingerprint(h_, &f), "kb_sim_true_fingerprint"); return f; }
  kb_sim* handle() const { return h_; }

  // the view census (kaboodle_census.h; HIP library only): who knows whom, mesh-wide, counted on the device.
  // arrays = false asks for the summary alone.
  struct Census { kb_census summary; std::vector<uint32_t> known_by, missing, stale; };
  Census census(bool arrays = true) const {
    Census c;
    if (arrays) { c.known_by.resize(capacity_); c.missing.resize(capacity_); c.stale.resize(capacity_); }
    check(kb_sim_census(h_, &c.summary, arrays ? c.known_by.data() : nullptr, c.known_by.size(),
                        arrays ? c.missing.data() : nullptr, arrays ? c.stale.data() : nullptr, c.missing.size()),
          "kb_sim_census");
    return c;
  }

  // the reciprocity census (kaboodle_reciprocity.h; HIP library only): one-way and mutual gaps between views.
  // pairs: the mutual pairs (i, j), i < j, ascending, two words each; empty when their number is above max_pairs
  // (summary.mutual_pairs has the total).  arrays = false asks for the summary alone.
  struct Reciprocity { kb_reciprocity summary; std::vector<uint32_t> mutual, lacks, lacked_by, pairs; };
  Reciprocity reciprocity(bool arrays = true, size_t max_pairs = 65536) const {
    Reciprocity r;
    if (arrays) { r.mutual.resize(capacity_); r.lacks.resize(capacity_); r.lacked_by.resize(capacity_); r.pairs.resize(2 * max_pairs); }
    check(kb_sim_reciprocity(h_, &r.summary, arrays ? r.mutual.data() : nullptr, arrays ? r.lacks.data() : nullptr,
                             arrays ? r.lacked_by.data() : nullptr, r.mutual.size(),
                             arrays && max_pairs ? r.pairs.data() : nullptr, arrays ? max_pairs : 0),
          "kb_sim_reciprocity");
    r.pairs.resize(2 * (size_t)r.summary.pairs_listed);
    return r;
  }

  // the fingerprint-class census (kaboodle_classes.h; HIP library only): the running rows grouped by equal
  // fingerprint.  classes: the first `top` <= KB_FPC_LIST_MAX classes, size descending then fp ascending; rep / size:
  // per id, the lowest id and the size of its class (KB_CENSUS_NONE / 0 for rows that are not running).
  // arrays = false asks for the summary and the list alone.
  struct FpClasses { kb_fp_classes summary; std::vector<kb_fp_class> classes; std::vector<uint32_t> rep, size; };
  FpClasses fp_classes(size_t top = 16, bool arrays = true) const {
    FpClasses r;
    r.classes.resize(top);
    if (arrays) { r.rep.resize(capacity_); r.size.resize(capacity_); }
    size_t n = 0;
    check(kb_sim_fp_classes(h_, &r.summary, top ? r.classes.data() : nullptr, top, &n, arrays ? r.rep.data() : nullptr,
                            arrays ? r.size.data() : nullptr, r.rep.size()),
          "kb_sim_fp_classes");
    r.classes.resize(n);
    return r;
  }

  // the latency census (kaboodle_latency.h; HIP library only, dense handles with track_latency): the ping-latency
  // table read mesh-wide.  Per id: the observers holding a first-hand latency of it, their sum, min and max; per row:
  // its measured entries and their sum.  arrays = false asks for the summary alone.
  struct LatencyCensus {
    kb_lat_census summary;
    std::vector<uint32_t> measured_by, min_ms, max_ms, measured;
    std::vector<uint64_t> sum_ms, row_sum_ms;
  };
  LatencyCensus latency_census(bool arrays = true) const {
    LatencyCensus r;
    if (arrays) {
      r.measured_by.resize(capacity_); r.min_ms.resize(capacity_); r.max_ms.resize(capacity_); r.sum_ms.resize(capacity_);
      r.measured.resize(capacity_); r.row_sum_ms.resize(capacity_);
    }
    check(kb_sim_latency_census(h_, &r.summary, arrays ? r.measured_by.data() : nullptr, arrays ? r.sum_ms.data() : nullptr,
                                arrays ? r.min_ms.data() : nullptr, arrays ? r.max_ms.data() : nullptr, r.measured_by.size(),
                                arrays ? r.measured.data() : nullptr, arrays ? r.row_sum_ms.data() : nullptr, r.measured.size()),
          "kb_sim_latency_census");
    return r;
  }

  // the contact-age census (kaboodle_age.h; HIP library only, sparse rows): the stamp table read mesh-wide.  Per id: the observers
  // holding it as suspect, ancient, windowed and fresh and the latest instant any of them heard from it; per row the same
  // four counts over its view.  arrays = false asks for the summary alone.
  struct AgeCensus {
    kb_age_census summary;
    std::vector<uint32_t> suspected_by, ancient_by, windowed_by, fresh_by, suspects, ancient, windowed, fresh;
    std::vector<int32_t> last_heard;
  };
  AgeCensus age_census(bool arrays = true) const {
    AgeCensus r;
    if (arrays) {
      for (auto* v : {&r.suspected_by, &r.ancient_by, &r.windowed_by, &r.fresh_by, &r.suspects, &r.ancient, &r.windowed, &r.fresh})
        v->resize(capacity_);
      r.last_heard.resize(capacity_);
    }
    auto p = [&](std::vector<uint32_t>& v) { return arrays ? v.data() : nullptr; };
    check(kb_sim_age_census(h_, &r.summary, p(r.suspected_by), p(r.ancient_by), p(r.windowed_by), p(r.fresh_by),
                            arrays ? r.last_heard.data() : nullptr, r.last_heard.size(), p(r.suspects), p(r.ancient),
                            p(r.windowed), p(r.fresh), r.suspects.size()),
          "kb_sim_age_census");
    return r;
  }

  // the view-delta census (kaboodle_delta.h; HIP library only, dense handles): what every view gained and lost since
  // delta_mark().  Per id: the continuing rows whose view gained / lost it; per row: the ids its view gained, lost, and
  // lost although they run.  advance = true makes the current state the baseline in the same pass; arrays = false asks
  // for the summary alone.
  struct DeltaCensus { kb_delta summary; std::vector<uint32_t> gained_by, lost_by, gained, lost, lost_live; };
  void delta_mark() { check(kb_sim_delta_mark(h_), "kb_sim_delta_mark"); }
  void delta_release() { check(kb_sim_delta_release(h_), "kb_sim_delta_release"); }
  DeltaCensus delta_census(bool advance = true, bool arrays = true) {
    DeltaCensus r;
    if (arrays) for (auto* v : {&r.gained_by, &r.lost_by, &r.gained, &r.lost, &r.lost_live}) v->resize(capacity_);
    auto p = [&](std::vector<uint32_t>& v) { return arrays ? v.data() : nullptr; };
    check(kb_sim_delta_census(h_, &r.summary, p(r.gained_by), p(r.lost_by), r.gained_by.size(), p(r.gained), p(r.lost),
                              p(r.lost_live), r.gained.size(), advance ? KB_DELTA_ADVANCE : 0u),
          "kb_sim_delta_census");
    return r;
  }

  // the island census (kaboodle_islands.h; HIP library only, dense handles): the connected components of the
  // "i holds j" graph over the running peers.  Per id: the lowest id of its island (KB_CENSUS_NONE where it does not
  // run) and the island's size.  arrays = false asks for the summary alone.
  struct Islands { kb_islands summary; std::vector<uint32_t> label, size; };
  Islands islands(bool arrays = true) const {
    Islands r;
    if (arrays) { r.label.resize(capacity_); r.size.resize(capacity_); }
    check(kb_sim_islands(h_, &r.summary, arrays ? r.label.data() : nullptr, arrays ? r.size.data() : nullptr, r.label.size()),
          "kb_sim_islands");
    return r;
  }

  // the gap list (kaboodle_gaps.h; HIP library only, dense handles): the cells the view census counts as missing and
  // stale, as (row, id) pairs in ascending order.  A list of more than max_pairs pairs stays empty and its *_listed
  // is 0; the totals are always there.  max_pairs = 0 asks for the totals alone.
  struct Gaps { kb_gaps summary; std::vector<uint32_t> missing_pairs, stale_pairs; };
  Gaps gaps(size_t max_pairs = 65536) const {
    Gaps r;
    r.missing_pairs.resize(2 * max_pairs); r.stale_pairs.resize(2 * max_pairs);
    check(kb_sim_gaps(h_, &r.summary, max_pairs ? r.missing_pairs.data() : nullptr, max_pairs,
                      max_pairs ? r.stale_pairs.data() : nullptr, max_pairs), "kb_sim_gaps");
    r.missing_pairs.resize(2 * r.summary.missing_listed); r.stale_pairs.resize(2 * r.summary.stale_listed);
    return r;
  }
  // the holders query: for each of 1 .. KB_HOLDERS_MAX ids the running rows whose view holds it; query q's rows are
  // rows[offsets[q]] .. rows[offsets[q + 1] - 1], ascending
  struct Holders { std::vector<uint64_t> offsets; std::vector<uint32_t> rows; };
  Holders holders(const std::vector<uint32_t>& ids) const {
    Holders r;
    r.offsets.resize(ids.size() + 1);
    uint64_t n = 0;
    check(kb_sim_holders(h_, ids.data(), ids.size(), r.offsets.data(), nullptr, 0, &n), "kb_sim_holders");
    if (!n) return r;
    r.rows.resize(n);                               // the state does not change between the two calls
    check(kb_sim_holders(h_, ids.data(), ids.size(), r.offsets.data(), r.rows.data(), r.rows.size(), &n), "kb_sim_holders");
    return r;
  }

  // the per-instance view: method names of src/lib.rs
  class Peer {
   public:
    Peer(kb_sim* h, uint32_t id) : h_(h), id_(id) {}
    // :136 — a stopped peer comes back at a fresh address (src/kaboodle.rs:138-152) with its map
    void start() { check(kb_sim_restart_node(h_, id_, &id_), "kb_sim_restart_node"); }
    void stop() { check(kb_sim_stop_node(h_, id_), "kb_sim_stop_node"); }               // :159
    bool is_running() const { int r; check(kb_sim_is_running(h_, id_, &r), "kb_sim_is_running"); return r != 0; }
    std::string self_addr() const { return format_addr(id_); }                          // :312
    void ping_addrs(const std::vector<uint32_t>& ids) {                                 // :268
      check(kb_sim_ping_addrs(h_, id_, ids.data(), ids.size()), "kb_sim_ping_addrs");
    }
    void set_identity(const std::vector<uint8_t>& ident) {                              // :323
      check(kb_sim_set_identity(h_, id_, ident.data(), ident.size()), "kb_sim_set_identity");
    }
    uint32_t fingerprint() const { uint32_t f; check(kb_sim_fingerprint(h_, id_, &f), "kb_sim_fingerprint"); return f; }
    std::vector<uint32_t> peers() const {                                               // :339 (ids)
      size_t n = 0;
      check(kb_sim_peers(h_, id_, nullptr, 0, &n), "kb_sim_peers");
      std::vector<uint32_t> v(n);
      check(kb_sim_peers(h_, id_, v.data(), v.size(), &n), "kb_sim_peers");
      v.resize(n);
      return v;
    }
    // Kaboodle::peers as the reference returns it (:339-345): address -> identity bytes
    std::vector<std::pair<std::string, std::vector<uint8_t>>> peers_with_identity() const {
      std::vector<std::pair<std::string, std::vector<uint8_t>>> out;
      for (uint32_t p : peers()) out.emplace_back(format_addr(p), identity_of(h_, p));
      return out;
    }
    std::vector<uint8_t> identity() const { return identity_of(h_, id_); }
    std::vector<kb_peer_state> peer_states() const {                                   // :348
      size_t n = 0;
      check(kb_sim_peer_states(h_, id_, nullptr, 0, &n), "kb_sim_peer_states");
      std::vector<kb_peer_state> v(n);
      check(kb_sim_peer_states(h_, id_, v.data(), v.size(), &n), "kb_sim_peer_states");
      v.resize(n);
      return v;
    }
    // events.rs:18-125 behind discover_peers / discover_departures / discover_fingerprint_changes
    // (:186-263): watch() once, then events() after each step drains one batch
    struct Events { std::vector<uint32_t> discovered, departed; bool fingerprint_changed; uint32_t fingerprint; };
    void watch() { check(kb_sim_watch(h_, id_), "kb_sim_watch"); }
    Events events() {
      Events e;
      size_t nd = 0, np = 0;
      int ch = 0;
      check(kb_sim_events(h_, id_, nullptr, 0, &nd, nullptr, 0, &np, &e.fingerprint, &ch), "kb_sim_events");
      e.discovered.resize(nd);
      e.departed.resize(np);
      check(kb_sim_events(h_, id_, e.discovered.data(), nd, &nd, e.departed.data(), np, &np, &e.fingerprint, &ch),
            "kb_sim_events");
      e.fingerprint_changed = ch != 0;
      return e;
    }
   private:
    static std::vector<uint8_t> identity_of(kb_sim* h, uint32_t id) {
      uint8_t buf[32];
      size_t len = 0;
      check(kb_sim_identity(h, id, buf, sizeof buf, &len), "kb_sim_identity");
      return std::vector<uint8_t>(buf, buf + len);
    }
    kb_sim* h_;
    uint32_t id_;
  };
  Peer peer(uint32_t id) const { return Peer(h_, id); }

  // real instances in the mesh: an external peer's records out, its datagrams in
  struct Record { kb_unicast rec; std::vector<uint32_t> ids; };
  void set_external(uint32_t id) { check(kb_sim_set_external(h_, id), "kb_sim_set_external"); }
  void inject(const kb_unicast& rec, const std::vector<uint32_t>& ids = {}) {
    kb_unicast m = rec;
    m.pay_len = (uint32_t)ids.size();
    check(kb_sim_inject(h_, &m, ids.empty() ? nullptr : ids.data()), "kb_sim_inject");
  }
  std::vector<Record> exported() {                    // drains: (round, wave, sender, seq) order
    size_t n = 0, ni = 0;
    check(kb_sim_exported(h_, nullptr, 0, &n, nullptr, 0, &ni), "kb_sim_exported");
    std::vector<kb_unicast> v(n);
    std::vector<uint32_t> ids(ni);
    check(kb_sim_exported(h_, v.data(), v.size(), &n, ids.data(), ids.size(), &ni), "kb_sim_exported");
    std::vector<Record> out;
    for (size_t k = 0; k < n; ++k)
      out.push_back({v[k], std::vector<uint32_t>(ids.begin() + v[k].pay_off, ids.begin() + v[k].pay_off + v[k].pay_len)});
    return out;
  }

 private:
  kb_sim* h_ = nullptr;
  uint32_t capacity_ = 0;
};

}  // namespace kb
