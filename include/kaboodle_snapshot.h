/*
 * kaboodle_snapshot.h — snapshot and restore of a simulated mesh: the tables of a handle taken out as one byte
 * string and put back into a new handle, in the same or another process, in the same or another shard layout
 * (DESIGN.md §18).
 *
 * An extension of the C ABI of kaboodle_sim.h, implemented by the HIP library only.  The simulator is
 * deterministic (Philox is keyed on (seed, node, round)), so the whole future of a run is a function of its tables
 * and the round number: a restored handle continues bit for bit as the source would have.
 *
 * When.  A snapshot is taken on the state after the last completed round.  kb_sim_snapshot reads the handle's
 * state and writes only its own scratch: a run that snapshots every round computes exactly what a run without
 * snapshots computes.
 *
 * Who answers.  KB_VARIANT_SPARSE_ROWS handles of kb_sim_create, and kb_sim_create_local groups of them.
 * KB_INVALID_OPERATION, with a kb_last_error text, for dense rows (text naming "dense") and for handles of
 * kb_sim_create_rank (text naming "rank").
 *
 * Quiescent control plane.  Calls that queue work for the next round start (kb_sim_start_node, kb_sim_stop_node,
 * kb_sim_restart_node, kb_sim_probe, kb_sim_inject, an external peer's Join) leave the handle between two states;
 * with any such work queued kb_sim_snapshot returns KB_INVALID_OPERATION with a text naming "queued": step first.
 * State that persists is carried: an identity set on a stopped instance for its next address, the marks of
 * instances that restarted elsewhere, the ping_addrs queues, the external peers, and the Join / Failed lists the
 * next round will deliver.  Undrained outputs (kb_sim_exported, kb_sim_probe_responses) stay with the source
 * handle and are not carried.  Observers (kb_sim_watch) do not travel: a restored handle has none, as a new
 * Kaboodle has none (kb_sim_events is KB_INVALID_OPERATION until kb_sim_watch).
 *
 * Canonical and shard-agnostic.  Rows are stored in global id order, per-id tables once, counters as the
 * mesh-wide values an unsharded handle holds; a row's cached fingerprint is stored as the fold of the row, whether
 * the handle had computed it yet or not.  The bytes are a function of the mesh state alone: an unsharded handle
 * and a 3-shard group in the same state write byte-identical snapshots, taking it twice gives the same bytes, and
 * snapshot -> restore -> snapshot is a fixed point.  Only the entries in use travel (4 bytes each), whatever
 * kb_config.sparse_row_cap allocated.  The encoding is little-endian (the magic says so: "KBSNAPLE").
 *
 * Restore.  kb_sim_restore creates a new handle: shards 0 or 1 the shape of kb_sim_create, shards 2..8 a
 * kb_sim_create_local group.  The stored cfg.device is replaced by `device` (-1: the current device).  The
 * restored handle equals the source in everything the inspection surface reads and continues bit for bit as the
 * source would.  In a group the mesh-wide counters go to shard 0 and replicated per-id facts to every shard.
 * Profiling times, kb_sim_host_syncs and debug counters start at zero.
 *
 * Validation happens before any device call; each of these is KB_INVALID_ARGUMENT with a text that says which:
 * a short buffer, bad magic, an unknown format_version, a different abi_version or sizeof(kb_config), a checksum
 * mismatch, a section that runs past len or holds values out of range, a shard count that leaves a shard without
 * rows.  Rows the engine never writes are refused too, each by name: a row whose ids are not strictly ascending, an
 * entry with neither x nor a stamp, a based byte above 1 (a row's `based` flag itself is a choice of representation:
 * either value is accepted for any row, with the entries that go with it).  On a machine without a GPU a corrupt
 * snapshot is therefore KB_INVALID_ARGUMENT and a valid one KB_NO_DEVICE.
 *
 * What is stored, what is rebuilt.  Whatever a handle derives from its config alone (the base bitset with its
 * prefix counts and folds, the powers of Z, the caps) is rebuilt by creating the handle from the stored config;
 * the per-id segment CRCs are rebuilt from the stored identities.  Per-round scratch (inboxes, outboxes, scan
 * tiles, Join-response buffers) is empty between rounds and is neither stored nor rebuilt.  DESIGN.md §18 lists
 * every field.
 *
 * Not part of this version: dense rows, rank handles, the C++ wrapper, and reading a snapshot of another
 * format_version.
 */
#ifndef KABOODLE_SNAPSHOT_H
#define KABOODLE_SNAPSHOT_H

#include "kaboodle_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KB_SNAPSHOT_VERSION 1u

typedef struct kb_snapshot_info {        /* what the header of a snapshot says, no device needed              */
  uint32_t format_version;               /* KB_SNAPSHOT_VERSION                                               */
  uint32_t abi_version;                  /* KB_ABI_VERSION of the library that wrote it                       */
  kb_config cfg;                         /* the config the mesh was created with                              */
  int32_t  round;                        /* kb_stats.round when taken                                         */
  uint32_t alive;
  uint64_t entries;                      /* packed row entries carried (4 bytes each)                         */
  uint64_t bytes;                        /* total length                                                      */
  uint32_t payload_crc32;                /* zlib CRC-32 of everything after the header                        */
  uint32_t reserved[7];
} kb_snapshot_info;

/* The header of a snapshot, validated as kb_sim_restore validates it (layout, checksum and the sections' values:
 * everything but the shard count).  A pure host function. */
int kb_snapshot_info_of(const void* buf, size_t len, kb_snapshot_info* out);

/* Write the snapshot into buf.  *bytes is its length; buf NULL or cap 0 is a size query.  A cap smaller than the
 * length is KB_CAPACITY with *bytes set and buf untouched. */
int kb_sim_snapshot(kb_sim* sim, void* buf, size_t cap, uint64_t* bytes);

/* A new handle in the state of the snapshot. */
int kb_sim_restore(const void* buf, size_t len, int32_t shards, int32_t device, kb_sim** out);

/* Device time of the handle's last pack (kb_sim_snapshot) or unpack (the kb_sim_restore that made it) in ms: HIP
 * events around the scan and the entry kernel; copies and the host's assembly are not in it.  A group reports the
 * sum over its shards.  Measurement surface (tools/snapshot_cost.py). */
int kb_sim_snapshot_device_ms(kb_sim* sim, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* KABOODLE_SNAPSHOT_H */
