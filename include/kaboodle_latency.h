/*
 * kaboodle_latency.h — the latency census of a simulated mesh: the ping-latency table (PeerInfo.latency) read
 * mesh-wide in one device pass.
 *
 * An extension of the C ABI of kaboodle_sim.h, implemented by the HIP library only (the CPU oracle answers the
 * same question through kaboodle_amd/latency.py's latency_census_ref, from peer_states).  The census streams the
 * latency table once on the device; it reads state and writes only its own scratch, so a run with a census every
 * round computes exactly what a run without one computes.
 *
 * Definitions.  The census is taken on the state after the last completed round, with the running set that
 * kb_sim_fingerprints uses at that moment (lifecycle calls queued since the last step do not count yet).
 *   observer        a running row held by the handle
 *   cell (i, j)     COUNTS iff i is an observer, j is in view(i) (the member bit is set: the bit is the
 *                   authority) and the stored latency is not None.  These are exactly the entries of
 *                   kb_sim_peer_states(i) with latency_ms != KB_LATENCY_NONE, suspects included; external ids
 *                   count as peers j like any other id.
 * Per id j < capacity, over the counting cells of column j:
 *   measured_by[j]  their number (the observers that hold a first-hand latency of j; known_by[j] of the view
 *                   census minus this is the number that hold j on hearsay alone)
 *   sum_ms[j]       the sum of their values
 *   min_ms[j], max_ms[j]   KB_CENSUS_NONE and 0 when measured_by[j] is 0
 * Per row i < capacity, over the counting cells of row i:
 *   measured[i], row_sum_ms[i]   both 0 for rows that are not observers
 * Everything is integer add, min and max: the result does not depend on the order of execution.
 */
#ifndef KABOODLE_LATENCY_H
#define KABOODLE_LATENCY_H

#include "kaboodle_census.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KB_LAT_HIST 17

typedef struct kb_lat_census {
  int32_t  round;           /* kb_stats.round when taken (-1: kb_latency_census_of)             */
  uint32_t observers;       /* running rows counted (all shards of an in-process group)         */
  uint64_t measured;        /* counting cells                                                   */
  uint64_t sum_ms;          /* the sum of their values                                          */
  uint32_t min_ms, max_ms;  /* over all counting cells; KB_CENSUS_NONE / 0 when there is none   */
  uint32_t max_peer;        /* the id whose max_ms is largest (lowest id on ties); KB_CENSUS_NONE when nothing
                               is measured                                                      */
  uint32_t measured_ids;    /* ids with measured_by > 0                                         */
  uint64_t hist[KB_LAT_HIST];  /* counting cells by value: bucket 0 holds 0, bucket b >= 1 the values v with
                               floor(log2 v) = b - 1; 65534, the largest value stored, is in bucket 16 */
  uint64_t orphans;         /* cells of running rows that hold a value while the member bit is clear (the
                               table's invariant says 0); counted here and in no other field */
  uint64_t reserved[4];
} kb_lat_census;

/* Take the census.  Any of the arrays may be NULL; a non-NULL array must hold `capacity` elements (cap_ids for
 * measured_by, sum_ms, min_ms and max_ms; cap_rows for measured and row_sum_ms), else KB_INVALID_ARGUMENT.
 *
 * Dense handles of kb_sim_create with track_latency answer, and kb_sim_create_local groups of them (each shard
 * runs the pass over its own rows; counts and sums add, min and max combine).  KB_INVALID_OPERATION, with a
 * kb_last_error text, for sparse rows (they keep no latency table), for handles without track_latency and for
 * handles of kb_sim_create_rank. */
int kb_sim_latency_census(kb_sim* sim, kb_lat_census* out,
                          uint32_t* measured_by, uint64_t* sum_ms, uint32_t* min_ms, uint32_t* max_ms, size_t cap_ids,
                          uint32_t* measured, uint64_t* row_sum_ms, size_t cap_rows);

/* Device time of the last kb_sim_latency_census of this handle in ms (HIP events around its kernels and the
 * clearing of its scratch; the copies to the host and the O(ids) summary are not in it).  A group reports the sum
 * over its shards.  Measurement surface (tools/latency_census_cost.py). */
int kb_sim_latency_census_device_ms(kb_sim* sim, double* ms);

/* The same kernels over host arrays: `lat` is peer-major [n_ids][n_rows] (0xFFFF = None), `member` is
 * [n_rows][n_ids] bytes (non-zero: j is in view(i)), `running` is [n_rows].  They are uploaded in the layout the
 * kernel reads from a real handle (columns padded to the table's row stride, member rows packed to bit rows of the
 * handle's width).  Rows and ids are independent here: measured_by .. max_ms hold n_ids elements (cap_ids),
 * measured and row_sum_ms n_rows (cap_rows).  A test surface; KB_NO_DEVICE without a GPU. */
int kb_latency_census_of(int device, const uint16_t* lat, const uint8_t* member, const uint8_t* running,
                         size_t n_ids, size_t n_rows, kb_lat_census* out,
                         uint32_t* measured_by, uint64_t* sum_ms, uint32_t* min_ms, uint32_t* max_ms, size_t cap_ids,
                         uint32_t* measured, uint64_t* row_sum_ms, size_t cap_rows);

#ifdef __cplusplus
}
#endif
#endif /* KABOODLE_LATENCY_H */
