/*
 * kaboodle_delta.h — the view-delta census of a simulated mesh: what every view gained and lost since a mark
 * (DESIGN.md §19).
 *
 * An extension of the C ABI of kaboodle_sim.h, implemented by the HIP library only (the CPU oracle answers the
 * same question through kaboodle_amd/delta.py's delta_ref, from its stamp rows).  A BASELINE is a device-side copy
 * of the member bits and of the running set, taken at a MARK.  A delta census is one streaming pass on the device
 * that compares the current member bits with the baseline.  It reads the mesh's state and writes only its own
 * scratch and its baseline, so a run with a delta census every round computes exactly what a run without one
 * computes.  Nothing is allocated or launched unless these calls are made.
 *
 * Definitions.  State "now" is the state after the last completed round, with the running set kb_sim_census uses
 * (lifecycle calls queued since the last step do not count yet).  State "base" is the same state as it was at the
 * mark.
 *   continuing row  an id that was running at base and is running now.  An id runs for one interval only (restarts
 *                   and churn joins bind fresh ids), so a continuing row ran the whole time.
 *   new row         running now, not at base;  ended row: running at base, not now.  Neither contributes to any
 *                   gained or lost count; both are counted in the summary.
 *   G(i), L(i)      for a continuing row i: G(i) = view_now(i) \ view_base(i), L(i) = view_base(i) \ view_now(i);
 *                   only ids < capacity count
 *   gained_by[j]    for every id j < capacity: the number of continuing rows i with j in G(i)
 *   lost_by[j]      the same over L(i)
 *   gained[i]       |G(i)|;  lost[i] = |L(i)|;  lost_live[i] = |L(i) ∩ running now|; all three are 0 for rows that
 *                   are not continuing
 * Every id is classified by the running and external sets NOW: running, external (kb_sim_set_external; never
 * running), or neither ("dead" below).  An id gained and lost again between base and now cancels: the census sees
 * the two states only.
 */
#ifndef KABOODLE_DELTA_H
#define KABOODLE_DELTA_H

#include "kaboodle_census.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KB_DELTA_ADVANCE 1u   /* kb_sim_delta_census flags: the baseline becomes "now" in the same pass */

typedef struct kb_delta {
  int32_t  round_base;      /* kb_stats.round at the mark                                             */
  int32_t  round;           /* kb_stats.round when taken                                              */
  uint32_t continuing;      /* rows running at base and now (all shards of an in-process group)       */
  uint32_t new_rows;        /* rows running now, not at base                                          */
  uint32_t ended_rows;      /* rows running at base, not now                                          */
  uint32_t changed_rows;    /* continuing rows with gained + lost > 0                                 */
  uint32_t changed_ids;     /* ids with gained_by + lost_by > 0                                       */
  uint32_t top_false_drop, top_false_drop_by;   /* the running id with the largest lost_by > 0 (lowest id on
                                                   ties); KB_CENSUS_NONE / 0 when no running id was lost  */
  uint32_t pad;
  uint64_t learned;         /* sum of gained_by over ids running now                                  */
  uint64_t ghost_adds;      /* sum of gained_by over dead ids: re-inserted by stale gossip            */
  uint64_t detections;      /* sum of lost_by over dead ids: (observer, leaver) removals              */
  uint64_t false_drops;     /* sum of lost_by over ids running now: a live peer dropped from a view   */
  uint64_t ext_gained, ext_lost;   /* sums of gained_by / lost_by over external ids                   */
  uint64_t reserved[4];
} kb_delta;

/* Take the baseline, or replace it: the member bits and the running set as they are now (device-to-device copies;
 * rows x W/8 bytes per handle or shard, W = capacity rounded up to 8192).  KB_CAPACITY when the device cannot hold
 * it; the text names the bytes asked for.
 *
 * Dense handles of kb_sim_create and kb_sim_create_local answer (each shard of a group keeps the baseline of its own
 * rows; the per-id arrays and sums are added on the host, as kb_sim_census does).  Sparse rows and handles of
 * kb_sim_create_rank answer KB_INVALID_OPERATION, in all three calls, sparse rows first. */
int kb_sim_delta_mark(kb_sim* sim);

/* Take the delta census against the baseline.  Any of the arrays may be NULL; a non-NULL array must hold `capacity`
 * elements (cap_ids for gained_by and lost_by, cap_rows for gained, lost and lost_live), else KB_INVALID_ARGUMENT.
 * KB_INVALID_OPERATION ("no baseline") before the first kb_sim_delta_mark and after kb_sim_delta_release.
 *
 * flags = 0: strictly read-only; repeating the call gives the same answer.
 * flags = KB_DELTA_ADVANCE: afterwards the baseline is the current state, as if kb_sim_delta_mark had followed (the
 * pass stores the words that differ, and copies the rows that began to run).  The bits kept for a row that does not
 * run at the mark are never read and are not defined. */
int kb_sim_delta_census(kb_sim* sim, kb_delta* out,
                        uint32_t* gained_by, uint32_t* lost_by, size_t cap_ids,
                        uint32_t* gained, uint32_t* lost, uint32_t* lost_live, size_t cap_rows,
                        uint32_t flags);

/* Free the baseline.  KB_OK when there is none. */
int kb_sim_delta_release(kb_sim* sim);

/* Device time of the last kb_sim_delta_census of this handle in ms (HIP events around its kernels and the clearing
 * of its scratch; the copies to the host, the refresh of the running-set copy and the O(ids) summary are not in it);
 * 0 before the first answer.  A group reports the sum over its shards.  Measurement surface
 * (tools/delta_census_cost.py). */
int kb_sim_delta_device_ms(kb_sim* sim, double* ms);

/* Test surface: the delta census's kernel over host arrays, no mesh.  The rows are ids [row_lo, row_lo + rows) of a
 * mesh of `capacity` ids (row_lo + rows <= capacity): bits_base and bits_now are their member bits, [rows][W/32]
 * words with W = capacity rounded up to 8192 (bit j & 31 of word j >> 5 is id j; bits at ids >= capacity are
 * ignored).  run_base, run_now and external are bytes per id, [capacity].  rpw: rows per wave of the pass (0: as a
 * handle chooses; else rounded up to a multiple of 8 and held within 8 .. 4080); results do not depend on it.
 * Outputs as kb_sim_delta_census (round_base and round are -1; rows outside the range are 0), so the parts of
 * several row ranges add up as the shards of a group do.  KB_NO_DEVICE without a GPU. */
int kb_delta_of(int device, const uint32_t* bits_base, const uint8_t* run_base,
                const uint32_t* bits_now, const uint8_t* run_now, const uint8_t* external,
                size_t capacity, size_t row_lo, size_t rows, uint32_t rpw, kb_delta* out,
                uint32_t* gained_by, uint32_t* lost_by, size_t cap_ids,
                uint32_t* gained, uint32_t* lost, uint32_t* lost_live, size_t cap_rows);

#ifdef __cplusplus
}
#endif
#endif /* KABOODLE_DELTA_H */
