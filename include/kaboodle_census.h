/*
 * kaboodle_census.h — the view census of a simulated mesh: who knows whom, mesh-wide.
 *
 * An extension of the C ABI of kaboodle_sim.h, implemented by the HIP library only (the CPU oracle answers the
 * same question through kaboodle_amd/census.py's census_ref, from its stamp rows).  The census is computed on
 * the device in one streaming pass over the member bits (dense engine) or the rows' exception lists (sparse
 * rows); it reads state and writes only its own scratch, so a run with a census every round computes exactly
 * what a run without one computes.
 *
 * Definitions.  The census is taken on the state after the last completed round, with the running set that
 * kb_sim_fingerprints and kb_sim_true_fingerprint use at that moment (lifecycle calls queued since the last
 * step do not count yet).
 *   observer      a running row held by the handle
 *   view(i)       the member set kb_sim_peers(i) reports (it includes i itself)
 *   known_by[j]   for every id j < capacity: the number of observers whose view contains j (non-running and
 *                 external ids get an entry too)
 *   missing[i]    the number of running ids not in view(i)
 *   stale[i]      the number of ids in view(i) that are neither running nor external
 * missing[i] and stale[i] are 0 for rows that are not observers.  External peers (kb_sim_set_external) are real
 * instances outside the mesh: they count in known_by and in pairs, never in missing or stale.
 */
#ifndef KABOODLE_CENSUS_H
#define KABOODLE_CENSUS_H

#include "kaboodle_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KB_CENSUS_NONE 0xFFFFFFFFu

typedef struct kb_census {
  int32_t  round;           /* kb_stats.round when taken                                        */
  uint32_t observers;       /* running rows counted (all shards of an in-process group)         */
  uint32_t running;         /* running ids of the whole mesh                                    */
  uint32_t exact_views;     /* observers with missing == 0 and stale == 0                       */
  uint64_t pairs;           /* sum of |view(i)| over observers                                  */
  uint64_t missing, stale;  /* sums of missing[i], stale[i]                                     */
  uint32_t full_ids;        /* running ids with known_by == observers                           */
  uint32_t ghost_ids;       /* non-running, non-external ids with known_by > 0                  */
  uint32_t least_known, least_known_by;   /* the running id with the smallest known_by (lowest id on ties);
                                             KB_CENSUS_NONE / 0 when nothing runs                */
  uint32_t top_ghost, top_ghost_by;       /* the ghost id with the largest known_by (lowest id on ties);
                                             KB_CENSUS_NONE / 0 when there is none                */
  uint64_t reserved[4];
} kb_census;

/* Take the census.  Any of the arrays may be NULL; a non-NULL array must hold `capacity` elements
 * (cap_ids for known_by, cap_rows for missing and stale), else KB_INVALID_ARGUMENT.
 *
 * Handles of kb_sim_create and kb_sim_create_local answer for the whole mesh (a group counts each shard's rows
 * and sums them, as kb_sim_stats does).
 *
 * Handles of kb_sim_create_rank answer for THEIR OWN ROWS ONLY and make no collective call: known_by is the
 * rank's partial sum, missing / stale are filled for its rows and zero elsewhere, and the summary fields cover
 * its observers (`running` is still the whole mesh's: the running set is replicated).  The caller adds the
 * ranks' partials: known_by, observers, pairs, missing and stale add; exact_views adds; full_ids, ghost_ids,
 * least_known and top_ghost follow from the summed known_by.
 */
int kb_sim_census(kb_sim* sim, kb_census* out,
                  uint32_t* known_by, size_t cap_ids,
                  uint32_t* missing, uint32_t* stale, size_t cap_rows);

/* Device time of the last kb_sim_census of this handle in ms (HIP events around its kernels and the clearing of
 * its scratch; the copies to the host and the O(ids) summary are not in it).  A group reports the sum over its
 * shards.  Measurement surface (tools/census_cost.py). */
int kb_sim_census_device_ms(kb_sim* sim, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* KABOODLE_CENSUS_H */
