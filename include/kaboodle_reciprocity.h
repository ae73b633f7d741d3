/*
 * kaboodle_reciprocity.h — the reciprocity census of a simulated mesh: one-way and mutual gaps between views
 * (DESIGN.md §13).
 *
 * An extension of the C ABI of kaboodle_sim.h, implemented by the HIP library only (the CPU oracle answers the
 * same question through kaboodle_amd/reciprocity.py's reciprocity_ref, from its stamp rows).  The view census
 * (kaboodle_census.h) says how many running ids a view lacks; this one says whether the lacked peer still holds
 * the observer.  Two peers that have dropped each other never message each other again, so a mutual gap is
 * permanent, while a one-way gap heals as soon as the side that still holds the other pings it.
 * It is computed on the device in one streaming pass over the member bits and their transpose; it reads state
 * and writes only its own scratch, so a run with a reciprocity census every round computes exactly what a run
 * without one computes.
 *
 * Definitions.  The census is taken on the state after the last completed round, with the running set that
 * kb_sim_census uses (lifecycle calls queued since the last step do not count yet).
 *   observer        a running row held by the handle
 *   view(i)         the member set kb_sim_peers(i) reports
 * For observers i != j:
 *   i lacks j       j is not in view(i)
 *   mutual gap      i lacks j and j lacks i
 *   one-way gap     i lacks j and j holds i
 * Per row i (0 for rows that are not observers):
 *   mutual[i]       the number of j with a mutual gap
 *   lacks[i]        the number of j that i lacks while j holds i
 *   lacked_by[i]    the number of j that i holds while j lacks i
 * so mutual[i] + lacks[i] is kb_sim_census's missing[i], the sums of lacks and lacked_by are equal, and the sum
 * of mutual is twice mutual_pairs.  Ids that are not running count neither as rows nor as columns, whatever
 * their rows still hold; external peers (kb_sim_set_external) are never observers and appear nowhere.
 */
#ifndef KABOODLE_RECIPROCITY_H
#define KABOODLE_RECIPROCITY_H

#include "kaboodle_census.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kb_reciprocity {
  int32_t  round;             /* kb_stats.round when taken                                          */
  uint32_t observers;         /* running rows counted                                               */
  uint64_t mutual_pairs;      /* unordered {i,j} with a mutual gap                                  */
  uint64_t oneway_pairs;      /* ordered (i,j): i lacks j, j holds i = sum of lacks                 */
  uint32_t rows_mutual, rows_oneway;     /* observers with mutual[i] > 0 / lacks[i] > 0             */
  uint32_t max_mutual_row, max_mutual;   /* the row with the largest mutual[i] (lowest id on ties);
                                            KB_CENSUS_NONE / 0 when no row has a mutual gap         */
  uint64_t pairs_listed;      /* entries written to `pairs` (0 or mutual_pairs)                     */
  uint64_t reserved[4];
} kb_reciprocity;

/* Take the reciprocity census.  Each array may be NULL; a non-NULL row array (mutual, lacks, lacked_by) must
 * hold `capacity` elements (cap_rows), else KB_INVALID_ARGUMENT.  out == NULL is KB_INVALID_ARGUMENT.
 *
 * `pairs` receives the mutual pairs as (i, j) with i < j, two words each (so it holds 2 * cap_pairs words),
 * ascending by (i, j).  It is written only when mutual_pairs <= cap_pairs; otherwise nothing is written,
 * pairs_listed is 0 and the call still returns KB_OK: the caller reads the total and decides.
 * Listing costs memory in proportion to the pairs listed, never more than the caller's own buffer: 8 bytes on the
 * device per pair (kept by the handle until it is destroyed) and 8 on the host during the call.  A mesh far from agreement has
 * 10^8 mutual pairs at 64K peers: a cap_pairs that admits them asks for gigabytes; when the device
 * cannot give them the call returns KB_CAPACITY.
 *
 * Handles of kb_sim_create (dense rows) and dense kb_sim_create_local groups answer for the whole mesh.
 *
 * Handles of kb_sim_create_rank and KB_VARIANT_SPARSE_ROWS handles return KB_INVALID_OPERATION (kb_last_error
 * says which).  A rank holds its own rows only and the transpose needs the other ranks' rows; sparse rows need an
 * O(entries) algorithm of their own, since an unbased row lacks O(N) ids.  Both are follow-ups, not built yet.
 */
int kb_sim_reciprocity(kb_sim* sim, kb_reciprocity* out,
                       uint32_t* mutual, uint32_t* lacks, uint32_t* lacked_by, size_t cap_rows,
                       uint32_t* pairs, size_t cap_pairs);

/* Device time of the last kb_sim_reciprocity of this handle in ms (HIP events around its kernels and the
 * clearing of its scratch, the pair pass included when it ran; the copies to the host, the summary and the sort of
 * the pair list are not in it).  Measurement surface (tools/reciprocity_cost.py). */
int kb_sim_reciprocity_device_ms(kb_sim* sim, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* KABOODLE_RECIPROCITY_H */
