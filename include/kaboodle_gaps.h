/*
 * kaboodle_gaps.h — the gap list and the holders query of a simulated mesh: which rows lack or hold which ids
 * (DESIGN.md §21).
 *
 * An extension of the C ABI of kaboodle_sim.h, implemented by the HIP library only (the CPU oracle answers the
 * same questions through kaboodle_amd/gaps.py's gaps_ref and holders_ref, from its stamp rows).  The censuses answer
 * with counts; these two calls answer with NAMES: kb_sim_gaps lists the (row, id) cells the view census counts as
 * missing and stale, kb_sim_holders lists the observers whose view holds a given id, for up to KB_HOLDERS_MAX ids a
 * call.  Both read the member bits, the running set and the external ids and write only their own scratch, so a run
 * that calls them every round computes exactly what a run without them computes.  Nothing is allocated or launched
 * unless these calls are made.
 *
 * Definitions: those of kaboodle_census.h.  The state is the one after the last completed round; lifecycle calls
 * queued since the last step do not count yet.
 *   observer       a running row held by the handle
 *   view(i)        the member set kb_sim_peers(i) reports (it includes i itself)
 *   missing cell   (i, j): i is an observer, j is running and j is not in view(i).  A running row that does not
 *                  hold itself lists (i, i)
 *   stale cell     (i, j): i is an observer, j is in view(i) and j is neither running nor external
 *   holders of j   the observers i whose view contains j (i itself included, when it runs and holds itself)
 * External peers (kb_sim_set_external) are in neither gap list; their holders are answered like any id's.
 */
#ifndef KABOODLE_GAPS_H
#define KABOODLE_GAPS_H

#include "kaboodle_census.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KB_HOLDERS_MAX 1024   /* ids one kb_sim_holders call answers */

typedef struct kb_gaps {
  int32_t  round;           /* kb_stats.round when taken                                                 */
  uint32_t observers;       /* running rows                                                              */
  uint64_t missing, stale;  /* the cells of each kind: kb_census.missing / .stale of the same state      */
  uint64_t missing_listed, stale_listed;   /* pairs written to each list: 0, or the total                */
  uint32_t rows_missing, rows_stale;       /* observers with at least one such cell                      */
  uint64_t reserved[4];
} kb_gaps;

/* List the gaps.  missing_pairs / stale_pairs receive (row, id), two words a pair, ascending by (row, id); cap_missing
 * and cap_stale are their capacities in PAIRS.  A list is written only when its total is at most its capacity;
 * otherwise nothing of it is written, its *_listed is 0 and the call still answers KB_OK with the totals (the rule
 * of kb_sim_reciprocity's pairs).  The two lists decide independently.  A NULL list with capacity 0 asks for the
 * totals alone; a NULL list with a capacity, or a list with capacity 0, is KB_INVALID_ARGUMENT, as is out == NULL.
 * The totals are 64-bit: a mesh that has just begun to join at 65,536 peers has billions of missing cells.  Device
 * memory for a list is allocated for the pairs that are listed, never from the capacity.
 *
 * Dense handles of kb_sim_create (either A3 order) and of kb_sim_create_local answer for the whole mesh: a group's
 * shards live on one device, their streams are drained first, and the launches read every shard's rows through a
 * table of at most 8 bases, so a group's output is byte for byte the unsharded mesh's.  Sparse rows and handles of
 * kb_sim_create_rank answer KB_INVALID_OPERATION, sparse rows first. */
int kb_sim_gaps(kb_sim* sim, kb_gaps* out,
                uint32_t* missing_pairs, size_t cap_missing,
                uint32_t* stale_pairs, size_t cap_stale);

/* Device time of the last kb_sim_gaps of this handle in ms (HIP events around the count and scan kernels, plus the
 * span of the listing kernels when a list was written; the host's read of the totals between the two and the
 * download of the lists are not in it); 0 before the first answer.  Measurement surface (tools/gaps_cost.py). */
int kb_sim_gaps_device_ms(kb_sim* sim, double* ms);

/* The holders of n_ids ids (1 .. KB_HOLDERS_MAX, each < capacity, else KB_INVALID_ARGUMENT; an id may be asked for
 * more than once and is answered each time).  offsets (n_ids + 1 entries, always written) delimits query q's slice
 * of rows: rows[offsets[q]] .. rows[offsets[q + 1] - 1] are the observers whose view holds ids[q], ascending;
 * offsets[q + 1] - offsets[q] is kb_sim_census's known_by[ids[q]] of the same state.  *n_rows (may be NULL) receives
 * the total, offsets[n_ids].  rows is written only when the total is at most cap_rows; otherwise nothing of it is
 * written.  rows may be NULL with cap_rows 0 (the offsets alone); NULL with a capacity, or non-NULL with capacity 0,
 * is KB_INVALID_ARGUMENT.  The same handles answer as for kb_sim_gaps. */
int kb_sim_holders(kb_sim* sim, const uint32_t* ids, size_t n_ids,
                   uint64_t* offsets,
                   uint32_t* rows, size_t cap_rows, uint64_t* n_rows);

/* Device time of the last kb_sim_holders of this handle in ms (as kb_sim_gaps_device_ms: the column pass, the count
 * and the scan, plus the listing kernel when rows was written); 0 before the first answer. */
int kb_sim_holders_device_ms(kb_sim* sim, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* KABOODLE_GAPS_H */
