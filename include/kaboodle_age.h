/*
 * kaboodle_age.h — the contact-age census of a simulated mesh: the per-(node, peer) stamp byte (PeerInfo.state:
 * Known(instant), WaitingForPing, WaitingForIndirectPing) read mesh-wide in one device pass.
 *
 * An extension of the C ABI of kaboodle_sim.h, implemented by the HIP library only (the CPU oracle answers the
 * same question through kaboodle_amd/age.py's age_census_ref, from peer_states).  The census passes over the rows'
 * entry lists once on the device (KB_VARIANT_SPARSE_ROWS handles; the dense stamp table's pass is not part of this
 * version, dense handles refuse); it reads state and writes only its own scratch, so a run with a census every round
 * computes exactly what a run without one computes.
 *
 * Definitions.  The census is taken on the state after the last completed round, with the running set that
 * kb_sim_census uses at that moment (lifecycle calls queued since the last step do not count yet).  Let
 * r = out.round - 1 be the last simulated round (0 before the first round, as kb_sim_peer_states decodes).
 *   observer        a running row held by the handle
 *   cell (i, j)     COUNTS iff i is an observer, j != i and j is in view(i).  The member bit is the authority:
 *                   removals clear the bit and leave the byte, so a byte under a clear bit counts nowhere.  The
 *                   self entry counts nowhere.  External ids and non-running ids count as columns j like any
 *                   other id.
 * A counting cell's class and `since` are exactly what kb_sim_peer_states(i) reports for j (the decode with the
 * last simulated round's epoch: since = byte + epoch_base(r) - 192):
 *   suspect         state WAITING_FOR_PING or WAITING_FOR_INDIRECT_PING (stamp byte 1)
 *   ancient         KNOWN with since == INT32_MIN (stamp byte 2): older than the 1-byte window
 *   windowed        KNOWN with a since (stamp byte b >= 3); age = r - since = (r mod 64) + 192 - b.  The engines
 *                   stamp at most Known(r), byte (r mod 64) + 192 <= 255, and the oldest windowed byte is 3, so
 *                   age is in [0, 252] and within KB_AGE_HIST = 256 buckets
 *   fresh           windowed with age < SHARE_AGE (10), the KnownPeersRequest reply's own predicate
 * (A set member bit over byte 0 does not occur in an engine's state; kb_sim_peer_states does not report such a
 * cell and it is in no class here.)  The census reads the byte only, under both A3 variants:
 * KB_VARIANT_EXACT_LRU's exact instants of saturated entries are not read, an ancient cell is ancient.
 *
 * Per id j < capacity, over the counting cells of column j:
 *   suspected_by[j], ancient_by[j], windowed_by[j], fresh_by[j]
 *   last_heard[j]   the largest since among the windowed cells, INT32_MIN when there is none
 * Per row i < capacity (0 for rows that are not observers): suspects[i], ancient[i], windowed[i], fresh[i].
 * Everything is integer add and max: the result does not depend on the order of execution.
 *
 * Identities: for every observer i, suspects + ancient + windowed = |view(i)| - [i holds itself]; for every id j
 * the three *_by sum to known_by[j] (kb_sim_census) - [j is an observer that holds itself]; the histogram sums to
 * `windowed`, its first SHARE_AGE buckets to `fresh`.
 */
#ifndef KABOODLE_AGE_H
#define KABOODLE_AGE_H

#include "kaboodle_census.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KB_AGE_HIST 256

typedef struct kb_age_census {
  int32_t  round;           /* kb_stats.round when taken                                                 */
  uint32_t observers;       /* running rows counted (all shards of an in-process group)                  */
  uint64_t cells;           /* counting cells in a class: suspects + ancient + windowed                  */
  uint64_t suspects, ancient, windowed, fresh;   /* totals over all counting cells                       */
  uint64_t dead_suspects, dead_ancient, dead_windowed, dead_fresh;   /* the same restricted to columns that
                               are neither running nor external (the view census's stale class)          */
  uint32_t unheard_ids;     /* running ids with windowed_by == 0                                         */
  uint32_t oldest_heard_id; /* the running id with the smallest last_heard, lowest id on ties;
                               KB_CENSUS_NONE when nothing runs                                          */
  int32_t  oldest_heard;    /* its last_heard (INT32_MIN: unheard, or nothing runs)                      */
  uint32_t pad;
  uint64_t hist[KB_AGE_HIST];  /* windowed cells by age: bucket a holds age a                            */
  uint64_t reserved[4];
} kb_age_census;

/* Take the census.  Any of the arrays may be NULL; a non-NULL array must hold `capacity` elements (cap_ids for
 * suspected_by .. last_heard; cap_rows for suspects .. fresh), else KB_INVALID_ARGUMENT, as is out == NULL.
 *
 * KB_VARIANT_SPARSE_ROWS handles of kb_sim_create answer, and kb_sim_create_local groups of them (each shard passes
 * over its own rows; counts add, last_heard combines by max).  KB_INVALID_OPERATION, with a kb_last_error text, for
 * dense rows (text naming "dense") and for handles of kb_sim_create_rank (text naming "rank"). */
int kb_sim_age_census(kb_sim* sim, kb_age_census* out,
                      uint32_t* suspected_by, uint32_t* ancient_by, uint32_t* windowed_by, uint32_t* fresh_by,
                      int32_t* last_heard, size_t cap_ids,
                      uint32_t* suspects, uint32_t* ancient, uint32_t* windowed, uint32_t* fresh, size_t cap_rows);

/* Device time of the last kb_sim_age_census of this handle in ms (HIP events around its kernels and the clearing
 * of its scratch; the copies to the host and the O(ids) summary are not in it).  A group reports the sum over its
 * shards.  Measurement surface (tools/age_census_cost.py). */
int kb_sim_age_census_device_ms(kb_sim* sim, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* KABOODLE_AGE_H */
