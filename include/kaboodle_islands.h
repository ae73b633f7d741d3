/*
 * kaboodle_islands.h — the island census of a simulated mesh: which peers can still reach each other
 * (DESIGN.md §20).
 *
 * An extension of the C ABI of kaboodle_sim.h, implemented by the HIP library only (the CPU oracle answers the
 * same question through kaboodle_amd/islands.py's islands_ref, from its stamp rows).  The other censuses describe
 * the views as they stand; this one says whether the mesh can still converge at all.  Unicast goes only to members
 * of the sender's own view, every envelope inserts its sender at the receiver (so a one-way edge becomes mutual at
 * the first ping that arrives), KnownPeers carries knowledge only along such edges, and a peer broadcasts Join again
 * only while it knows nobody but itself.  So the weakly connected components of the "i holds j" graph over the
 * running peers are ISLANDS: with no new joiner, restart, ping_addrs or external peer, two islands never learn of
 * each other again; the one exception is a peer whose view is down to itself.
 *
 * The census is a few streaming passes on the device over the member bits.  It reads the mesh's state and writes
 * only its own scratch, so a run with an island census every round computes exactly what a run without one
 * computes.  Nothing is allocated or launched unless these calls are made.
 *
 * Definitions.  The state is the one after the last completed round, with the running set kb_sim_census uses
 * (lifecycle calls queued since the last step do not count yet).
 *   observer   a running row
 *   edge       between i and j whenever i and j both run, i != j, and j is in view(i) OR i is in view(j).  Rows of
 *              ids that do not run are masked out as rows and as columns (two groups joined only through a stopped
 *              id are two islands); external ids never run and appear nowhere; padding columns >= capacity count
 *              nowhere
 *   island     a connected component of that graph.  Its LABEL is its lowest id, which makes the result a function
 *              of the state alone, whatever order the device works in
 *   label[j]   for every id j < capacity: the label of j's island; KB_CENSUS_NONE when j does not run
 *   size[j]    the number of observers in j's island; 0 when j does not run
 */
#ifndef KABOODLE_ISLANDS_H
#define KABOODLE_ISLANDS_H

#include "kaboodle_census.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KB_ISLANDS_TOP 8   /* islands listed in kb_islands.top */

typedef struct kb_islands {
  int32_t  round;           /* kb_stats.round when taken                                              */
  uint32_t observers;       /* running rows                                                           */
  uint32_t islands;         /* connected components among them                                        */
  uint32_t singletons;      /* islands of size 1                                                      */
  uint32_t rebroadcasting;  /* singletons whose row holds at most itself (kb_sim_peers reports <= 1
                               entries): the peers that broadcast Join again                          */
  uint32_t largest;         /* the size of the largest island; 0 without observers                    */
  uint32_t largest_label;   /* its label (the lowest label on ties); KB_CENSUS_NONE without observers */
  uint32_t second;          /* the size of the second largest island; 0 when there is none            */
  uint64_t unreachable_pairs;   /* ordered pairs of observers in different islands:
                                   sum over islands of size * (observers - size)                      */
  uint32_t top[KB_ISLANDS_TOP][2];   /* (label, size) by size descending, then label ascending; padded
                                        with (KB_CENSUS_NONE, 0)                                      */
  uint32_t sweeps;          /* device sweeps the call took (the last one changed nothing).  A property of
                               the execution, not of the state: it may differ between two calls on the
                               same state and is no part of any reference result                      */
  uint32_t pad;
  uint64_t reserved[4];
} kb_islands;

/* Take the island census.  label and size may be NULL; a non-NULL array must hold `capacity` elements (cap_ids),
 * else KB_INVALID_ARGUMENT; out == NULL is KB_INVALID_ARGUMENT.
 *
 * Dense handles of kb_sim_create (either A3 order) and of kb_sim_create_local answer: a group's shards live on one
 * device, their streams are drained first, and one launch reads every shard's rows through a table of at most 8
 * bases in its arguments; there is one label array for the whole mesh.  Sparse rows and handles of
 * kb_sim_create_rank answer KB_INVALID_OPERATION, sparse rows first.  KB_IO_ERROR if the labels have not settled
 * after capacity + 1 sweeps (the sum of the labels strictly decreases with every sweep that changes one, so this
 * cannot happen). */
int kb_sim_islands(kb_sim* sim, kb_islands* out, uint32_t* label, uint32_t* size, size_t cap_ids);

/* Device time of the last kb_sim_islands of this handle in ms (HIP events around the first and the last kernel: the
 * host's 4-byte read of the "changed" word between two sweeps is inside the span; the download of the labels and the
 * O(ids) summary are not); 0 before the first answer.  Measurement surface (tools/islands_cost.py). */
int kb_sim_islands_device_ms(kb_sim* sim, double* ms);

/* Test surface: the island census's kernels over host arrays, no mesh.  bits: the member bits of all `capacity`
 * rows, [capacity][W/32] words with W = capacity rounded up to 8192 (bit j & 31 of word j >> 5 is id j; bits at ids
 * >= capacity and rows of ids that do not run are ignored).  running: a byte per id, [capacity].  Outputs as
 * kb_sim_islands (round is -1).  KB_NO_DEVICE without a GPU. */
int kb_islands_of(int device, const uint32_t* bits, const uint8_t* running, size_t capacity, kb_islands* out,
                  uint32_t* label, uint32_t* size, size_t cap_ids);

#ifdef __cplusplus
}
#endif
#endif /* KABOODLE_ISLANDS_H */
