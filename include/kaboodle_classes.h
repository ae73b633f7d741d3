/*
 * kaboodle_classes.h — the fingerprint-class census of a simulated mesh: which camps the views fall into
 * (DESIGN.md §14).
 *
 * An extension of the C ABI of kaboodle_sim.h, implemented by the HIP library only (the CPU oracle answers the
 * same question through kaboodle_amd/classes.py's fp_classes_ref, from its fingerprints).  A peer decides whether
 * its view matches another's by comparing fingerprints; kb_stats.agree counts the rows that match the running
 * set's fingerprint and says nothing about the others.  This census groups the running rows by equal
 * fingerprint: two camps after a partition, one camp and a tail of stragglers, or every row alone.  The view
 * census (kaboodle_census.h) counts who knows whom and the reciprocity census (kaboodle_reciprocity.h) the gaps
 * between pairs; neither groups rows by equal view.  The grouping runs on the device over the fingerprints the
 * engines already keep there; it reads state and writes only its own scratch, so a run with a class census every
 * round computes exactly what a run without one computes.
 *
 * Definitions.  The census is taken on the state after the last completed round, with the running set that
 * kb_sim_fingerprints uses at that moment (lifecycle calls queued since the last step do not count yet).
 *   observer      a running row.  A running row whose fingerprint happens to be 0 is still an observer: whether
 *                 a row is one comes from the running flags, never from fp != 0
 *   fp(i)         what kb_sim_fingerprints reports for observer i
 *   class         a maximal set of observers with equal fp; its size is the number of observers in it, its
 *                 rep(resentative) its lowest id
 *   canonical order of the classes: size descending, then fp ascending
 */
#ifndef KABOODLE_CLASSES_H
#define KABOODLE_CLASSES_H

#include "kaboodle_census.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KB_FPC_LIST_MAX 1024u

typedef struct kb_fp_class {
  uint32_t fp;                /* the class's fingerprint                                            */
  uint32_t size;              /* observers in it                                                    */
  uint32_t rep;               /* its lowest id                                                      */
  uint32_t pad;
} kb_fp_class;

typedef struct kb_fp_classes {
  int32_t  round;             /* kb_stats.round when taken (-1 from kb_fp_classes_of)               */
  uint32_t observers;         /* running rows                                                       */
  uint32_t classes;           /* distinct fingerprints among them                                   */
  uint32_t largest;           /* size of the first class in canonical order (0 when there is none)  */
  uint32_t singletons;        /* classes of size 1                                                  */
  uint32_t true_fp;           /* what kb_sim_true_fingerprint reports                               */
  uint32_t true_size;         /* size of the class whose fp equals true_fp (0 if there is none).
                                 NOT kb_stats.agree: that field is taken at the ping step inside the
                                 round, before the waves; this one on the state after the round     */
  uint32_t true_rank;         /* that class's index in canonical order (KB_CENSUS_NONE if none)     */
  uint32_t size_hist[32];     /* size_hist[b] = classes with floor(log2(size)) == b                 */
  uint32_t listed;            /* entries written to `list` = min(classes, cap_list)                 */
  uint32_t listed_observers;  /* the sum of their sizes                                             */
  uint64_t reserved[4];
} kb_fp_classes;

/* Take the class census.  out == NULL is KB_INVALID_ARGUMENT.
 *
 * `list` receives the first min(classes, cap_list) classes in canonical order; *n_list (when n_list is not NULL)
 * and out->listed say how many.  cap_list may be 0 with list NULL; list NULL with cap_list > 0, and cap_list above
 * KB_FPC_LIST_MAX, are KB_INVALID_ARGUMENT.
 *
 * rep[i] and size[i], over all ids: the representative and the size of the class row i belongs to;
 * KB_CENSUS_NONE and 0 for rows that are not observers.  Either may be NULL; a non-NULL array must hold `capacity`
 * elements (cap_rows), else KB_INVALID_ARGUMENT.  Together the two arrays determine the whole partition, so no
 * caller needs a list longer than KB_FPC_LIST_MAX.
 *
 * Handles of kb_sim_create and kb_sim_create_local (dense or sparse rows) answer for the whole mesh; a group's
 * shards sit on one device, their fingerprints are gathered there.  Handles of kb_sim_create_rank return
 * KB_INVALID_OPERATION (kb_last_error says why): a class spans ranks and an inspection function makes no
 * collective call.
 *
 * The scratch (50 to 90 bytes of device memory per id of capacity: DESIGN.md §14) is allocated by the first call,
 * grown on demand and owned by the handle.
 */
int kb_sim_fp_classes(kb_sim* sim, kb_fp_classes* out, kb_fp_class* list, size_t cap_list, size_t* n_list,
                      uint32_t* rep, uint32_t* size, size_t cap_rows);

/* Device time of the last kb_sim_fp_classes of this handle in ms (HIP events around the clearing of its scratch,
 * the gather of a group's fingerprints and its kernels; the refresh of out-of-date fingerprints that
 * kb_sim_fingerprints would do as well, the running set's fingerprint and the copies to the host are not in it).
 * Measurement surface (tools/classes_cost.py). */
int kb_sim_fp_classes_device_ms(kb_sim* sim, double* ms);

/* The same kernels over a caller's host arrays of n fingerprints and running flags (running[i] != 0: row i is an
 * observer), with the caller's true_fp; round is reported as -1 and cap_rows is measured against n.  Needs no
 * handle; KB_NO_DEVICE without a GPU.  A test surface: it hands the kernels inputs that no simulated mesh
 * produces on demand. */
int kb_fp_classes_of(int device, const uint32_t* fps, const uint8_t* running, size_t n, uint32_t true_fp,
                     kb_fp_classes* out, kb_fp_class* list, size_t cap_list, size_t* n_list,
                     uint32_t* rep, uint32_t* size, size_t cap_rows);

#ifdef __cplusplus
}
#endif
#endif /* KABOODLE_CLASSES_H */
