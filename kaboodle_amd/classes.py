"""The fingerprint-class census in numpy: which camps the views fall into (include/kaboodle_classes.h).

`Sim.fp_classes()` (kaboodle_amd/_ffi.py) asks the HIP library's kb_sim_fp_classes, which groups on the device.
`fp_classes_ref` computes the same result from a handle's fingerprints, running flags and true fingerprint; it is
what `Sim.fp_classes()` falls back to for a library without kb_sim_fp_classes (the CPU oracle), so the oracle and
the GPU answer the same call.  `fp_classes_of_arrays` is the same computation on plain arrays.  Pure numpy: nothing
here needs a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._ffi import KB_CENSUS_NONE, diff_results

KB_FPC_LIST_MAX = 1024
SUMMARY_FIELDS = ("round", "observers", "classes", "largest", "singletons", "true_fp", "true_size", "true_rank",
                  "size_hist", "listed", "listed_observers")


@dataclass
class FpClasses:
    """One class census: `summary` (the fields of kb_fp_classes; size_hist a list of 32), `classes` (the first
    `top` classes in canonical order — size descending, then fingerprint ascending — as an [n, 3] uint32 array of
    fp, size, rep) and, over all ids, `rep` (the lowest id of the row's class, KB_CENSUS_NONE for rows that are not
    running) and `size` (its class's size, 0 for those rows); the two arrays are None with arrays=False."""
    summary: dict
    classes: np.ndarray
    rep: np.ndarray | None
    size: np.ndarray | None

    def same_as(self, other: "FpClasses") -> list[str]:
        """The differences to another class census (empty: identical summary, list and arrays)."""
        return diff_results(self, other, ("classes", "rep", "size"))


def fp_classes_of_arrays(fps, running, true_fp: int, top: int = 16, arrays: bool = True, round_: int = -1) -> FpClasses:
    """The class census of rows with fingerprints `fps` and running flags `running` (non-zero: an observer).
    Whether a row counts comes from `running` alone: a running row with fingerprint 0 is an observer, a stopped
    row's slot is ignored whatever it holds."""
    fps = np.asarray(fps, dtype=np.uint32)
    run = np.asarray(running) != 0
    n = len(fps)
    ids = np.flatnonzero(run)
    keys, first, inverse, counts = np.unique(fps[ids], return_index=True, return_inverse=True, return_counts=True)
    reps = ids[first] if len(ids) else np.zeros(0, dtype=np.int64)       # np.unique: the first occurrence = lowest id
    order = np.lexsort((keys, -counts.astype(np.int64)))                  # size descending, then fp ascending
    hist = [0] * 32
    for c in counts:
        hist[int(c).bit_length() - 1] += 1
    where = np.flatnonzero(keys[order] == np.uint32(true_fp))
    listed = order[:top]
    s = {"round": int(round_), "observers": int(len(ids)), "classes": int(len(keys)),
         "largest": int(counts.max()) if len(counts) else 0, "singletons": int((counts == 1).sum()),
         "true_fp": int(true_fp), "true_size": int(counts[order[where[0]]]) if len(where) else 0,
         "true_rank": int(where[0]) if len(where) else KB_CENSUS_NONE, "size_hist": hist,
         "listed": int(len(listed)), "listed_observers": int(counts[listed].sum())}
    cls = np.stack([keys[listed], counts[listed], reps[listed]], axis=1).astype(np.uint32) if len(listed) \
        else np.zeros((0, 3), dtype=np.uint32)
    if not arrays:
        return FpClasses(s, cls, None, None)
    rep = np.full(n, KB_CENSUS_NONE, dtype=np.uint32)
    size = np.zeros(n, dtype=np.uint32)
    rep[ids] = reps[inverse]
    size[ids] = counts[inverse]
    return FpClasses(s, cls, rep, size)


def fp_classes_ref(sim, top: int = 16, arrays: bool = True) -> FpClasses:
    """The class census of `sim` from `sim.fingerprints()`, column 0 of `sim.scalars()` (the running set) and the
    true fingerprint.  One fingerprint download and a sort on the host: the test and small-mesh path, and what the
    CPU oracle answers with.  On the GPU use Sim.fp_classes()."""
    return fp_classes_of_arrays(sim.fingerprints(), sim.scalars()[:, 0], sim.true_fingerprint(), top, arrays,
                                sim.stats()["round"])
