"""The reciprocity census in numpy: one-way and mutual gaps between views (include/kaboodle_reciprocity.h).

`Sim.reciprocity()` (kaboodle_amd/_ffi.py) asks the HIP library's kb_sim_reciprocity, which counts on the device.
`reciprocity_ref` computes the same result from a handle's stamp rows and scalars; it is what `Sim.reciprocity()`
falls back to for a library without kb_sim_reciprocity (the CPU oracle), so the oracle and the GPU answer the same
call.  Pure numpy: nothing here needs a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._ffi import KB_CENSUS_NONE, diff_results

SUMMARY_FIELDS = ("round", "observers", "mutual_pairs", "oneway_pairs", "rows_mutual", "rows_oneway",
                  "max_mutual_row", "max_mutual", "pairs_listed")


@dataclass
class Reciprocity:
    """One reciprocity census: `summary` (the fields of kb_reciprocity) and, over all ids, `mutual` (peers the row
    lacks that lack it too), `lacks` (peers it lacks that still hold it) and `lacked_by` (peers it holds that lack
    it); uint32 arrays, or None when only the summary was asked for.  `pairs`: the mutual pairs as an [n, 2] uint32
    array of (i, j), i < j, ascending; empty when there is none or the total is above the caller's max_pairs
    (summary["pairs_listed"] tells which), None with arrays=False."""
    summary: dict
    mutual: np.ndarray | None
    lacks: np.ndarray | None
    lacked_by: np.ndarray | None
    pairs: np.ndarray | None

    def same_as(self, other: "Reciprocity") -> list[str]:
        """The differences to another reciprocity census (empty: identical summary, arrays and pair list)."""
        return diff_results(self, other, ("mutual", "lacks", "lacked_by", "pairs"))


def summarize(round_: int, observers: np.ndarray, mutual: np.ndarray, lacks: np.ndarray, pairs_listed: int) -> dict:
    """The summary fields from the arrays (observers: bool per id)."""
    s = {"round": int(round_), "observers": int(observers.sum()),
         "mutual_pairs": int(mutual.sum(dtype=np.uint64)) // 2, "oneway_pairs": int(lacks.sum(dtype=np.uint64)),
         "rows_mutual": int((mutual > 0).sum()), "rows_oneway": int((lacks > 0).sum())}
    if mutual.any():
        k = int(np.argmax(mutual))                        # argmax: the first (lowest id) of the largest
        s["max_mutual_row"], s["max_mutual"] = k, int(mutual[k])
    else:
        s["max_mutual_row"], s["max_mutual"] = KB_CENSUS_NONE, 0
    s["pairs_listed"] = int(pairs_listed)
    return s


def reciprocity_ref(sim, max_pairs: int = 65536, arrays: bool = True) -> Reciprocity:
    """The reciprocity census of `sim` from `sim.row()` of every running row and `sim.scalars()`: a row entry != 0
    is a member, column 0 of the scalars is the running set.  The handle must hold every row.  arrays=False gives
    what Sim.reciprocity(arrays=False) gives on the device: the summary alone, nothing listed (pairs_listed 0).

    A test and small-mesh path only: it builds the whole bool matrix on the host, O(N^2) bytes over the bus.  On
    the GPU use Sim.reciprocity()."""
    C = sim.capacity
    running = sim.scalars()[:, 0] != 0
    B = np.zeros((C, C), dtype=bool)
    for i in np.flatnonzero(running):
        B[i] = sim.row(int(i)) != 0
    pair = running[:, None] & running[None, :] & ~np.eye(C, dtype=bool)     # observers i != j
    gap = pair & ~B                                                          # i lacks j
    both = gap & gap.T
    mutual = both.sum(axis=1).astype(np.uint32)
    lacks = (gap & B.T).sum(axis=1).astype(np.uint32)
    lacked_by = (pair & B & ~B.T).sum(axis=1).astype(np.uint32)
    if not arrays:
        return Reciprocity(summarize(sim.stats()["round"], running, mutual, lacks, 0), None, None, None, None)
    n_pairs = int(mutual.sum(dtype=np.uint64)) // 2
    listed = 0 < n_pairs <= max_pairs
    pairs = np.argwhere(np.triu(both, 1)).astype(np.uint32) if listed else np.zeros((0, 2), dtype=np.uint32)
    s = summarize(sim.stats()["round"], running, mutual, lacks, len(pairs))
    return Reciprocity(s, mutual, lacks, lacked_by, pairs)
