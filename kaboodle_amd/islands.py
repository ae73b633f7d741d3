"""The island census in numpy: which peers can still reach each other (include/kaboodle_islands.h).

`Sim.islands()` (kaboodle_amd/_ffi.py) asks the HIP library's kb_sim_islands, which labels the connected components
of the "i holds j" graph on the device.  `islands_ref` computes the same result from a bool member matrix and a
running set with a plain union-find; `islands_of_sim` feeds it a handle's stamp rows and scalars and is what
`Sim.islands()` falls back to for a library without kb_sim_islands (the CPU oracle), so the oracle and the GPU answer
the same call.  Pure numpy: nothing here needs a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._ffi import KB_CENSUS_NONE, diff_results

KB_ISLANDS_TOP = 8
SUMMARY_FIELDS = ("round", "observers", "islands", "singletons", "rebroadcasting", "largest", "largest_label",
                  "second", "unreachable_pairs", "top", "sweeps")
ARRAYS = ("label", "size")


@dataclass
class Islands:
    """One island census: `summary` (the fields of kb_islands; `top` as a list of [label, size]) and, over all ids,
    `label` (the lowest id of the id's island, KB_CENSUS_NONE where the id does not run) and `size` (the observers
    of its island, 0 where it does not run); uint32 arrays, or None when only the summary was asked for."""
    summary: dict
    label: np.ndarray | None
    size: np.ndarray | None

    def same_as(self, other: "Islands") -> list[str]:
        """The differences to another island census (empty: identical summary and arrays).  `sweeps` is a property
        of the execution, not of the state, and is not compared."""
        strip = lambda r: Islands({k: v for k, v in r.summary.items() if k != "sweeps"}, r.label, r.size)
        return diff_results(strip(self), strip(other), ARRAYS)


def summarize(round_: int, label: np.ndarray, size: np.ndarray, entries: np.ndarray, sweeps: int = 0) -> dict:
    """The summary fields from the arrays (entries: the number of ids each row holds)."""
    heads = np.flatnonzero(label == np.arange(len(label)))            # one id per island: its label
    sz = size[heads].astype(np.int64)
    order = sorted(range(len(heads)), key=lambda k: (-sz[k], heads[k]))
    obs = int(sz.sum())
    top = [[int(heads[k]), int(sz[k])] for k in order[:KB_ISLANDS_TOP]]
    single = heads[sz == 1]
    return {"round": int(round_), "observers": obs, "islands": len(heads), "singletons": len(single),
            "rebroadcasting": int((entries[single] <= 1).sum()),
            "largest": top[0][1] if top else 0, "largest_label": top[0][0] if top else KB_CENSUS_NONE,
            "second": top[1][1] if len(top) > 1 else 0,
            "unreachable_pairs": int(sum(int(n) * (obs - int(n)) for n in sz)),
            "top": top + [[KB_CENSUS_NONE, 0]] * (KB_ISLANDS_TOP - len(top)), "sweeps": int(sweeps)}


def islands_ref(member, running, round_: int = -1, arrays: bool = True) -> Islands:
    """The island census from its definitions.  member: [C][>= C], an entry != 0 means the row's id holds the
    column's (columns at ids >= C are ignored); running: per id ([C]).  A union-find over the edges of B | B.T between
    running ids, each set named by its lowest id."""
    run = np.asarray(running) != 0
    C = len(run)
    B = np.asarray(member)[:C, :C] != 0
    parent = list(range(C))

    def find(x: int) -> int:
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in np.argwhere(B & run[:, None] & run[None, :]):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)                              # the lower id stays the root
    label = np.full(C, KB_CENSUS_NONE, dtype=np.uint32)
    for j in np.flatnonzero(run):
        label[j] = find(int(j))
    size = np.zeros(C, dtype=np.uint32)
    counts = np.bincount(label[run], minlength=C) if run.any() else np.zeros(C, dtype=np.int64)
    size[run] = counts[label[run]]
    s = summarize(round_, label, size, B.sum(axis=1))
    return Islands(s, label, size) if arrays else Islands(s, None, None)


def islands_of_sim(sim, arrays: bool = True) -> Islands:
    """The island census of `sim` from `sim.row()` of every running row and `sim.scalars()`: a row entry != 0 is a
    member, column 0 of the scalars is the running set.  The handle must hold every row.

    A test and small-mesh path only: it builds the whole bool matrix on the host, O(N^2) bytes over the bus.  On the
    GPU use Sim.islands()."""
    C = sim.capacity
    running = sim.scalars()[:, 0] != 0
    B = np.zeros((C, C), dtype=bool)
    for i in np.flatnonzero(running):
        B[i] = sim.row(int(i)) != 0
    return islands_ref(B, running, sim.stats()["round"], arrays)
