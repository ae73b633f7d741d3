"""The gap list and the holders query in numpy: which rows lack or hold which ids (include/kaboodle_gaps.h).

`Sim.gaps()` and `Sim.holders()` (kaboodle_amd/_ffi.py) ask the HIP library's kb_sim_gaps and kb_sim_holders, which
list on the device.  `gaps_ref` and `holders_ref` compute the same results from the `row()` tables, a running set and
the external ids; `gaps_of_sim` / `holders_of_sim` feed them a handle's rows and scalars and are what the two methods
fall back to for a library without the exports (the CPU oracle), so the oracle and the GPU answer the same calls.
Pure numpy: nothing here needs a GPU.
"""
from __future__ import annotations

import numpy as np

SUMMARY_FIELDS = ("round", "observers", "missing", "stale", "missing_listed", "stale_listed", "rows_missing",
                  "rows_stale")
KB_HOLDERS_MAX = 1024


def _tables(rows, running, external=None):
    run = np.asarray(running) != 0
    C = len(run)
    B = np.asarray(rows)[:C, :C] != 0
    ext = np.zeros(C, dtype=bool) if external is None else np.asarray(external) != 0
    return B, run, ext


def gaps_ref(rows, running, external=None, round_: int = -1, max_pairs: int | None = None) -> dict:
    """The gap list from its definitions.  rows: [C][>= C], an entry != 0 means the row's id holds the column's
    (columns at ids >= C are ignored; rows of ids that do not run are not read); running, external: per id ([C]).
    Returns the fields of kb_gaps and `missing_pairs` / `stale_pairs`: (n, 2) uint32 arrays of (row, id), ascending,
    or None for a list of more than max_pairs pairs (None: no limit)."""
    B, run, ext = _tables(rows, running, external)
    miss = run[:, None] & run[None, :] & ~B                            # an observer lacks a running id
    stale = run[:, None] & B & (~run & ~ext)[None, :]                  # an observer holds an id that is gone
    out = {"round": int(round_), "observers": int(run.sum()), "missing": int(miss.sum()), "stale": int(stale.sum())}
    lists = {}
    for name, m in (("missing", miss), ("stale", stale)):
        listed = max_pairs is None or out[name] <= max_pairs
        out[name + "_listed"] = out[name] if listed else 0
        lists[name + "_pairs"] = np.argwhere(m).astype(np.uint32).reshape(-1, 2) if listed else None   # row-major
    out["rows_missing"], out["rows_stale"] = int(miss.any(axis=1).sum()), int(stale.any(axis=1).sum())
    return {**out, **lists}


def holders_ref(rows, running, ids, max_rows: int | None = None):
    """The holders of each id of `ids` from the definitions: (offsets, rows).  offsets: uint64 [len(ids) + 1]; rows:
    uint32, query q's observers ascending at rows[offsets[q]:offsets[q + 1]], or None when there are more than
    max_rows of them (None: no limit)."""
    B, run, _ = _tables(rows, running)
    cols = [np.flatnonzero(B[:, int(j)] & run).astype(np.uint32) for j in ids]
    off = np.zeros(len(cols) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in cols], dtype=np.uint64)
    if max_rows is not None and int(off[-1]) > max_rows:
        return off, None
    return off, np.concatenate(cols) if cols else np.zeros(0, dtype=np.uint32)


def host_tables(sim):
    """(rows, running, external) of `sim` from `sim.row()` of every running row and `sim.scalars()`.  The handle must
    hold every row.  A test and small-mesh path only: O(N^2) bytes over the bus."""
    C = sim.capacity
    running = sim.scalars()[:, 0] != 0
    B = np.zeros((C, C), dtype=bool)
    for i in np.flatnonzero(running):
        B[i] = sim.row(int(i)) != 0
    ext = np.zeros(C, dtype=bool)
    ext[list(sim.external)] = True
    return B, running, ext


def gaps_of_sim(sim, max_pairs: int = 65536) -> dict:
    """Sim.gaps() for a library without kb_sim_gaps."""
    B, running, ext = host_tables(sim)
    return gaps_ref(B, running, ext, sim.stats()["round"], max_pairs)


def holders_of_sim(sim, ids, max_rows: int | None = None):
    """Sim.holders() for a library without kb_sim_holders."""
    ids = [int(j) for j in ids]
    if not 1 <= len(ids) <= KB_HOLDERS_MAX or any(not 0 <= j < sim.capacity for j in ids):
        raise ValueError("holders: 1 .. KB_HOLDERS_MAX ids, each below the capacity")
    B, running, _ = host_tables(sim)
    return holders_ref(B, running, ids, max_rows)


def same_gaps(a: dict, b: dict) -> list[str]:
    """The differences between two gaps() results (empty: identical summary and lists)."""
    out = [f"{k}: {a[k]} != {b[k]}" for k in SUMMARY_FIELDS if a[k] != b[k]]
    for k in ("missing_pairs", "stale_pairs"):
        x, y = a[k], b[k]
        if (x is None) != (y is None):
            out.append(f"{k}: listed on one side only")
        elif x is not None and (x.shape != y.shape or not np.array_equal(x, y)):
            out.append(f"{k}: {len(x)} pairs != {len(y)} pairs, or other entries")
    return out
