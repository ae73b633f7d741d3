"""The gap list and the holders query on the GPU (kb_sim_gaps / kb_sim_holders, include/kaboodle_gaps.h; kernels in
kaboodle_amd/csrc/kb_gaps.h).  The reference is gaps_ref / holders_ref over the CPU oracle's rows, in lock step (GPU =
oracle is established by the parity suite): every round of four scenarios, unsharded and as 2 and 3 shards; long rows;
ids on word, lane, pass and capacity edges; the caps; the zero case; external ids; the identities against
kb_sim_census; read-only; the refusals."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import parity
import scenarios
from kaboodle_amd._ffi import (KB_HOLDERS_MAX, KB_INIT_CONVERGED, KB_INVALID_ARGUMENT, KB_INVALID_OPERATION,
                               KB_VARIANT_SPARSE_ROWS, KbError, KbGaps, Sim, SimConfig, rccl_unique_id)
from kaboodle_amd.gaps import SUMMARY_FIELDS, gaps_ref, holders_ref, host_tables, same_gaps

pytestmark = pytest.mark.gpu

K_JOIN = 16                                                            # Sim.inject: an external peer's Join broadcast
P32, P64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


SYMBOLS = ("sim_gaps", "sim_gaps_device_ms", "sim_holders", "sim_holders_device_ms")


def has_kernel(lib) -> None:
    # the numpy fallback cannot stand in for the kernels
    assert all(n in lib.fn for n in SYMBOLS)


def test_exports(gpu):
    has_kernel(gpu)
    for n in ("kb_sim_gaps", "kb_sim_gaps_device_ms", "kb_sim_holders", "kb_sim_holders_device_ms",
              "kb_sim_census", "kb_sim_census_device_ms"):             # and the yardstick the tests compare with
        assert getattr(gpu.lib, n) is not None


def reference(o: Sim, ids) -> tuple:
    """(gaps, holders offsets, holders rows) of the oracle's state through the references, every pair listed."""
    rows, run, ext = host_tables(o)
    off, who = holders_ref(rows, run, ids)
    return gaps_ref(rows, run, ext, o.stats()["round"]), off, who


def answer(g: Sim, ids) -> tuple:
    gp = g.gaps(max_pairs=g.capacity ** 2)
    off, who = g.holders(ids)
    return gp, off, who


def differences(got: tuple, want: tuple) -> list[str]:
    d = same_gaps(got[0], want[0])
    if not np.array_equal(got[1], want[1]):
        d.append("holders: offsets differ")
    elif got[2] is None or not np.array_equal(got[2], want[2]):
        d.append("holders: rows differ")
    return d


def raw(x: tuple) -> bytes:
    return b"".join([repr([x[0][k] for k in SUMMARY_FIELDS]).encode(), x[0]["missing_pairs"].tobytes(),
                     x[0]["stale_pairs"].tobytes(), x[1].tobytes(), x[2].tobytes()])


_ORACLE: dict = {}


def oracle_rounds(name: str):
    """The reference after every round of the scenario, holders of every id: computed once, shared, never changed."""
    if name not in _ORACLE:
        sc = scenarios.BY_NAME[name]
        out = []
        with Sim(parity.oracle_lib(), sc["cfg"]) as o:
            scenarios.setup(o, sc)
            for r in range(sc["rounds"]):
                scenarios.apply_events(o, sc, r)
                o.step(1)
                out.append(reference(o, range(o.capacity)))
        _ORACLE[name] = out
    return _ORACLE[name]


NONZERO = {"stop_start": ("missing", "stale"), "partition": ("missing",), "churn40": ("missing", "stale"),
           "old_stamps": ("missing", "stale")}                         # partition stops nobody: nothing can be stale


@pytest.mark.parametrize("name", list(NONZERO))
def test_every_round_against_the_reference(gpu, name):
    """Capacities 24, 32, 60 and 160: holders of every id in one call.  Unsharded, 2 shards and 3 shards in lock step:
    the unsharded answer equals the reference, the groups' bytes equal the unsharded answer's."""
    has_kernel(gpu)
    sc = scenarios.BY_NAME[name]
    want = oracle_rounds(name)
    ids = range(sc["cfg"].capacity)
    with Sim(gpu, sc["cfg"]) as g0, Sim(gpu, sc["cfg"], shards=2) as g2, Sim(gpu, sc["cfg"], shards=3) as g3:
        for g in (g0, g2, g3):
            scenarios.setup(g, sc)
        for r in range(sc["rounds"]):
            for g in (g0, g2, g3):
                scenarios.apply_events(g, sc, r)
                g.step(1)
            got = answer(g0, ids)
            d = differences(got, want[r])
            assert not d, f"{name} round {r}: " + "; ".join(d[:6])
            assert raw(answer(g2, ids)) == raw(got), f"{name} round {r}: 2 shards"
            assert raw(answer(g3, ids)) == raw(got), f"{name} round {r}: 3 shards"
    for kind in NONZERO[name]:                                         # else the case shows nothing
        assert any(w[0][kind] > 0 for w in want), kind
    assert any(len(w[2]) > 0 for w in want)


assert all(any(kind in v for v in NONZERO.values()) for kind in ("missing", "stale"))


def lockstep(gpu, sc: dict, rounds: int, ids, before=None, at_round=None):
    """The scenario on the oracle and the GPU side by side; yields (round, gpu handle, oracle handle) after each step."""
    with Sim(parity.oracle_lib(), sc["cfg"]) as o, Sim(gpu, sc["cfg"]) as g:
        for s in (o, g):
            scenarios.setup(s, sc)
            if before:
                before(s)
        for r in range(rounds):
            for s in (o, g):
                scenarios.apply_events(s, sc, r)
                if at_round:
                    at_round(s, r)
                s.step(1)
            yield r, g, o


def test_long_rows_and_many_rows(gpu):
    """trunc_join: 700 peers joining, after rounds 1 and 2.  After the first every row lacks 699 ids (more than a wave
    of lanes holds) and the scan crosses all 700 rows; the whole list, 489,300 pairs, is compared."""
    has_kernel(gpu)
    sc = scenarios.BY_NAME["trunc_join"]
    ids = list(range(0, 700, 7))
    for r, g, o in lockstep(gpu, sc, 2, ids):
        want = reference(o, ids)
        d = differences(answer(g, ids), want)
        assert not d, f"round {r}: " + "; ".join(d[:6])
        if r == 0:                                                     # the second round's Join responses fill the views
            per_row = np.bincount(want[0]["missing_pairs"][:, 0], minlength=700)
            assert want[0]["rows_missing"] == 700 and per_row.min() > 100 and want[0]["missing"] > 65536


EDGE_STOP = [0, 31, 32, 63, 64, 8191, 8192, 8199]
EDGE_LATE = [8190, 8191, 8192, 8198, 8199]
EDGE_IDS = [0, 1, 31, 32, 63, 64, 8190, 8191, 8192, 8198, 8199]


@pytest.mark.parametrize("what", ["stale", "missing"])
def test_boundaries(gpu, what):
    """Capacity 8,200: W = 16,384, so two 8,192-id wave passes per row and a partial last word.  Converged start, 2
    rounds, both lists and the holders of eleven ids on word, lane, pass and capacity edges.

    stale: all 8,200 run; ids 0, 31, 32, 63, 64, 8191, 8192 and 8199 are stopped before round 0 and stay in the views.
    missing: a converged start binds ids 0 .. initial_nodes - 1 and a stopped instance restarts at a fresh address
    (kb_sim_start_node refuses it), so a low id cannot be left unstarted; the ids that start late are 8190, 8191, 8192,
    8198 and 8199 of a mesh of 8,190, started before round 1: both sides of the pass edge and the capacity edge."""
    has_kernel(gpu)
    if what == "stale":
        sc = {"cfg": SimConfig(capacity=8200, initial_nodes=8200, init_mode=KB_INIT_CONVERGED, seed=41), "identities": {},
              "start": [], "events": {0: [("stop", j, None) for j in EDGE_STOP]}}
    else:
        sc = {"cfg": SimConfig(capacity=8200, initial_nodes=8190, init_mode=KB_INIT_CONVERGED, seed=42), "identities": {},
              "start": [], "events": {1: [("start", j, None) for j in EDGE_LATE]}}
    seen = set()
    for r, g, o in lockstep(gpu, sc, 2, EDGE_IDS):
        want = reference(o, EDGE_IDS)
        d = differences(answer(g, EDGE_IDS), want)
        assert not d, f"round {r}: " + "; ".join(d[:6])
        seen |= set(np.unique(want[0][what + "_pairs"][:, 1]).tolist())
    assert seen >= set(EDGE_STOP if what == "stale" else EDGE_LATE), seen


def state_with_both(gpu):
    """A churn40 mesh stepped to the first round at which the oracle shows missing and stale cells at once."""
    want = oracle_rounds("churn40")
    r0 = next(r for r, w in enumerate(want) if w[0]["missing"] > 1 and w[0]["stale"] > 1)
    sc = scenarios.BY_NAME["churn40"]
    g = Sim(gpu, sc["cfg"])
    scenarios.setup(g, sc)
    for r in range(r0 + 1):
        scenarios.apply_events(g, sc, r)
        g.step(1)
    return g, want[r0]


def call_gaps(g: Sim, cap_m: int, cap_s: int):
    out = KbGaps()
    bm, bs = (np.full((max(c, 1), 2), SENTINEL, dtype=np.uint32) for c in (cap_m, cap_s))
    g.lib.call("sim_gaps", g.h, C.byref(out), bm.ctypes.data_as(P32) if cap_m else None, cap_m,
               bs.ctypes.data_as(P32) if cap_s else None, cap_s)
    return out.as_dict(), bm, bs


def test_caps(gpu):
    has_kernel(gpu)
    g, want = state_with_both(gpu)
    with g:
        gw = want[0]
        nm, ns = gw["missing"], gw["stale"]
        totals = {k: gw[k] for k in SUMMARY_FIELDS if not k.endswith("_listed")}
        s, bm, bs = call_gaps(g, nm, ns)                               # cap == total: written
        assert s == {k: gw[k] for k in SUMMARY_FIELDS}
        assert np.array_equal(bm[:nm], gw["missing_pairs"]) and np.array_equal(bs[:ns], gw["stale_pairs"])
        s, bm, bs = call_gaps(g, nm - 1, ns)                           # one short: that list alone is not written
        assert {k: s[k] for k in totals} == totals and s["missing_listed"] == 0 and s["stale_listed"] == ns
        assert (bm == SENTINEL).all() and np.array_equal(bs[:ns], gw["stale_pairs"])
        s, bm, bs = call_gaps(g, nm + 3, ns - 1)
        assert {k: s[k] for k in totals} == totals and s["missing_listed"] == nm and s["stale_listed"] == 0
        assert (bs == SENTINEL).all() and np.array_equal(bm[:nm], gw["missing_pairs"]) and (bm[nm:] == SENTINEL).all()
        s, bm, bs = call_gaps(g, 0, 0)                                 # totals only
        assert {k: s[k] for k in totals} == totals and s["missing_listed"] == s["stale_listed"] == 0
        py = g.gaps(max_pairs=max(nm, ns) - 1)                         # the Python surface: None for the longer list
        assert (py["missing_pairs"] is None) == (nm >= ns) and (py["stale_pairs"] is None) == (ns >= nm)
        # the holders' rows buffer
        ids = np.arange(g.capacity, dtype=np.uint32)
        total = len(want[2])
        assert total > 0
        for cap in (total, total - 1):
            off = np.zeros(len(ids) + 1, dtype=np.uint64)
            rows = np.full(total, SENTINEL, dtype=np.uint32)
            n = C.c_uint64(0)
            g.lib.call("sim_holders", g.h, ids.ctypes.data_as(P32), len(ids), off.ctypes.data_as(P64),
                       rows.ctypes.data_as(P32), cap, C.byref(n))
            assert n.value == total and np.array_equal(off, want[1])
            assert np.array_equal(rows, want[2]) if cap == total else (rows == SENTINEL).all()
        off = np.zeros(len(ids) + 1, dtype=np.uint64)                  # offsets alone; n_rows may be NULL
        g.lib.call("sim_holders", g.h, ids.ctypes.data_as(P32), len(ids), off.ctypes.data_as(P64), None, 0, None)
        assert np.array_equal(off, want[1])
        assert g.holders(ids, max_rows=total - 1)[1] is None


def test_zero_case(gpu):
    has_kernel(gpu)
    cfg = SimConfig(capacity=100, initial_nodes=100, init_mode=KB_INIT_CONVERGED, seed=3)
    with Sim(gpu, cfg) as g:
        g.step(2)
        s, bm, bs = call_gaps(g, 50, 50)
        assert s == {"round": 2, "observers": 100, "missing": 0, "stale": 0, "missing_listed": 0, "stale_listed": 0,
                     "rows_missing": 0, "rows_stale": 0}
        assert (bm == SENTINEL).all() and (bs == SENTINEL).all()
        py = g.gaps()
        assert py["missing_pairs"].shape == py["stale_pairs"].shape == (0, 2)
        off, who = g.holders(range(100))
        assert np.array_equal(off, np.arange(101, dtype=np.uint64) * 100)
        assert np.array_equal(who.reshape(100, 100), np.tile(np.arange(100, dtype=np.uint32), (100, 1)))


def test_externals_dead_and_unheld_ids(gpu):
    """Id 35 is external and broadcasts Join: every view takes it in, neither gap list names it, its holders are
    answered.  Id 5 is stopped (dead, still held); id 39 never ran and nobody holds it."""
    has_kernel(gpu)
    sc = {"cfg": SimConfig(capacity=40, initial_nodes=32, init_mode=KB_INIT_CONVERGED, seed=12), "identities": {},
          "start": [], "events": {1: [("stop", 5, None)]}}
    ids = [35, 5, 39, 0]

    def join(s, r):
        if r == 1:
            s.inject(35, 0, K_JOIN)

    held = 0
    for r, g, o in lockstep(gpu, sc, 4, ids, before=lambda s: s.set_external(35), at_round=join):
        want = reference(o, ids)
        got = answer(g, ids)
        d = differences(got, want)
        assert not d, f"round {r}: " + "; ".join(d[:6])
        for k in ("missing_pairs", "stale_pairs"):
            assert 35 not in got[0][k][:, 1]
        assert got[1][3] == got[1][2]                                  # nobody holds 39: an empty slice
        held = max(held, int(got[1][1] - got[1][0]))
        last = got
    assert held > 16                                                   # the external id sits in most views
    assert last[1][2] - last[1][1] > 0 and (last[0]["stale_pairs"][:, 1] == 5).any()   # the dead id: held, and stale


def test_identities_with_the_view_census(gpu):
    """On one handle (trunc_odd: capacity 1,300, so KB_HOLDERS_MAX ids in one call and a second call for the rest)."""
    has_kernel(gpu)
    sc = scenarios.BY_NAME["trunc_odd"]
    with Sim(gpu, sc["cfg"]) as g:
        scenarios.setup(g, sc)
        g.step(3)
        cap = g.capacity
        c = g.census()
        gp = g.gaps(max_pairs=cap * cap)
        assert (gp["missing"], gp["stale"], gp["observers"], gp["round"]) == (
            c.summary["missing"], c.summary["stale"], c.summary["observers"], c.summary["round"])
        assert gp["missing"] > 0 and gp["stale"] > 0
        for kind, arr in (("missing", c.missing), ("stale", c.stale)):
            assert np.array_equal(np.bincount(gp[kind + "_pairs"][:, 0], minlength=cap), arr), kind
            assert gp["rows_" + kind] == int((arr > 0).sum())
        off_a, who_a = g.holders(range(KB_HOLDERS_MAX))
        off_b, who_b = g.holders(range(KB_HOLDERS_MAX, cap))
        assert np.array_equal(np.concatenate([np.diff(off_a), np.diff(off_b)]).astype(np.uint32), c.known_by)
        rng = np.random.default_rng(8)
        for j in rng.choice(cap, 32, replace=False):
            off1, who1 = g.holders([int(j)])
            a, w = (off_a, who_a) if j < KB_HOLDERS_MAX else (off_b, who_b)
            q = int(j) % KB_HOLDERS_MAX
            assert np.array_equal(who1, w[int(a[q]):int(a[q + 1])]) and off1.tolist() == [0, len(who1)], j
        off2, who2 = g.holders([7, 1299, 7])                          # a duplicate is answered twice
        assert np.array_equal(who2[: int(off2[1])], who2[int(off2[2]):]) and off2[1] - off2[0] == off2[3] - off2[2] == c.known_by[7]


def test_read_only(gpu):
    has_kernel(gpu)
    sc = scenarios.BY_NAME["churn40"]
    with Sim(gpu, sc["cfg"]) as a, Sim(gpu, sc["cfg"]) as b:
        for r in range(15):
            for s in (a, b):
                scenarios.apply_events(s, sc, r)
                s.step(1)
            first = a.gaps()
            assert not same_gaps(a.gaps(), first)                      # the same again
            a.holders(range(a.capacity))
            assert scenarios.digest_sim(a) == scenarios.digest_sim(b), r
        assert not a.census().same_as(b.census())


def test_arguments_and_refusals(gpu):
    has_kernel(gpu)
    sc = scenarios.BY_NAME["stop_start"]
    cap = sc["cfg"].capacity
    buf = np.zeros((8, 2), dtype=np.uint32)
    ptr = buf.ctypes.data_as(P32)
    off = np.zeros(KB_HOLDERS_MAX + 2, dtype=np.uint64)
    ids = np.zeros(KB_HOLDERS_MAX + 1, dtype=np.uint32)
    ip, op = ids.ctypes.data_as(P32), off.ctypes.data_as(P64)
    with Sim(gpu, sc["cfg"]) as g:
        g.step(2)
        assert g.gaps_device_ms() == 0.0 and g.holders_device_ms() == 0.0
        out = KbGaps()
        bad = [("sim_gaps", (None, None, 0, None, 0)),                 # out == NULL
               ("sim_gaps", (C.byref(out), ptr, 0, None, 0)),          # a list with capacity 0
               ("sim_gaps", (C.byref(out), None, 8, None, 0)),         # a capacity without a list
               ("sim_gaps", (C.byref(out), None, 0, ptr, 0)),
               ("sim_gaps", (C.byref(out), None, 0, None, 8)),
               ("sim_holders", (ip, 0, op, None, 0, None)),            # no ids
               ("sim_holders", (ip, KB_HOLDERS_MAX + 1, op, None, 0, None)),
               ("sim_holders", (ip, 1, op, ptr, 0, None)),
               ("sim_holders", (ip, 1, op, None, 8, None))]
        for name, args in bad:
            with pytest.raises(KbError) as e:
                g.lib.call(name, g.h, *args)
            assert e.value.code == KB_INVALID_ARGUMENT, (name, args)
        ids[1] = cap                                                   # an id that is not below the capacity
        with pytest.raises(KbError) as e:
            g.lib.call("sim_holders", g.h, ip, 2, op, None, 0, None)
        assert e.value.code == KB_INVALID_ARGUMENT
        assert g.gaps_device_ms() == 0.0 and g.holders_device_ms() == 0.0          # nothing has answered yet
        g.gaps()
        g.holders([0])
        assert 0.0 < g.gaps_device_ms() < 1000.0 and 0.0 < g.holders_device_ms() < 1000.0
    # handles that cannot answer say so: sparse rows (alone, as shards, as a rank), and a dense rank handle
    for kind in ("sparse", "sparse_x2", "rank", "sparse_rank"):
        kc = parity.with_cfg(sc, variant=KB_VARIANT_SPARSE_ROWS if kind.startswith("sparse") else 0, track_latency=0)
        kw = dict(rank=0, world=1, uid=rccl_unique_id(gpu)) if kind.endswith("rank") else dict(shards=2 if kind == "sparse_x2" else 0)
        with Sim(gpu, kc["cfg"], **kw) as g:
            g.step(2)
            for call in (g.gaps, lambda: g.holders([0])):
                with pytest.raises(KbError) as e:
                    call()
                assert e.value.code == KB_INVALID_OPERATION
                assert ("sparse" if kind.startswith("sparse") else "rank") in str(e.value), kind
            assert g.gaps_device_ms() == 0.0 and g.holders_device_ms() == 0.0
