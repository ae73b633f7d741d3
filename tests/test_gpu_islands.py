"""The island census on the GPU (kb_sim_islands, include/kaboodle_islands.h; kernels in
kaboodle_amd/csrc/kb_islands.h): crafted graphs through kb_islands_of against islands_ref, meshes against the CPU
oracle through the same call every round (unsharded and as 3 shards; 8 shards against the unsharded handle), read-only,
and the refusals."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import (KB_CENSUS_NONE, KB_INIT_CONVERGED, KB_INVALID_ARGUMENT, KB_INVALID_OPERATION,
                               KB_VARIANT_EXACT_LRU, KB_VARIANT_SPARSE_ROWS, KbError, KbIslands, Sim, SimConfig,
                               islands_of, rccl_unique_id)
from kaboodle_amd.islands import islands_ref

pytestmark = pytest.mark.gpu

NONE = KB_CENSUS_NONE
STD = {n: (c, r) for n, c, r in parity.standard_cases()}
# a partition long enough for each side to drop the other wholesale (sim_sender honours Failed): from round 26 on the
# oracle shows two islands of 16, and they stay two after the partition ends (tests/test_islands.py asserts it)
SPLIT = ({"cfg": SimConfig(capacity=32, initial_nodes=32, init_mode=KB_INIT_CONVERGED, loss=0.02, partition_groups=2,
                           partition_start=2, partition_end=40, seed=4)}, 48)
CASES = {"partition_heal": STD["partition_heal"], "churn_loss_512": STD["churn_loss_512"], "stop_start": STD["stop_start"],
         "config1_2x2": STD["config1_2x2"], "split32": SPLIT}


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


def has_kernel(lib) -> None:
    # the numpy fallback cannot stand in for the kernels
    assert "sim_islands" in lib.fn and "islands_of" in lib.fn and "sim_islands_device_ms" in lib.fn


def test_exports(gpu):
    has_kernel(gpu)


# ---- crafted graphs through kb_islands_of ------------------------------------------------------------------------
def pack(m: np.ndarray, cap: int) -> np.ndarray:
    """bool [cap][cols <= W] -> uint32 [cap][W/32], bit j & 31 of word j >> 5 is id j."""
    W = (cap + 8191) // 8192 * 8192
    full = np.zeros((m.shape[0], W), dtype=np.uint8)
    full[:, : m.shape[1]] = m
    return np.packbits(full, axis=1, bitorder="little").view("<u4")


def check(gpu, m: np.ndarray, run, packed: np.ndarray | None = None):
    """kb_islands_of == islands_ref on summary, labels and sizes; returns the GPU's result."""
    has_kernel(gpu)
    run = np.asarray(run, dtype=bool)
    want = islands_ref(m, run)
    got = islands_of(gpu, pack(m, len(run)) if packed is None else packed, run)
    d = got.same_as(want)
    assert not d, "; ".join(d[:6])
    assert got.summary["round"] == -1 and got.summary["sweeps"] >= 1
    assert islands_of(gpu, pack(m, len(run)) if packed is None else packed, run, arrays=False).summary["top"] == want.summary["top"]
    return got


def path(cap: int, ids: np.ndarray, direction: str) -> np.ndarray:
    """A path through `ids` in the given order; every id holds itself.  up: the lower id of each edge holds the higher
    (labels travel by pull only); down: the higher holds the lower (push only); alternating: edge k by its parity."""
    m = np.eye(cap, dtype=bool)
    for k, (a, b) in enumerate(zip(ids[:-1], ids[1:])):
        lo, hi = min(a, b), max(a, b)
        up = direction == "up" or (direction == "alternating" and k % 2 == 0)
        m[(lo, hi) if up else (hi, lo)] = True
    return m


@pytest.mark.parametrize("direction", ["up", "down", "alternating"])
@pytest.mark.parametrize("cap", [300, 8200], ids=["cap300", "cap8200"])
def test_path_in_a_random_order(gpu, cap, direction):
    """300 ids on one path visited in a seeded random order: one island, whatever way the edges point.  At capacity
    8,200 (W = 16,384, two 8,192-id steps a row) the ids lie on both sides of column 8,192."""
    rng = np.random.default_rng(cap)
    if cap == 300:
        ids = rng.permutation(300)
    else:
        ids = rng.choice(cap, 300, replace=False)
        ids[:4] = [8191, 8192, 8199, 5]
        ids = np.array(list(dict.fromkeys(ids.tolist())))              # still a path: no id twice
        assert (ids < 8192).sum() > 50 and (ids >= 8192).sum() >= 2
    run = np.zeros(cap, dtype=bool)
    run[ids] = True
    got = check(gpu, path(cap, ids, direction), run)
    assert got.summary["islands"] == 1 and got.summary["largest"] == len(ids) and got.summary["largest_label"] == ids.min()
    assert got.summary["sweeps"] >= 2                                 # the loop ran; the count itself is not fixed


def cliques(cap: int, groups) -> np.ndarray:
    m = np.eye(cap, dtype=bool)
    for g in groups:
        g = np.asarray(g)
        m[np.ix_(g, g)] = True
    return m


@pytest.mark.parametrize("bridge", [True, False], ids=["bridged", "apart"])
def test_cliques_of_whole_words(gpu, bridge):
    """Two cliques that fill whole 32-id words (a row's word equals the running mask: the wmin shortcut), joined by one
    one-way edge from the higher clique to the lower, or not at all."""
    cap = 300
    a, b = np.arange(0, 64), np.arange(96, 192)
    m = cliques(cap, [a, b])
    if bridge:
        m[150, 40] = True
    run = np.zeros(cap, dtype=bool)
    run[a] = run[b] = True
    got = check(gpu, m, run)
    assert got.summary["top"][:2] == ([[0, 160], [NONE, 0]] if bridge else [[96, 96], [0, 64]])
    assert got.summary["unreachable_pairs"] == (0 if bridge else 2 * 64 * 96)


def test_partial_words_and_a_dead_bridge(gpu):
    """Cliques whose words are partly filled (some ids of the word run and are no members; some do not run), and two
    cliques whose only common neighbour is an id that does not run: its row holds both and both hold it."""
    cap = 300
    a, b, c = np.arange(3, 50, 2), np.arange(40, 120, 3), np.arange(200, 299)
    a = np.setdiff1d(a, b)
    m = cliques(cap, [a, b, c])
    dead = 130
    m[a[0], dead] = m[b[0], dead] = True
    m[dead, a[0]] = m[dead, b[0]] = m[dead, dead] = True
    run = np.zeros(cap, dtype=bool)
    run[a] = run[b] = run[c] = True
    run[[7, 43, 250]] = False                                          # members that do not run
    run[[0, 65, 199]] = True                                           # observers that hold only themselves
    got = check(gpu, m, run)
    s = got.summary
    assert s["islands"] == 6 and s["singletons"] == s["rebroadcasting"] == 3
    assert got.label[a[0]] == a[0] != got.label[b[0]] == b[0] and got.label[dead] == NONE and got.size[dead] == 0


def test_stale_rows_and_padding_columns_change_nothing(gpu):
    cap = 300
    rng = np.random.default_rng(11)
    m = cliques(cap, [np.arange(0, 40), np.arange(100, 140)])
    run = np.zeros(cap, dtype=bool)
    run[0:40] = run[100:140] = True
    clean = check(gpu, m, run)
    W = 8192
    noisy = np.zeros((cap, W), dtype=bool)
    noisy[:, :cap] = m
    noisy[~run] = rng.random((int((~run).sum()), W)) < 0.5             # rows of ids that do not run: full of bits
    noisy[:, cap:] = rng.random((cap, W - cap)) < 0.5                  # padding columns >= capacity
    noisy[np.ix_(run, ~run)] |= rng.random((80, cap - 80)) < 0.3       # live rows holding ids that do not run
    got = check(gpu, noisy[:, :cap], run, packed=pack(noisy, cap))
    assert not got.same_as(clean) and got.summary["top"][:2] == [[0, 40], [100, 40]]
    assert got.summary["rebroadcasting"] == 0


def test_nobody_and_one_observer(gpu):
    cap = 70
    m = np.ones((cap, cap), dtype=bool)
    got = check(gpu, m, np.zeros(cap, dtype=bool))
    assert got.summary["observers"] == got.summary["islands"] == 0 and got.summary["largest_label"] == NONE
    assert (got.label == NONE).all() and not got.size.any()
    one = np.zeros(cap, dtype=bool)
    one[37] = True
    got = check(gpu, m, one)                                           # it holds 69 ids that do not run
    assert got.summary["top"][0] == [37, 1] and got.summary["singletons"] == 1 and got.summary["rebroadcasting"] == 0
    got = check(gpu, np.eye(cap, dtype=bool), one)
    assert got.summary["rebroadcasting"] == 1


@pytest.mark.parametrize("seed", range(5))
def test_random_graphs_near_the_threshold(gpu, seed):
    """G(n, p) at n = 600, p around ln n / n: many components of mixed sizes, edges one-way at random."""
    n = 600
    rng = np.random.default_rng(100 + seed)
    p = [0.4, 0.7, 1.0, 0.55, 0.2][seed] * np.log(n) / n / 2           # each direction drawn independently
    m = (rng.random((n, n)) < p) | np.eye(n, dtype=bool)
    run = rng.random(n) < 0.9
    got = check(gpu, m, run)
    assert got.summary["islands"] > 3 and got.summary["largest"] > 3


# ---- meshes against the oracle ----------------------------------------------------------------------------------
_ORACLE: dict = {}


def oracle_results(key: str, case: dict, rounds: int):
    """The oracle's island census after every round of the case: computed once, shared, never changed."""
    if key not in _ORACLE:
        out = []
        with Sim(parity.oracle_lib(), case["cfg"]) as o:
            assert "sim_islands" not in o.lib.fn
            parity.setup(o, case)
            for r in range(rounds):
                parity.apply_events((o,), case, r)
                o.step(1)
                out.append(o.islands())
        _ORACLE[key] = out
    return _ORACLE[key]


def run_against(gpu, key: str, case: dict, rounds: int, gcase: dict | None = None, shards: int = 0):
    has_kernel(gpu)
    want = oracle_results(key, case, rounds)
    gc = gcase or case
    with Sim(gpu, gc["cfg"], shards=shards) as g:
        parity.setup(g, gc)
        for r in range(rounds):
            parity.apply_events((g,), gc, r)
            g.step(1)
            d = g.islands().same_as(want[r])
            assert not d, f"{key} round {r}: " + "; ".join(d[:6])
    return want


@pytest.mark.parametrize("shards", [0, 3], ids=["unsharded", "shards3"])
@pytest.mark.parametrize("name", list(CASES))
def test_islands_equal_oracle_every_round(gpu, name, shards):
    case, rounds = CASES[name]
    if name == "config1_2x2" and shards:
        shards = 2                                                     # 4 ids make 2 shards of 2 rows
    want = run_against(gpu, "std:" + name, case, rounds, shards=shards)
    if name == "split32":                                              # not vacuous: two islands of 16, and they stay
        assert sum(w.summary["second"] >= 2 for w in want) > 10 and want[-1].summary["top"][:2] == [[0, 16], [16, 16]]
    if name == "churn_loss_512":                                       # joiners before their first Join is answered
        assert any(w.summary["rebroadcasting"] > 3 for w in want)


def test_islands_eight_shards_equal_the_unsharded_handle(gpu):
    """The row table at its last entry: 8 shards of 4 rows (split32, the smallest case here that 8 shards can split)
    against the unsharded handle, summary and arrays, every round."""
    has_kernel(gpu)
    case, rounds = CASES["split32"]
    assert min(c["cfg"].capacity for c, _ in CASES.values() if 7 * -(-c["cfg"].capacity // 8) < c["cfg"].capacity) == 32
    with Sim(gpu, case["cfg"]) as one, Sim(gpu, case["cfg"], shards=8) as grp:
        for g in (one, grp):
            parity.setup(g, case)
        for r in range(rounds):
            parity.apply_events((one, grp), case, r)
            one.step(1)
            grp.step(1)
            d = grp.islands().same_as(one.islands())
            assert not d, f"round {r}: " + "; ".join(d[:6])


def test_islands_exact_lru(gpu):
    case, rounds = SPLIT
    run_against(gpu, "lru:split32", parity.with_cfg(case, variant=KB_VARIANT_EXACT_LRU), rounds)


# ---- the handle's contract -----------------------------------------------------------------------------------------
def test_islands_is_read_only(gpu):
    """Two meshes side by side, one taking the island census (and the view census, whose k_id_masks it shares) every
    round: the complete state and the view census's results stay identical."""
    has_kernel(gpu)
    case, rounds = STD["churn_loss_512"]
    with Sim(gpu, case["cfg"]) as a, Sim(gpu, case["cfg"]) as b:
        for r in range(20):
            a.step(1)
            b.step(1)
            before = a.census()
            first = a.islands()
            assert not a.islands().same_as(first)                      # the same again
            assert not a.census().same_as(before) and not b.census().same_as(before)
            d = parity.diff_states(parity.state_of(a), parity.state_of(b))
            assert not d, f"round {r}: " + "; ".join(d[:6])


def test_arguments_and_refusals(gpu):
    has_kernel(gpu)
    case, rounds = STD["stop_start"]
    want = oracle_results("std:stop_start", case, rounds)
    cap = case["cfg"].capacity
    with Sim(gpu, case["cfg"]) as g:
        assert g.islands_device_ms() == 0.0
        parity.setup(g, case)
        for r in range(rounds):
            parity.apply_events((g,), case, r)
            g.step(1)
        out = KbIslands()
        buf = np.zeros(cap, dtype=np.uint32)
        ptr = buf.ctypes.data_as(C.POINTER(C.c_uint32))
        g.lib.call("sim_islands", g.h, C.byref(out), None, None, 0)                   # both arrays NULL
        assert {**out.as_dict(), "sweeps": 0} == want[-1].summary
        assert 0.0 < g.islands_device_ms() < 1000.0
        g.lib.call("sim_islands", g.h, C.byref(out), None, ptr, cap)                  # size alone
        assert np.array_equal(buf, want[-1].size)
        for args in ((ptr, None), (None, ptr)):                                       # a short array
            with pytest.raises(KbError) as e:
                g.lib.call("sim_islands", g.h, C.byref(out), *args, cap - 1)
            assert e.value.code == KB_INVALID_ARGUMENT
        with pytest.raises(KbError) as e:                                             # out == NULL
            g.lib.call("sim_islands", g.h, None, None, None, 0)
        assert e.value.code == KB_INVALID_ARGUMENT
    with pytest.raises(KbError) as e:
        gpu.call("islands_of", 0, ptr, buf.ctypes.data_as(C.POINTER(C.c_uint8)), cap, None, None, None, 0)
    assert e.value.code == KB_INVALID_ARGUMENT
    # handles that cannot answer say so: sparse rows (alone, as shards, as a rank), and a dense rank handle
    for kind in ("sparse", "sparse_x2", "rank", "sparse_rank"):
        sc = parity.with_cfg(case, variant=KB_VARIANT_SPARSE_ROWS if kind.startswith("sparse") else 0, track_latency=0)
        kw = dict(rank=0, world=1, uid=rccl_unique_id(gpu)) if kind.endswith("rank") else dict(shards=2 if kind == "sparse_x2" else 0)
        with Sim(gpu, sc["cfg"], **kw) as g:
            g.step(2)
            with pytest.raises(KbError) as e:
                g.islands()
            assert e.value.code == KB_INVALID_OPERATION
            assert ("sparse" if kind.startswith("sparse") else "rank") in str(e.value), kind
            assert g.islands_device_ms() == 0.0
