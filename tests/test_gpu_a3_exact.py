"""The exact-order A3 kernel (k_a3_exact, KB_VARIANT_EXACT_LRU) against the dense CPU oracle on an MI355X: all three
instantiations, every exit of the narrow path, and the block pruning.

The reference is the oracle's exact branch, a linear scan of the row that keeps the five smallest (instant, rotated
id) (oracle/kb_oracle.c, a3_candidates; itself pinned to tests/pyref.py by test_oracle_live_pin_exact).  Every case
goes through parity.run_case: complete state (rows, scalars, suspects, curious, fingerprints, counters), bit-exact,
after every round.  Parity alone cannot tell which path answered or how much of a row was read, so each case also
reads kb_sim_debug_counters every round and asserts on the round's deltas: rows, rows that loaded more than one
1024-id block, blocks loaded, and one slot per exit (32-bit keys / clamp redo / few-saturated redo / live-byte pass /
one-pass wide kernel).

Each case runs on the kernel its width picks (<2>), on KB_DBG_A3X_KPL8 (<8>, otherwise only the 139K-id test) and on
KB_DBG_A3X_WIDE (<0>, rows above 512K ids: otherwise never run).  Capacity 2100 gives W = 4096: four blocks, block 3
without ids, block 2 ending at id 2099 inside a lane's 16 ids.

The stamp window is 192 rounds deep (a byte encodes instant - epoch base + 192): an entry saturates at the first
rebase at which it is 190 rounds old, so no instant from round 0 on saturates before round 192.  Cases that need
saturated instants other than the converged start's therefore pass round 192."""
import ctypes as C

import pytest

import parity
from kaboodle_amd._ffi import KB_DBG_A3X_KPL8, KB_DBG_A3X_WIDE, KB_INIT_CONVERGED, KB_VARIANT_EXACT_LRU, SimConfig

pytestmark = pytest.mark.gpu

KERNELS = {"default": 0, "kpl8": KB_DBG_A3X_KPL8, "wide": KB_DBG_A3X_WIDE}
ROWS, DEEP, BLOCKS, K32, CLAMP, FEW, LIVE, WIDE = 0, 1, 2, 5, 6, 7, 8, 9


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


def run_counted(case, rounds, flags=0, shards=0):
    """parity.run_case on `case` under the exact order; returns the per-round deltas of kb_sim_debug_counters (a
    list of 10-tuples) and the running peers after each round."""
    deltas, alive, last = [], [], [0] * 10

    def on_round(r, o, g):
        buf = (C.c_uint64 * 10)()
        assert g.lib.lib.kb_sim_debug_counters(g.h, buf, 10) == 0
        now = list(buf)
        deltas.append(tuple(a - b for a, b in zip(now, last)))
        last[:] = now
        alive.append(o.stats()["alive"])

    case = parity.with_cfg(case, variant=KB_VARIANT_EXACT_LRU, debug_flags=flags)
    ok, msg, _ = parity.run_case(case, rounds, full_rows=True, shards=shards, omp=case["cfg"].capacity >= 2048,
                                 on_round=on_round)
    assert ok, f"debug_flags={flags} shards={shards}: {msg}"
    assert len(deltas) == rounds
    return deltas, alive


def check_common(deltas, alive, flags):
    """What holds in every round of every case: the kernel saw every running row, each row took exactly one exit,
    the forced kernels ran (and only they)."""
    for r, (d, n) in enumerate(zip(deltas, alive)):
        assert d[ROWS] == n, f"round {r}: {d[ROWS]} rows scanned, {n} running"
        if flags & KB_DBG_A3X_WIDE:
            assert d[WIDE] == n and d[K32] == d[CLAMP] == d[FEW] == d[LIVE] == 0, f"round {r}: {d}"
        else:
            assert d[WIDE] == 0 and d[K32] + d[CLAMP] + d[FEW] == n and d[LIVE] == d[FEW], f"round {r}: {d}"
            assert d[BLOCKS] >= d[ROWS] + d[DEEP], f"round {r}: {d}"


TIES_3BLOCKS = {"cfg": SimConfig(capacity=2100, initial_nodes=2100, init_mode=KB_INIT_CONVERGED, loss=0.01, seed=43)}


@pytest.mark.parametrize("kernel", list(KERNELS) + ["x3"])
def test_ties_3blocks(gpu, kernel):
    """A converged start of 2100 peers, 8 rounds.  Round 0: every bound is INT32_MIN, the first bound is the base,
    every offset clamps: each row is redone and loads at least its three id-holding blocks.  That pass leaves every
    bound exact and equal (INT32_MIN / 2, the start's tie), so from round 1 a row starts in the sweep front's block
    and stops once it holds five ties, which span at most that block and the next: at most 2 blocks per row, from
    the 32-bit keys.  The block bound is what fails if the bounds stop tightening (tried: without a3x_narrow's
    `lbrow[b] = smin` writes only this assertion fails)."""
    flags, shards = KERNELS.get(kernel, 0), 3 if kernel == "x3" else 0
    deltas, alive = run_counted(TIES_3BLOCKS, 8, flags, shards)
    print(f"ties_3blocks[{kernel}]:", deltas)
    check_common(deltas, alive, flags)
    if flags & KB_DBG_A3X_WIDE:
        return
    d = deltas[0]
    assert d[CLAMP] == d[ROWS] == 2100 and d[BLOCKS] >= 3 * d[ROWS], f"round 0: {d}"
    for r, d in enumerate(deltas[1:], 1):
        assert d[BLOCKS] <= 2 * d[ROWS] and d[BLOCKS] < 3 * d[ROWS], f"round {r}: {d[BLOCKS]} blocks for {d[ROWS]} rows"
        assert d[K32] >= 0.99 * d[ROWS], f"round {r}: {d}"


# 48 peers started by id on both sides of every block edge: 1023/1024, 2047/2048, and the last id, 2099
SPREAD = [0, 1, 2, 3] + list(range(1016, 1032)) + list(range(2040, 2056)) + list(range(2088, 2100))
STALE = [2, 1023, 1024, 2047, 2099]       # stopped before round 2 with maps heard in rounds 0-1, back in round 196
JOIN_SPREAD = {"cfg": SimConfig(capacity=2100, initial_nodes=0, loss=0.01, seed=47), "start": SPREAD,
               "events": {2: [("stop", i, None) for i in STALE], 196: [("restart", i, None) for i in STALE]}}
JOIN_ROUNDS = 204


@pytest.mark.parametrize("kernel", list(KERNELS) + ["x3"])
def test_join_spread(gpu, kernel):
    """A join from nothing.  No entry saturates before round 192 (the window's depth), and a running peer of a 48-peer
    mesh hears every entry again long before it is 190 rounds old: every row of every round has fewer than five
    saturated entries, is redone and takes the live-byte pass over all three blocks.  Five peers stop before round 2
    and restart in round 196 with the maps they held: entries of rounds -10..1 across three blocks, all saturated by
    the rebase at round 192, beside the live entries they then hear.  Their rows, moved with all bounds reset, are
    redone for the clamp once and then answered from the 32-bit keys (offsets from the exact first bound <= 11)."""
    flags, shards = KERNELS.get(kernel, 0), 3 if kernel == "x3" else 0
    assert {1023, 1024, 2047, 2048, 2099} <= set(SPREAD)
    deltas, alive = run_counted(JOIN_SPREAD, JOIN_ROUNDS, flags, shards)
    print(f"join_spread[{kernel}]:", deltas[:3], deltas[190:])
    check_common(deltas, alive, flags)
    if flags & KB_DBG_A3X_WIDE:
        return
    for r, d in enumerate(deltas[:196]):
        assert d[FEW] == d[LIVE] == d[ROWS] > 0, f"round {r}: {d}"
    assert sum(d[CLAMP] for d in deltas[196:]) >= 1, deltas[196:]
    assert sum(d[K32] for d in deltas[197:]) >= 1, deltas[196:]


TIES_RUN_OUT = {"cfg": SimConfig(capacity=400, initial_nodes=400, init_mode=KB_INIT_CONVERGED, seed=1)}


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_ties_run_out(gpu, kernel):
    """Exact bounds, one to four start ties left beside real saturated instants: the fifth key is a real instant,
    2^30 above the ties' base, clamps, and the row must be redone with 64-bit keys (kb_round.h, `h == 255u`).  A row
    of a loss-free converged n-peer mesh hears about two of its start ties again per round, and the first real
    instants saturate at round 192, so the ties must last past it: 400 peers is the smallest round size at which
    they do (by the oracle's rows: ties run out in rounds 196-203; at 390 peers they run out as round 192 ends, at
    300 in round 160 with nothing saturated beside them).  After the ties every row has fewer than five saturated
    entries.  One block holds ids here (W = 2048)."""
    flags = KERNELS[kernel]
    deltas, alive = run_counted(TIES_RUN_OUT, 208, flags)
    print(f"ties_run_out[{kernel}]:", [(r, d) for r, d in enumerate(deltas) if d[CLAMP]], deltas[-1])
    check_common(deltas, alive, flags)
    if flags & KB_DBG_A3X_WIDE:
        return
    clamp = [r for r, d in enumerate(deltas) if d[CLAMP] and r >= 64]
    assert clamp and min(clamp) >= 192, clamp
    assert all(d[K32] == d[ROWS] for d in deltas[1:190]), "the tied start is answered from the 32-bit keys"
    assert any(d[K32] and d[CLAMP] for d in deltas[192:]), "clamp redos beside 32-bit answers in one round"
    assert deltas[-1][FEW] == deltas[-1][LIVE] == deltas[-1][ROWS], deltas[-1]


# ties_3blocks with two free addresses: the restarts bind 2098 and 2099, rows of block 2's last, partial lane
RESTARTS = {"cfg": SimConfig(capacity=2100, initial_nodes=2098, init_mode=KB_INIT_CONVERGED, loss=0.01, seed=43),
            "events": {2: [("stop", 1500, None), ("stop", 2060, None)], 5: [("restart", 1500, None)],
                       8: [("restart", 2060, None)]}}


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_restart_multiblock(gpu, kernel):
    """A stop and a restart of an id of block 1 and of an id of block 2.  The restart moves the row to a fresh
    address and resets its bounds to INT32_MIN (k_row_unpack), so in the round of the restart that one row is redone
    for the clamp and loads its whole row again.  Its blocks are isolated from the round's sum: every row answered
    from the 32-bit keys loads one or two blocks here (checked in the rounds without a redo: blocks = rows + rows
    that loaded more than one), and a redone row always loads more than one."""
    flags = KERNELS[kernel]
    deltas, alive = run_counted(RESTARTS, 12, flags)
    print(f"restart_multiblock[{kernel}]:", deltas)
    check_common(deltas, alive, flags)
    if flags & KB_DBG_A3X_WIDE:
        return
    for r, d in enumerate(deltas[1:], 1):
        assert d[FEW] == 0 and d[CLAMP] == (1 if r in (5, 8) else 0), f"round {r}: {d}"
        redone = d[BLOCKS] - (d[ROWS] - d[CLAMP]) - (d[DEEP] - d[CLAMP])
        if d[CLAMP]:
            assert redone >= 3, f"round {r}: the moved row loaded {redone} blocks, its row has 3 with ids"
        else:
            assert redone == 0, f"round {r}: {d}"
