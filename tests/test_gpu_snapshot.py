"""Snapshot and restore of a sparse-row mesh on the GPU (kb_sim_snapshot / kb_sim_restore,
include/kaboodle_snapshot.h; kernels in kaboodle_amd/csrc/kb_snapshot.h): a restored handle equals its source and
continues in parity with the sparse CPU oracle, whatever shard layout wrote and reads the bytes; the bytes are
canonical; only the entries in use travel; the handles and states that refuse."""
from __future__ import annotations

import ctypes as C
import os

import pytest

import parity
from kaboodle_amd import snapshot
from kaboodle_amd._ffi import (KB_CAPACITY, KB_INIT_CONVERGED, KB_INVALID_ARGUMENT, KB_INVALID_OPERATION,
                               KB_VARIANT_SPARSE_ROWS, KbError, Sim, SimConfig, rccl_unique_id)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snapshot_v1_fresh_ids.bin")
STD = {n: (c, r) for n, c, r in parity.standard_cases()}


def sparse(name: str, **kw) -> tuple[dict, int]:
    case, rounds = STD[name]
    return parity.with_cfg(case, variant=KB_VARIANT_SPARSE_ROWS, track_latency=0, **kw), rounds


# case -> the last round simulated before the snapshot
SPLITS = {"join_loss_300_ids": 2, "stop_start": 9, "identity_change": 3, "fresh_ids": 6, "partition_heal": 11,
          "churn_loss_512": 20, "probes": 3, "old_stamps": 70, "config2_join_1k": 1, "converged_loss_256": 0}


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    lib = parity.gpu_lib()
    assert "sim_snapshot" in lib.fn and "sim_restore" in lib.fn
    return lib


def run_to(sims, case: dict, first: int, last: int) -> None:
    """Rounds first..last (inclusive) with the case's events on every handle."""
    for r in range(first, last + 1):
        parity.apply_events(sims, case, r)
        for s in sims:
            s.step(1)


def start(lib, case: dict, split: int, shards: int = 0):
    """The oracle and a GPU handle of the case after round `split`, equal (which also drains both)."""
    o, a = Sim(parity.oracle_lib(), case["cfg"]), Sim(lib, case["cfg"], shards=shards)
    parity.setup(o, case)
    parity.setup(a, case)
    run_to((o, a), case, 0, split)
    assert parity.diff_states(parity.state_of(o), parity.state_of(a)) == []
    return o, a


def same_handles(a: Sim, b: Sim) -> None:
    assert parity.diff_states(parity.state_of(a), parity.state_of(b)) == []
    for i in range(a.capacity):
        assert a.peer_states(i) == b.peer_states(i), f"peer_states[{i}]"


def follow(o: Sim, others, case: dict, first: int, rounds: int) -> None:
    """The oracle and the handles run on to the case's last round; the restored ones (all but the last, the source)
    are compared with the oracle every round, the source at the end."""
    *restored, src = others
    for r in range(first, rounds):
        run_to((o, *others), case, r, r)
        so = parity.state_of(o)
        for b in restored:
            assert parity.diff_states(so, parity.state_of(b)) == [], f"round {r}"
            assert parity.diff_peer_states(o, b, range(o.capacity)) == [], f"round {r}"
        src.probe_responses()                         # drained like the others, whose state_of drains them
    assert parity.diff_states(parity.state_of(o), parity.state_of(src)) == []


@pytest.mark.parametrize("name", list(SPLITS))
def test_continuation_parity(gpu, name):
    case, rounds = sparse(name)
    split = SPLITS[name]
    o, a = start(gpu, case, split)
    blob = a.snapshot()
    assert 0.0 < a.snapshot_device_ms() < 1000.0
    b = Sim.restore(gpu, blob)
    assert b.stats()["round"] == split + 1
    same_handles(a, b)
    follow(o, (b, a), case, split + 1, rounds)
    for s in (o, a, b):
        s.close()


@pytest.mark.parametrize("name", ["churn_loss_512", "stop_start"])
def test_shard_agnostic(gpu, name):
    """An unsharded handle and a 3-shard group write the same bytes; each one's snapshot continues in the other's
    layout (stop_start's later restarts move rows between the shards of the restored group)."""
    case, rounds = sparse(name)
    split = SPLITS[name]
    o, a1 = start(gpu, case, split)
    a3 = Sim(gpu, case["cfg"], shards=3)
    parity.setup(a3, case)
    run_to((a3,), case, 0, split)
    blob1, blob3 = a1.snapshot(), a3.snapshot()
    assert blob1 == blob3
    b3, b1 = Sim.restore(gpu, blob1, shards=3), Sim.restore(gpu, blob3, shards=1)
    assert b3.shard_info()[1] == 3 and b1.shard_info()[1] == 1
    same_handles(a1, b3)
    same_handles(a1, b1)
    assert b3.snapshot() == blob1
    follow(o, (b3, b1, a1), case, split + 1, rounds)
    for s in (o, a1, a3, b1, b3):
        s.close()


def test_canonical(gpu):
    case, rounds = sparse("stop_start")
    o, a = start(gpu, case, SPLITS["stop_start"])
    blob = a.snapshot()
    assert a.snapshot() == blob                       # twice: the same bytes
    a.fingerprints()                                  # (a read that fills the fingerprint cache changes no byte)
    assert a.snapshot() == blob
    b = Sim.restore(gpu, blob)
    assert b.snapshot() == blob                       # a fixed point
    info = snapshot.info(blob, gpu)
    assert info["bytes"] == len(blob) and info["round"] == SPLITS["stop_start"] + 1
    assert info["alive"] == a.stats()["alive"] and info["cfg"]["device"] == -1
    for s in (o, a, b):
        s.close()


def test_snapshot_every_round_changes_nothing(gpu):
    case, rounds = sparse("socket_faithful")
    a, b = Sim(gpu, case["cfg"]), Sim(gpu, case["cfg"])
    for r in range(rounds):
        run_to((a, b), case, r, r)
        assert len(a.snapshot()) > 0
        assert parity.diff_states(parity.state_of(a), parity.state_of(b)) == [], f"round {r}"
    a.close()
    b.close()


def test_no_padding_travels(gpu):
    case, _ = sparse("converged_loss_256")
    small, _ = sparse("converged_loss_256", sparse_row_cap=160)
    lens = []
    for c in (case, small):
        with Sim(gpu, c["cfg"]) as g:
            g.step(1)
            blob = g.snapshot()
            info = snapshot.info(blob, gpu)
            assert info["entries"] * 4 == g.sparse_footprint()["bytes"]
            assert info["cfg"]["sparse_row_cap"] == c["cfg"].sparse_row_cap
            lens.append(len(blob))
    assert lens[0] == lens[1]


def test_golden_restores(gpu):
    case, rounds = sparse("fresh_ids")
    split = SPLITS["fresh_ids"]
    with open(GOLDEN, "rb") as f:
        blob = f.read()
    o = Sim(parity.oracle_lib(), case["cfg"])
    parity.setup(o, case)
    run_to((o,), case, 0, split)
    b = Sim.restore(gpu, blob)
    assert parity.diff_states(parity.state_of(o), parity.state_of(b)) == []
    assert parity.diff_peer_states(o, b, range(o.capacity)) == []
    for r in range(split + 1, rounds):
        run_to((o, b), case, r, r)
        assert parity.diff_states(parity.state_of(o), parity.state_of(b)) == [], f"round {r}"
    o.close()
    b.close()


def test_externals(gpu):
    cfg = SimConfig(capacity=132, initial_nodes=128, init_mode=KB_INIT_CONVERGED, loss=0.02, seed=19,
                    variant=KB_VARIANT_SPARSE_ROWS)
    ext = 130
    with Sim(gpu, cfg) as a:
        a.set_external(ext)
        a.inject(ext, 0, parity.K_JOIN)
        got = 0
        for r in range(3):
            for k in range(4):                        # the external instance pings members, which answer it
                a.inject(ext, 8 * r + k, parity.K_PING)
            a.step(1)
            got += len(a.exported())
        assert got > 0                                # Acks to the external address are exported
        b = Sim.restore(gpu, a.snapshot())
        more = 0
        for r in range(3):
            for s in (a, b):
                for k in range(4):
                    s.inject(ext, 64 + 8 * r + k, parity.K_PING)
                s.step(1)
            ea, eb = a.exported(), b.exported()
            assert ea == eb, f"round {r}"
            more += len(ea)
            assert parity.diff_states(parity.state_of(a), parity.state_of(b)) == []
        assert more > 0
        b.close()


def test_contracts(gpu):
    dense = STD["stop_start"][0]["cfg"]
    sp = sparse("stop_start")[0]["cfg"]
    with Sim(gpu, dense) as g:
        g.step(1)
        with pytest.raises(KbError) as e:
            g.snapshot()
        assert e.value.code == KB_INVALID_OPERATION and "dense" in str(e.value)
    with Sim(gpu, sp, rank=0, world=1, uid=rccl_unique_id(gpu)) as g:
        g.step(1)
        with pytest.raises(KbError) as e:
            g.snapshot()
        assert e.value.code == KB_INVALID_OPERATION and "rank" in str(e.value)
    with Sim(gpu, sp) as g:
        g.step(2)
        g.stop_node(3)
        with pytest.raises(KbError) as e:
            g.snapshot()
        assert e.value.code == KB_INVALID_OPERATION and "queued" in str(e.value)
        g.step(1)
        blob = g.snapshot()
        n = C.c_uint64(0)
        buf = C.create_string_buffer(len(blob))
        with pytest.raises(KbError) as e:
            g.lib.call("sim_snapshot", g.h, buf, len(blob) - 1, C.byref(n))
        assert e.value.code == KB_CAPACITY and n.value == len(blob)
        b = Sim.restore(gpu, blob)
        with pytest.raises(KbError) as e:             # observers do not travel
            b.events(0)
        assert e.value.code == KB_INVALID_OPERATION
        b.watch(0)
        b.events(0)
        b.close()
    tiny = SimConfig(capacity=4, initial_nodes=4, variant=KB_VARIANT_SPARSE_ROWS)
    with Sim(gpu, tiny) as g:
        g.step(1)
        blob = g.snapshot()
        with pytest.raises(KbError) as e:
            Sim.restore(gpu, blob, shards=8)
        assert e.value.code == KB_INVALID_ARGUMENT and "shard" in str(e.value)
        Sim.restore(gpu, blob, shards=4).close()      # a row each
