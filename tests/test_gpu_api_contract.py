"""The C ABI's refusals, size queries and drains, pinned on every handle kind.

One script of raw calls (return codes through parity's SimLib, no exceptions) runs on the CPU oracle and on the four
kinds of HIP handle: dense, dense x3 (kb_sim_create_local), sparse rows, sparse rows x2.  Every call's return code
and outputs must equal the oracle's, call by call.  The round-by-round parity tests compare the happy paths; this
file covers what they hardly reach: node range and null pointers, lifecycle refusals, identity rules, the
ping_addrs queue, external-peer limits, and size query / too-small buffer / full drain of every list call.

Capacity 64, 40 initial members, 3 rounds between phases.  Where a kind disagrees with the oracle the value is
recorded in KNOWN with a one-line comment, as found; nothing here is a fix.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import replace

import pytest

import parity
from kaboodle_amd._ffi import (KB_INIT_CONVERGED, KB_VARIANT_SPARSE_ROWS, KbBroadcast, KbError, KbPeerState,
                               KbProbeResponse, KbStats, KbUnicast, Sim, SimConfig, rccl_unique_id, wire_addr)

CAP, N0, GAP = 64, 40, 3
PAQ, TICK_MAX, MAXID = 8, 33, 32            # kb_device.h
K_PING, K_PINGREQ, K_ACK, K_KP, K_KPR, K_JOIN = 0, 1, 2, 3, 4, 16
CFG = SimConfig(capacity=CAP, initial_nodes=N0, init_mode=KB_INIT_CONVERGED, loss=0.02, seed=5, id_len=4)
KINDS = {"dense": (0, 0), "dense_x3": (0, 3), "sparse": (KB_VARIANT_SPARSE_ROWS, 0),
         "sparse_x2": (KB_VARIANT_SPARSE_ROWS, 2)}

# label -> {kind: (rc, outputs)}: where the parent's kinds disagree with the oracle, as found
KNOWN: dict[str, dict[str, tuple]] = {
    # the HIP library checks the peers' range before "not started"; the oracle the other way round
    "ping:stopped_and_range": {k: (5, None) for k in KINDS},
}

U32 = C.c_uint32


def u32s(v):
    return (U32 * max(len(v), 1))(*v)


class Script:
    """The calls of one implementation, logged as (label, rc, outputs)."""

    def __init__(self, sim: Sim):
        self.sim, self.fn, self.h, self.log = sim, sim.lib.fn, sim.h, []

    def call(self, label, name, *args, out=None):
        rc = self.fn["sim_" + name](self.h, *args)
        self.log.append((label, rc, out() if out is not None and rc == 0 else None))
        return rc

    def step(self, n=GAP):
        self.call(f"step@{len(self.log)}", "step", n)

    # size query, one too small, full read, read again: fn(buf, cap) makes the call's arguments; n the count var(s)
    def drain(self, label, name, mk, elem, count, decode, unit=1):
        self.call(f"{label}:size", name, *mk(None, 0), out=lambda: count.value)
        n = count.value
        if n:
            small = (elem * (n * unit))()
            self.call(f"{label}:small", name, *mk(small, n * unit - 1), out=lambda: count.value)
        buf = (elem * max(n * unit, 1))()
        self.call(f"{label}:full", name, *mk(buf, n * unit), out=lambda: decode(buf, count.value))
        return n


def run_script(sim: Sim) -> list:
    s = Script(sim)
    n, n2, fp, flag, v32 = C.c_size_t(), C.c_size_t(), U32(), C.c_int(), U32()
    ibuf = (C.c_int32 * (6 * 64))()
    ubuf = (U32 * CAP)()
    idb = (C.c_uint8 * MAXID)()
    row = (C.c_uint8 * CAP)()

    def identity(label, node):
        s.call(label, "identity", node, idb, MAXID, C.byref(n), out=lambda: bytes(idb[: n.value]))

    def running(label, node):
        s.call(label, "is_running", node, C.byref(flag), out=lambda: flag.value)

    def restart(label, node):
        return s.call(label, "restart_node", node, C.byref(v32), out=lambda: v32.value)

    def inject(label, sender, dest, kind, a=0, ids=()):
        m = KbUnicast(sender=sender, dest=dest, kind=kind, a=a, pay_len=len(ids))
        return s.call(label, "inject", C.byref(m), u32s(ids))

    def peers(label, node):
        return s.drain(label, "peers", lambda b, c: (node, b, c, C.byref(n)), U32, n, lambda b, k: list(b[:k]))

    def peer_states(label, node):
        dec = lambda b, k: [(a.peer, a.state, a.since, a.latency_ms, bytes(a.identity[: a.identity_len])) for a in b[:k]]
        return s.drain(label, "peer_states", lambda b, c: (node, b, c, C.byref(n)), KbPeerState, n, dec)

    def suspects(label, node):
        return s.drain(label, "dump_suspects", lambda b, c: (node, b, c, C.byref(n)), C.c_int32, n,
                       lambda b, k: list(b[: 3 * k]), unit=3)

    def curious(label, node):
        return s.drain(label, "dump_curious", lambda b, c: (node, b, c, C.byref(n)), C.c_int32, n,
                       lambda b, k: list(b[: 6 * k]), unit=6)

    def broadcasts(label):
        return s.drain(label, "broadcasts", lambda b, c: (b, c, C.byref(n)), KbBroadcast, n,
                       lambda b, k: [(a.kind, a.sender, a.peer) for a in b[:k]])

    def probe_responses(label):
        dec = lambda b, k: [(a.round, a.responder, a.probe, bytes(a.prober.ip), a.prober.port,
                             bytes(a.identity[: a.identity_len])) for a in b[:k]]
        return s.drain(label, "probe_responses", lambda b, c: (b, c, C.byref(n)), KbProbeResponse, n, dec)

    def events(label, node):
        nd, npp = C.c_size_t(), C.c_size_t()
        head = lambda d, cd, p, cp: (node, d, cd, C.byref(nd), p, cp, C.byref(npp), C.byref(fp), C.byref(flag))
        s.call(f"{label}:size", "events", *head(None, 0, None, 0), out=lambda: (nd.value, npp.value, fp.value, flag.value))
        a, b = nd.value, npp.value
        d, p = (U32 * max(a, 1))(), (U32 * max(b, 1))()
        if a:
            s.call(f"{label}:small", "events", *head(d, a - 1, p, b))
        s.call(f"{label}:full", "events", *head(d, a, p, b),
               out=lambda: (list(d[: nd.value]), list(p[: npp.value]), fp.value, flag.value))
        return a + b

    def exported(label):
        ni = C.c_size_t()
        dec = lambda us, ids: [(u.round, u.wave, u.sender, u.dest, u.seq, u.kind, u.a, u.fp, u.n,
                                list(ids[u.pay_off:u.pay_off + u.pay_len])) for u in us]
        s.call(f"{label}:size", "exported", None, 0, C.byref(n), None, 0, C.byref(ni), out=lambda: (n.value, ni.value))
        a, b = n.value, ni.value
        us, ids = (KbUnicast * max(a, 1))(), (U32 * max(b, 1))()
        if a:
            s.call(f"{label}:small", "exported", us, a - 1, C.byref(n), ids, b, C.byref(ni))
        if b:
            s.call(f"{label}:small_ids", "exported", us, a, C.byref(n), ids, b - 1, C.byref(ni))
        s.call(f"{label}:full", "exported", us, a, C.byref(n), ids, b, C.byref(ni), out=lambda: dec(us[: n.value], ids))
        return a

    # ---- node range: node >= capacity on every entry point that takes a node ---------------------------------
    m0 = KbUnicast(sender=0, dest=1, kind=K_PING)
    one = u32s([1])
    range_calls = {
        "start_node": (), "stop_node": (), "restart_node": (C.byref(v32),), "is_running": (C.byref(flag),),
        "ping_addrs": (one, 1), "set_identity": (b"abcd", 4), "identity": (idb, MAXID, C.byref(n)),
        "fingerprint": (C.byref(fp),), "peers": (ubuf, CAP, C.byref(n)), "peer_states": (None, 0, C.byref(n)),
        "dump_row": (row, CAP), "dump_suspects": (ibuf, 384, C.byref(n)), "dump_curious": (ibuf, 384, C.byref(n)),
        "watch": (), "events": (None, 0, C.byref(n), None, 0, C.byref(n2), C.byref(fp), C.byref(flag)),
        "set_external": (),
    }
    for name, rest in range_calls.items():
        for node in (CAP, 0xFFFFFFFF):
            s.call(f"range:{name}:{node}", name, node, *rest)
    # ---- null pointers ------------------------------------------------------------------------------------------
    null_calls = {
        "restart_node": (3, None), "is_running": (3, None), "ping_addrs": (3, None, 1), "set_identity": (45, None, 4),
        "identity": (3, idb, MAXID, None), "fingerprint": (3, None), "fingerprints": (None, CAP),
        "true_fingerprint": (None,), "peers": (3, ubuf, CAP, None), "peer_states": (3, None, 0, None),
        "stats": (None,), "dump_row": (3, None, CAP), "dump_scalars": (None, 4 * CAP),
        "dump_suspects": (3, ibuf, 384, None), "dump_curious": (3, ibuf, 384, None),
        "events": (3, None, 0, None, None, 0, C.byref(n2), C.byref(fp), C.byref(flag)), "probe": (None,),
        "probe_responses": (None, 0, None), "broadcasts": (None, 0, None), "inject": (None, None),
        "exported": (None, 0, None, None, 0, None),
    }
    for name, args in null_calls.items():
        s.call(f"null:{name}", name, *args)
    s.call("short:fingerprints", "fingerprints", ubuf, CAP - 1)
    s.call("short:dump_row", "dump_row", 3, row, CAP - 1)
    s.call("short:dump_scalars", "dump_scalars", ibuf, 4 * CAP - 1)
    s.call("inject:pay_null", "inject", C.byref(KbUnicast(sender=0, dest=1, kind=K_KP, pay_len=2)), None)
    # ---- observers ----------------------------------------------------------------------------------------------
    s.call("watch:3", "watch", 3)
    s.call("watch:3:again", "watch", 3)
    s.call("watch:30", "watch", 30)
    s.call("events:unwatched", "events", 5, None, 0, C.byref(n), None, 0, C.byref(n2), C.byref(fp), C.byref(flag))
    s.step()
    # ---- lifecycle ------------------------------------------------------------------------------------------------
    s.call("start:running", "start_node", 0)
    s.call("stop:5", "stop_node", 5)
    running("running:5:queued_stop", 5)                 # the device's alive, not the queue: still 1
    s.step()
    running("running:5:stopped", 5)
    s.call("start:stopped", "start_node", 5)
    # ---- identity ---------------------------------------------------------------------------------------------------
    s.call("ident:running", "set_identity", 0, b"abcd", 4)
    s.call("ident:stopped_ran", "set_identity", 5, b"pend", 4)
    identity("ident:stopped_ran:still_old", 5)
    s.call("ident:never_bound", "set_identity", N0, b"frsh", 4)
    identity("ident:never_bound:now", N0)
    s.call("ident:too_long", "set_identity", 45, b"x" * (MAXID + 1), MAXID + 1)
    s.call("ident:len_max", "set_identity", 45, b"y" * MAXID, MAXID)
    restart("restart:5", 5)                             # skips N0 (an identity was set): N0 + 1
    to = v32.value
    identity("ident:pending_moved", to)
    restart("restart:5:again", 5)
    restart("restart:never_bound", 50)
    restart("restart:running", 0)
    s.call("start:queued_restart_target", "start_node", to)
    s.call("ident:moved", "set_identity", 5, b"zzzz", 4)
    s.step()
    running("running:restarted", to)
    running("running:50", 50)
    running("running:5:moved", 5)
    # ---- ping_addrs ---------------------------------------------------------------------------------------------------
    s.call("ping:stopped", "ping_addrs", 5, one, 1)
    s.call("ping:peer_range", "ping_addrs", 0, u32s([1, CAP]), 2)
    s.call("ping:stopped_and_range", "ping_addrs", 5, u32s([CAP]), 1)
    s.call("ping:known", "ping_addrs", 0, u32s([1, 2, 3]), 3)
    s.call("ping:empty", "ping_addrs", 0, None, 0)
    s.call("ping:fill", "ping_addrs", 0, u32s([55] * PAQ), PAQ)
    s.call("ping:full", "ping_addrs", 0, u32s([56]), 1)
    s.call("ping:full:known", "ping_addrs", 0, u32s([1]), 1)
    s.call("ping:30", "ping_addrs", 30, u32s([1, 55, 2, 57]), 4)
    s.step()
    # ---- external peers ---------------------------------------------------------------------------------------------
    s.call("ext:bound", "set_external", 0)
    s.call("ext:60", "set_external", 60)
    s.call("ext:60:again", "set_external", 60)
    s.call("ext:61", "set_external", 61)
    s.call("ident:external", "set_identity", 61, b"extn", 4)
    inject("inject:not_external", 7, 1, K_PING)
    inject("inject:join", 60, 0, K_JOIN)
    inject("inject:join:second", 60, 0, K_JOIN)
    inject("inject:join:61", 61, 0, K_JOIN)
    inject("inject:bad_kind", 60, 1, 7)
    inject("inject:dest_range", 60, CAP, K_PING)
    inject("inject:ack_a_range", 60, 1, K_ACK, a=CAP)
    inject("inject:pay_range", 61, 2, K_KP, ids=[1, CAP])
    for k in range(TICK_MAX):
        inject(f"inject:ping:{k}", 60, k % 8, K_PING)
    inject("inject:ping:over", 60, 1, K_PING)
    inject("inject:kp", 61, 2, K_KP, ids=[9, 1, 60])
    inject("inject:kpr", 61, 3, K_KPR)
    inject("inject:pingreq", 61, 30, K_PINGREQ, a=4)
    for k in range(24):
        s.call(f"probe:{k}", "probe", C.byref(wire_addr(("192.0.2.10", 41000 + k))))
    s.step(1)
    exported("exported:r1")
    probe_responses("probes:r1")
    s.step(GAP - 1)
    # ---- lists: size query, a buffer one too small, the full drain, the drain again -------------------------------
    s.call("stop:6", "stop_node", 6)
    s.step(2)
    restart("restart:51:first_start", 51)               # its first tick broadcasts Join in the last round
    restart("restart:6", 6)
    s.step(1)
    broadcasts("broadcasts")
    exported("exported")
    exported("exported:again")
    probe_responses("probes:again")
    for node in (3, 30):
        peers(f"peers:{node}", node)
        peer_states(f"peer_states:{node}", node)
        events(f"events:{node}", node)
        events(f"events:{node}:again", node)
    peers("peers:stopped", 5)
    peer_states("peer_states:never_bound", 58)
    # ---- restarts until no fresh address is left --------------------------------------------------------------------
    for node in range(8, 32):
        s.call(f"stop:{node}", "stop_node", node)
    s.step()
    for node in range(8, 32):
        restart(f"exhaust:{node}", node)
    s.step()
    # ---- the state after the script ---------------------------------------------------------------------------------
    st = KbStats()
    s.call("final:stats", "stats", C.byref(st), out=st.as_dict)
    sc = (C.c_int32 * (4 * CAP))()
    s.call("final:scalars", "dump_scalars", sc, 4 * CAP, out=lambda: list(sc))
    s.call("final:fingerprints", "fingerprints", ubuf, CAP, out=lambda: list(ubuf))
    s.call("final:true_fingerprint", "true_fingerprint", C.byref(fp), out=lambda: fp.value)
    for node in range(CAP):
        s.call(f"final:row:{node}", "dump_row", node, row, CAP, out=lambda: bytes(row))
        s.call(f"final:fingerprint:{node}", "fingerprint", node, C.byref(fp), out=lambda: fp.value)
        suspects(f"final:suspects:{node}", node)
        curious(f"final:curious:{node}", node)
        running(f"final:running:{node}", node)
        identity(f"final:identity:{node}", node)
    broadcasts("final:broadcasts")
    exported("final:exported")
    events("final:events:3", 3)
    return s.log


def check_coverage(log: list) -> None:
    """The script reaches what it is meant to pin (decided on the oracle's log)."""
    got = {label: (rc, out) for label, rc, out in log}
    for label in ("exported:r1:small", "exported:r1:small_ids", "probes:r1:small", "broadcasts:small", "peers:3:small",
                  "peer_states:30:small", "events:3:small"):
        assert label in got, f"the script never reads {label.rsplit(':', 1)[0]} with a buffer one too small"
    assert any(rc == 6 for label, rc, _ in log if label.startswith("exhaust:")), "fresh addresses never ran out"


_ORACLE_LOG: list = []


def oracle_log() -> list:
    if not _ORACLE_LOG:
        with Sim(parity.oracle_lib(), CFG) as o:
            _ORACLE_LOG.extend(run_script(o))
        check_coverage(_ORACLE_LOG)
    return _ORACLE_LOG


def compare(kind: str, log: list, ref: list) -> list[str]:
    bad = []
    assert [e[0] for e in log] == [e[0] for e in ref], "the scripts diverged: different calls were made"
    for (label, rc, out), (_, orc, oout) in zip(log, ref):
        want = KNOWN.get(label, {}).get(kind, (orc, oout))
        if (rc, out) != want:
            bad.append(f"{label}: got rc {rc} {out!r:.200}, want rc {want[0]} {want[1]!r:.200}")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_api_contract(kind):
    variant, shards = KINDS[kind]
    ref = oracle_log()
    with Sim(parity.gpu_lib(), replace(CFG, variant=variant), shards=shards) as g:
        log = run_script(g)
    bad = compare(kind, log, ref)
    for line in bad:
        print(line)
    assert not bad, f"{len(bad)} of {len(log)} calls differ from the oracle, first: {bad[0]}"


# ---- the five censuses against the handle kinds -------------------------------------------------------------------
# What each census entry point does on each kind of handle: None = it answers, else (code, kb_last_error()), exact.
# Capacity 96, 64 initial members, 2 rounds.  Dense handles track latency ("dense_nolat" is the one that does not).
# "rank" is one rank of a one-rank kb_sim_create_rank world; "sparse_rank" the same over sparse rows (which refusal
# comes first is part of the contract).
CENSUSES = ("census", "reciprocity", "fp_classes", "latency_census", "age_census")
_OWN_ROWS = " (use kb_sim_create or kb_sim_create_local)"
_RC_SPARSE = (1, "kb_sim_reciprocity: sparse rows need an O(entries) algorithm of their own (not built yet)")
_RC_RANK = (1, "kb_sim_reciprocity: a rank handle holds its own rows only; the census needs every rank's" + _OWN_ROWS)
_FC_RANK = (1, "kb_sim_fp_classes: a rank handle holds its own rows only and a class spans ranks" + _OWN_ROWS)
_LC_SPARSE = (1, "kb_sim_latency_census: sparse rows keep no latency table")
_LC_RANK = (1, "kb_sim_latency_census: a rank handle holds its own rows only" + _OWN_ROWS)
_LC_NOLAT = (1, "kb_sim_latency_census: the handle was created without track_latency")
_AG_DENSE = (1, "kb_sim_age_census: dense rows are not answered yet (KB_VARIANT_SPARSE_ROWS handles are)")
_AG_RANK = (1, "kb_sim_age_census: a rank handle holds its own rows only" + _OWN_ROWS)
# kind -> (variant, shards, rank handle, track_latency), then the row of expectations in the order of CENSUSES
CENSUS_MATRIX = {
    "dense": ((0, 0, False, 1), (None, None, None, None, _AG_DENSE)),
    "dense_nolat": ((0, 0, False, 0), (None, None, None, _LC_NOLAT, _AG_DENSE)),
    "sparse": ((KB_VARIANT_SPARSE_ROWS, 0, False, 0), (None, _RC_SPARSE, None, _LC_SPARSE, None)),
    "dense_x2": ((0, 2, False, 1), (None, None, None, None, _AG_DENSE)),
    "sparse_x2": ((KB_VARIANT_SPARSE_ROWS, 2, False, 0), (None, _RC_SPARSE, None, _LC_SPARSE, None)),
    "rank": ((0, 0, True, 1), (None, _RC_RANK, _FC_RANK, _LC_RANK, _AG_RANK)),     # the view census: its own rows
    "sparse_rank": ((KB_VARIANT_SPARSE_ROWS, 0, True, 0), (None, _RC_SPARSE, _FC_RANK, _LC_SPARSE, _AG_RANK)),
}
CENSUS_CFG = SimConfig(capacity=96, initial_nodes=64, init_mode=KB_INIT_CONVERGED, loss=0.02, seed=5)


@pytest.mark.gpu
def test_census_refusal_matrix():
    """Every census on every kind of handle answers or refuses with exactly the pinned code and text, and the
    *_device_ms getters read 0.0 until their census has answered on that handle, > 0 afterwards, and on a group the
    last call's time alone (a second call on the unchanged mesh is not the sum of both)."""
    lib = parity.gpu_lib()
    bad = []
    for kind, ((variant, shards, rank, track), row) in CENSUS_MATRIX.items():
        cfg = replace(CENSUS_CFG, variant=variant, track_latency=track)
        kw = dict(rank=0, world=1, uid=rccl_unique_id(lib)) if rank else dict(shards=shards)
        with Sim(lib, cfg, **kw) as g:
            ms = {name: getattr(g, name + "_device_ms") for name in CENSUSES}
            for name in CENSUSES:
                assert ms[name]() == 0.0, f"{kind}: {name}_device_ms() on a fresh handle"
            g.step(2)
            for name, want in zip(CENSUSES, row):
                try:
                    getattr(g, name)()
                    got = None
                except KbError as e:
                    got = (e.code, lib.fn["last_error"]().decode())
                if got != want:
                    bad.append(f"{kind}.{name}: got {got!r}, want {want!r}")
                    continue
                if want is not None:
                    assert ms[name]() == 0.0, f"{kind}: {name}_device_ms() after a refusal"
                    continue
                first = ms[name]()
                assert first > 0.0, f"{kind}: {name}_device_ms() after an answer"
                if shards:
                    getattr(g, name)()
                    second = ms[name]()
                    print(f"{kind}.{name}: device ms {first:.4f} then {second:.4f}")
                    assert 0.0 < second < 2.0 * first, f"{kind}: {name}_device_ms() {first} then {second}: it accumulates"
    for line in bad:
        print(line)
    assert not bad, f"{len(bad)} cells differ, first: {bad[0]}"
