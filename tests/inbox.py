"""Crafted wave-0 inboxes for the receive window (csrc/kb_waves.h: k_kp, k_sortfast, k_proc; k_sp_handle on sparse
rows), injected by external peers (kb_sim_set_external / kb_sim_inject).

A crafted case is a loss-free, churn-free mesh of a few running peers, a list of external ids and a script:
script[r] = the records injected after round r (they arrive in wave 0 of round r + 1), each a tuple
(sender, dest, kind, a, fp, n, ids).  A script may be a function of the oracle's state (group F answers from
whichever external peer a node suspects): it is evaluated on the oracle alone, once, and the recorded records are
replayed verbatim to every other handle.  Everything a simulated peer answers to an external peer comes back
through kb_sim_exported in (round, wave, sender, seq) order, which exposes the order the handlers ran in.

tests/test_inbox.py checks on the oracle alone that every case is what it claims; tests/test_gpu_inbox.py runs the
cases on the HIP library.  Both import the case builders below (groups A-F)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, replace

import numpy as np

import parity
from kaboodle_amd._ffi import KB_INIT_CONVERGED, KT_PROC, Sim, SimConfig

K_PING, K_PINGREQ, K_ACK, K_KP, K_KPR, K_JOIN = parity.K_PING, parity.K_PINGREQ, parity.K_ACK, parity.K_KP, parity.K_KPR, parity.K_JOIN
PER_SENDER = 33                       # records one external peer may inject per round (kb_sim_inject)
FAST_MAX, WAVE_SORT, SORT_MAX, KP_BIG = 8, 64, 8192, 4096      # the thresholds of csrc/kb_waves.h
CSLOTS, NOBS = 8, 4                   # the curious table: targets per node, observers per target
PATH_KP_BIG_HBM, PATH_PROC_UNSORTED, PATH_KP_BIG_LDS, PATH_PROC_DEFERRED = 8, 16, 128, 512   # kb_common.h PATH_*
DROPS = ("drop_dead", "drop_loss", "drop_window", "drop_oversize", "drop_partition", "drop_bcast")
SENT = {K_PING: "sent_ping", K_PINGREQ: "sent_ping_req", K_ACK: "sent_ack", K_KP: "sent_known_peers", K_KPR: "sent_kpr"}


@dataclass
class Case:
    name: str
    cfg: SimConfig
    externals: list
    script: object                    # {r: [records]} or f(r, oracle, exported) -> [records]
    rounds: int
    events: dict = field(default_factory=dict)
    identities: dict = field(default_factory=dict)
    dests: tuple = (0,)               # the destinations the script addresses (fingerprint / peer_states checks)
    # conditions, checked on the oracle (tests/test_inbox.py): before delivery round r the view of dest contains /
    # lacks these ids; the round exports this many records; curious_overflow after the round
    contains: dict = field(default_factory=dict)      # {r: {dest: ids}}
    lacks: dict = field(default_factory=dict)         # {r: {dest: ids}}
    exports: dict = field(default_factory=dict)       # {r: count}
    overflow: dict = field(default_factory=dict)      # {r: curious_overflow after round r}
    sink: int = -1                    # an external id that takes filler records (they are exported, never handled)
    may_drop: bool = False            # the lists teach ids that never ran: the peers' own later Pings to them are dropped

    def plain(self) -> bool:
        return not self.identities and not self.cfg.id_len

    def parity_case(self) -> dict:
        return {"cfg": self.cfg, "events": self.events, "identities": self.identities}


def interleave(per_sender: dict) -> list:
    """The records of every sender in a call order that takes one record of each sender in turn, senders in
    descending id order: arrival order then differs from the canonical (sender, seq) order, seq stays per sender."""
    out, k = [], 0
    senders = sorted(per_sender, reverse=True)
    while True:
        row = [per_sender[s][k] for s in senders if k < len(per_sender[s])]
        if not row:
            return out
        out += row
        k += 1


def identity_table(sim: Sim):
    """(identities [capacity, 32], lengths) as the handle reports them; (None, None) when every identity is empty
    (id_len = 0 and none set: kb_fingerprint_of_set then takes no table)."""
    cap = sim.capacity
    idents = np.zeros((cap, 32), dtype=np.uint8)
    lens = np.zeros(cap, dtype=np.uint8)
    for j in range(cap):
        b = sim.identity(j)
        idents[j, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        lens[j] = len(b)
    return idents, lens


def check_fingerprints(sim: Sim, dests, tag: str, plain: bool) -> None:
    """Independent of the oracle: the fingerprint of every addressed running destination is generate_fingerprint
    (kb_fingerprint_of_set, a pure host function of either library) over the peers() of its row.  plain: the case
    has empty identities throughout (no table to read back)."""
    f = getattr(sim.lib.lib, sim.lib.prefix + "fingerprint_of_set")
    f.restype = C.c_uint32
    f.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    idents, lens = (None, None) if plain else identity_table(sim)
    fps = sim.fingerprints()
    running = sim.scalars()[:, 0]
    for i in dests:
        if running[i]:
            p = sim.peers(i)
            arr = (C.c_uint32 * max(1, len(p)))(*p)
            want = f(arr, len(p), None, 0, None) if plain else f(arr, len(p), idents.ctypes.data, 32, lens.ctypes.data)
            assert want == fps[i], f"{tag}: fingerprint of {i} is {int(fps[i]):#x}, its peers() give {want:#x}"


def compact(st: dict) -> dict:
    """The complete state with the all-zero rows (ids that never ran) left out of the row matrix: `rowidx` names the
    rows kept, so equal (rowidx, rows) means equal full matrices, and a trace of a capacity-8192 case stays small."""
    idx = np.flatnonzero(st["rows"].any(axis=1))
    st["rowidx"], st["rows"] = idx, np.ascontiguousarray(st["rows"][idx])
    return st


def row_of(st: dict, i: int):
    """Row i of a compacted state (all zero when it was left out)."""
    k = np.flatnonzero(st["rowidx"] == i)
    return st["rows"][int(k[0])] if len(k) else np.zeros(st["rows"].shape[1], dtype=st["rows"].dtype)


def proc_bytes(sim: Sim):
    """Algorithmic bytes k_proc has counted so far (it counts per node it handles: a round in which the figure does
    not move left every in-order inbox to k_sortfast's fast lane).  An engine that counts none raises."""
    return sim.kernel_bytes(KT_PROC)


def diff_compact(a: dict, b: dict) -> list:
    if not np.array_equal(a["rowidx"], b["rowidx"]):
        return [f"non-empty rows differ: {a['rowidx'][:8].tolist()} vs {b['rowidx'][:8].tolist()}"]
    return parity.diff_states(a, b)


def drive(sim: Sim, case: Case, injections=None):
    """The case on one handle: yields (r, view, state, exported, injected) per round; view = peers() of every dest
    before the round.  injections: the recorded records of another run, replayed; None: from the script."""
    pc = case.parity_case()
    parity.setup(sim, pc)
    for x in case.externals:
        sim.set_external(x)
    for r in range(case.rounds):
        parity.apply_events((sim,), pc, r)
        view = {i: set(sim.peers(i)) for i in case.dests}
        sim.step(1)
        ex = sim.exported()
        st = compact(parity.state_of(sim))
        if case.cfg.track_latency:
            st["peer_states"] = {i: sim.peer_states(i) for i in case.dests}
        if injections is not None:
            inj = injections[r]
        elif callable(case.script):
            inj = case.script(r, sim, ex)
        else:
            inj = case.script.get(r, [])
        for m in inj:
            sim.inject(*m[:6], ids=m[6])
        yield r, view, st, ex, inj


_TRACES: dict = {}


def oracle_trace(case: Case) -> list:
    """The oracle's run of the case, [(view, state, exported, injected)] per round: computed once per case and
    variant, shared by the tests, never modified."""
    key = (case.name, case.cfg.variant)
    if key not in _TRACES:
        with Sim(parity.oracle_lib(case.cfg.capacity > 2048), replace(case.cfg, debug_flags=0)) as o:
            tr = []
            for r, view, st, ex, inj in drive(o, case):
                check_fingerprints(o, case.dests, f"{case.name} oracle round {r}", case.plain())
                tr.append((view, st, ex, inj))
        _TRACES[key] = tr
    return _TRACES[key]


def check_conditions(case: Case) -> dict:
    """The non-vacuity conditions of a case, on the oracle alone.  The ABI has no per-kind received counter: a round
    in which none of the drop counters moves delivered every record it sent (loss = 0), the injected ones among
    them, and the sent counters rise by at least the number injected per kind."""
    tr = oracle_trace(case)
    ninj = 0
    for r in range(1, case.rounds):
        inj = [m for m in tr[r - 1][3] if m[2] != K_JOIN]
        prev, cur = tr[r - 1][1]["stats"], tr[r][1]["stats"]
        if inj:
            ninj += len(inj)
            moved = {k: cur[k] - prev[k] for k in DROPS if cur[k] != prev[k] and not (case.may_drop and k == "drop_dead")}
            assert not moved, f"{case.name} round {r}: records dropped: {moved}"
            running = tr[r][1]["scalars"][:, 0]
            assert all(running[m[1]] or m[1] == case.sink for m in inj), f"{case.name} round {r}: a record went to a stopped receiver"
            for kind, name in SENT.items():
                n = sum(1 for m in inj if m[2] == kind)
                assert cur[name] - prev[name] >= n, f"{case.name} round {r}: {name} rose by {cur[name] - prev[name]} < {n} injected"
            for m in inj:
                assert m[0] in case.externals and (m[1] in case.dests or m[1] == case.sink), f"{case.name}: record {m[:3]} outside the case"
        view = tr[r][0]
        for i, ids in case.contains.get(r, {}).items():
            assert set(ids) <= view[i], f"{case.name} round {r}: view of {i} lacks {sorted(set(ids) - view[i])[:4]}"
        for i, ids in case.lacks.get(r, {}).items():
            assert not set(ids) & view[i], f"{case.name} round {r}: view of {i} holds {sorted(set(ids) & view[i])[:4]}"
        if r in case.exports:
            assert len(tr[r][2]) == case.exports[r], f"{case.name} round {r}: {len(tr[r][2])} exported, want {case.exports[r]}"
        if r in case.overflow:
            assert cur["curious_overflow"] == case.overflow[r], f"{case.name} round {r}: overflow {cur['curious_overflow']}"
    assert ninj > 0, f"{case.name}: nothing injected"
    return {"injected": ninj}


def run_crafted(case: Case, gpu_kwargs: dict | None = None, pre_round=None, post_round=None) -> dict:
    """The case on the HIP library against the oracle's recorded run.  gpu_kwargs: shards, debug_flags, lib, proc_bytes.  After
    every round: the complete state (full rows, stats, tables, broadcasts), the exported records with their payload
    ids, peer_states of the addressed destinations (track_latency), and, independent of the oracle, the addressed
    destinations' fingerprints against kb_fingerprint_of_set of their peers().  pre_round(r, g) runs before round
    r's step, post_round(r, g) after its comparison.  Returns the paths, launches and per-round results, among them
    the bytes k_proc counted in each round (proc_bytes)."""
    kw = dict(gpu_kwargs or {})
    lib = kw.pop("lib", None) or parity.gpu_lib()
    counted = kw.pop("proc_bytes", True)      # False on sparse rows, whose kernels count no bytes
    cfg = replace(case.cfg, debug_flags=kw.pop("debug_flags", 0))
    tr = oracle_trace(case)
    out = {"states": [], "exports": [], "proc_bytes": []}
    gcase = replace(case, cfg=cfg)
    with Sim(lib, cfg, shards=kw.pop("shards", 0)) as g:
        assert not kw, f"unknown gpu_kwargs {kw}"
        g.set_profiling(2)
        g.reset_kernel_time()
        it = drive(g, gcase, injections=[t[3] for t in tr])
        for r in range(case.rounds):
            if pre_round:
                pre_round(r, g)
            b0 = proc_bytes(g) if counted else 0
            _, _, st, ex, _ = next(it)
            if counted:
                out["proc_bytes"].append(proc_bytes(g) - b0)
            ost, oex = tr[r][1], tr[r][2]
            tag = f"{case.name} round {r}"
            assert ex == oex, f"{tag}: exports differ ({len(oex)} vs {len(ex)}): " + str(
                [(a, b) for a, b in zip(oex, ex) if a != b][:2])
            d = diff_compact(ost, st)
            assert not d, f"{tag}: " + "; ".join(d[:6])
            if cfg.track_latency:
                assert st["peer_states"] == ost["peer_states"], f"{tag}: peer_states differ"
            check_fingerprints(g, case.dests, tag, case.plain())
            if post_round:
                post_round(r, g)
            out["states"].append(st)
            out["exports"].append(ex)
        out["paths"] = g.debug_paths()
        out["launches"] = {k: v["launches"] for k, v in g.kernel_breakdown().items()}
    return out


# ---- the groups ---------------------------------------------------------------------------------------------------
RUNNING = 3                            # running peers 0, 1, 2 (converged start); every script addresses peer 0


def base_cfg(capacity: int, running: int = RUNNING, **kw) -> SimConfig:
    """running = 1 where the length of peer 0's in-order inbox must be exactly the script's (groups A, C, E): with
    peers 1 and 2 running, their own A3 Pings reach peer 0 in wave 0 of some rounds and blur the edge."""
    return SimConfig(capacity=capacity, initial_nodes=running, init_mode=KB_INIT_CONVERGED, seed=5, **kw)


def ping(s, d=0):
    return (s, d, K_PING, 0, 0, 0, [])


def teach(externals, d=0) -> list:
    """One Ping of every external peer: its prologue makes the sender a member of d's view."""
    return [ping(x, d) for x in sorted(externals, reverse=True)]


A_SIZES = (1, 8, 9, 63, 64, 65, 128, 129, 255, 257, 8192, 8193)
A_MIXED = (9, 65, 129)
MIX = (K_PING, K_PINGREQ, K_ACK, K_KPR, K_PING)


def case_a(n: int, mixed: bool = False, flavor: str = "") -> Case:
    """Group A: peer 0 receives n in-order records in wave 0 of round 2 from external senders it learned in round 1.
    Plain: one Ping per record, the senders taking turns (one record each up to 300 senders, 249 x 33 cover 8193).
    mixed: four records per sender, kinds Ping / PingRequest(the first sender) / Ack / KnownPeersRequest in an order that
    depends on the sender, so seq order inside a sender shows in the answers.  flavor "nonmember": one of the
    senders was not taught; "stale": a member's KnownPeers list teaches peer 0 a new id in the same wave (k_kp
    runs ahead of the in-order handlers and leaves the fingerprint stale).  Answers: one Ack per Ping, exported in
    wave 1 in the handlers' order.  Peer 0 is the only running peer: its inbox is the script's, record for record."""
    if flavor == "unsorted":
        return case_a_unsorted(n)
    cap = 320 if n <= 257 else 512
    nx = (n + 3) // 4 if mixed else (n if n <= 300 else (n + PER_SENDER - 1) // PER_SENDER)
    ext = list(range(cap - nx - 2, cap - 2))
    per = {x: [] for x in ext}
    for k in range(n):
        x = ext[k % nx]
        kind = MIX[(len(per[x]) + x) % 5] if mixed else K_PING
        a = ext[0] if kind == K_PINGREQ else (x if kind == K_ACK else 0)
        fp, nn = (0xC0FFEE00 + x, 1000) if kind in (K_ACK, K_KPR) else (0, 0)
        per[x].append((x, 0, kind, a, fp, nn, []))
    taught = list(ext)
    recs = interleave(per)
    lacks = {}
    extra = []
    if flavor == "nonmember":
        taught = ext[1:]
        lacks = {2: {0: [ext[0]]}}
    elif flavor == "stale":
        extra = [cap - 2]                              # the member that sends the list; cap - 1 is the id it teaches
        recs = recs + [(cap - 2, 0, K_KP, 0, 0, 0, [cap - 1])]
        taught = ext + extra
        lacks = {2: {0: [cap - 1]}}
    name = f"A{n}" + ("_mixed" if mixed else "") + (f"_{flavor}" if flavor else "")
    return Case(name, base_cfg(cap, 1), ext + extra, {0: teach(taught), 1: recs}, rounds=4,
                contains={2: {0: taught}}, lacks=lacks)


A_UNSORTED = (8, 9, 64, 65, 129, 257)


def case_a_unsorted(n: int) -> Case:
    """Group A with a device inbox that arrives out of order.  k_scatter walks the outboxes of 64 consecutive senders
    per wave, 64 records per step, so the call order of kb_sim_inject never reaches the inbox: records of one wave
    arrive in (sender, seq) order.  Here the low senders (ids 66.., second wave of the first scatter workgroup) sit
    behind two fillers (ids 64, 65) whose 66 records to an external sink take the whole first step of that wave,
    while the high senders (ids 128.. and 256..: the third wave, and the second workgroup) are placed by their
    waves' first step.  The high senders' records therefore reach peer 0's inbox ahead of the low senders', and
    every sender has three records, so the sorts see an inbox that is neither sorted nor reversed.  Nothing in the
    kernel guarantees this order: it follows from how concurrent waves of one launch are scheduled, so it is likely,
    not certain, and only mutation shows it (on an MI355X, with any of the three sorts disabled these cases fail,
    while the plain cases below 64 records pass).  The cases themselves pass either way; what depends on the
    scheduler is only their power to catch a broken sort."""
    cap, sink = 320, 319
    fill = [64, 65]
    nh = n // 2
    per = {f: [ping(f, sink)] * PER_SENDER for f in fill}
    low, high = [], []
    for k in range(n - nh):
        x = 66 + k // 3
        per.setdefault(x, []).append(ping(x))
        low.append(x)
    hi_ids = [i for pair in zip(range(128, 190), range(256, 318)) for i in pair]   # the two places in turn
    for k in range(nh):
        x = hi_ids[k // 3]
        per.setdefault(x, []).append(ping(x))
        high.append(x)
    assert all(len(v) <= PER_SENDER for v in per.values()) and max(low) < 128
    ext = sorted(set(per) | {sink})
    taught = sorted(set(low) | set(high))
    return Case(f"A{n}_unsorted", base_cfg(cap, 1), ext, {0: teach(taught), 1: interleave(per)}, rounds=4,
                contains={2: {0: taught}}, sink=sink)


def acks_in_order(injected, exported, dest: int = 0) -> int:
    """The Acks `dest` exported in wave 1 answer the injected Pings in (sender, seq) order (seq = call order per
    sender); returns their number."""
    want = [s for s, _ in sorted((m[0], k) for k, m in enumerate(injected) if m[2] == K_PING and m[1] == dest)]
    got = [e[3] for e in exported if e[1] == 1 and e[2] == dest and e[5] == K_ACK and e[6] == dest]
    assert got == want, f"Acks of {dest} answer {got[:6]}.. ({len(got)}), want {want[:6]}.. ({len(want)})"
    return len(want)


B_COUNTS = (1, 7, 8, 9, 63, 64, 65, 200)
B_PLACES = ("edges", "block", "last")


def b_ids(k: int, place: str, cap: int) -> list:
    """k external ids.  edges: 127 and 128, 4095 and 4096, then the first and last id of further 128-id segments,
    ending at capacity - 1; block: consecutive ids inside one segment (k <= 65) or two adjacent ones; last: the
    last k ids up to capacity - 1."""
    if place == "block":                               # 1280..1407 is one segment: 200 ids run into the next two
        return list(range(1290, 1290 + k)) if cap > 200 else list(range(30, 30 + k))
    if place == "last":
        return list(range(cap - k, cap))
    ids = [cap - 1, 127, 128, 4095, 4096]
    for s in [(2 + 5 * q) % 63 + 1 for q in range(63)]:          # every segment but the first, far ones in turn
        ids += [s * 128, s * 128 + 127]
    ids += [s * 128 + o for s in range(1, 64) for o in (1, 126)]   # k = 200: the ids next to the edges as well
    ids += list(range(cap - 2, 130, -1)) + list(range(126, 30, -1))   # (capacity 200: the ids next to the edge)
    ids = [i for i in dict.fromkeys(ids) if i < cap]
    return sorted(ids[:k])


def case_b(k: int, place: str = "edges", cap: int = 8192, nonuniform: bool = False, stale: bool = False) -> Case:
    """Group B: k first-contact external senders ping peer 0 in one wave (round 1): k prologue insertions into a
    row whose checkpoint segments are 128 ids wide.  nonuniform: identities of 4 bytes, one never-started id with
    another length (the non-incremental path); both libraries accept identities of mixed lengths up to capacity 200
    only, so these cases are drawn at capacity 200 (190 for 8190): one segment edge, 127 | 128, and the last id.  stale: a member taught in round 1 sends, in the wave of the
    insertions (round 2 then), a KnownPeers list of two new ids in other segments."""
    if nonuniform:
        cap = 200 - (8192 - cap)
    ext = b_ids(k, place, cap)
    helper, news = (2000, [3000, 6000]) if cap > 200 else (10, [20, 129])
    idents = {5: b"another-length"} if nonuniform else {}
    cfg = base_cfg(cap, id_len=4 if nonuniform else 0)
    name = f"B{k}_{place}_{cap}" + ("_nonuniform" if nonuniform else "") + ("_stale" if stale else "")
    if not stale:
        return Case(name, cfg, ext, {0: teach(ext)}, rounds=3, identities=idents, lacks={1: {0: ext}}, exports={})
    recs = teach(ext) + [(helper, 0, K_KP, 0, 0, 0, news)]
    return Case(name, cfg, ext + [helper], {0: [ping(helper)], 1: recs}, rounds=4, identities=idents,
                contains={2: {0: [helper]}}, lacks={2: {0: ext + news}}, may_drop=True)


def case_c(slow: bool) -> Case:
    """Group C: PingRequests from members fill peer 0's curious table: 8 targets then a 9th (overflow), 4 observers
    of one target then a 5th (overflow) and one observer twice (no overflow); Acks of two targets are forwarded to
    exactly the recorded observers and free their entries; the 9th target then fits, and its Ack is forwarded.
    slow: every round carries 9 more Pings of other members, so k_proc's copy of the handlers runs, not the fast
    lane's (at most 8 records, all members)."""
    obs = [300, 301, 302, 303, 304]
    tgt = list(range(280, 289))
    pad = list(range(260, 269)) if slow else []

    def pr(o, t):
        return (o, 0, K_PINGREQ, t, 0, 0, [])

    def ack(t):
        return (t, 0, K_ACK, t, 0xC0FFEE00 + t, 1, [])

    body = {1: [pr(obs[0], t) for t in tgt[:8]],
            2: interleave({obs[1]: [pr(obs[1], tgt[8]), pr(obs[1], tgt[0])], obs[2]: [pr(obs[2], tgt[0])],
                           obs[3]: [pr(obs[3], tgt[0])], obs[4]: [pr(obs[4], tgt[0])], obs[0]: [pr(obs[0], tgt[0])]}),
            3: [ack(tgt[3]), ack(tgt[0])],
            4: [pr(obs[2], tgt[8])],
            5: [ack(tgt[8])]}
    script = {0: teach(obs + tgt + pad)}
    for r, recs in body.items():
        script[r] = interleave({**{m[0]: [q for q in recs if q[0] == m[0]] for m in recs}, **{p: [ping(p)] for p in pad}})
    np_ = len(pad)
    # round 2: 8 Pings to the targets; round 3: 6 Pings; round 4: 4 + 1 forwarded Acks; round 5: 1 Ping; round 6: 1 Ack
    return Case("C_slow" if slow else "C_fast", base_cfg(320, 1), obs + tgt + pad, script, rounds=8,
                contains={r + 1: {0: sorted({m[0] for m in script[r]})} for r in body},
                overflow={2: 0, 3: 2, 4: 2, 5: 2, 6: 2})


def spread(start: int, n: int, cap: int, step: int = 7) -> list:
    return [(start + step * j) % cap for j in range(n)]


def case_d(name: str, lists, cap: int = 8192, ext=None, stopped=(), taught=()) -> Case:
    """Group D: the KnownPeers lists [(sender, ids)] reach peer 0 in one wave (round 2; round 1 teaches `taught`).
    stopped: ids started with the mesh and stopped in round 0."""
    ext = sorted(set(ext if ext is not None else [s for s, _ in lists]))
    per = {}
    for s, ids in lists:
        per.setdefault(s, []).append((s, 0, K_KP, 0, 0, 0, list(ids)))
    cfg = replace(base_cfg(cap), initial_nodes=RUNNING + len(stopped))
    ev = {0: [("stop", i, None) for i in stopped]} if stopped else {}
    return Case(name, cfg, ext, {0: teach(taught), 1: interleave(per)}, rounds=4, events=ev,
                contains={2: {0: list(taught)}} if taught else {}, may_drop=True)


D_EXT = list(range(8100, 8133))        # 33 external ids in the row's second column part (words >= NWR/2)


def d_total(total: int) -> Case:
    """7 lists of 585 ids (4095), the last one longer by total - 4095: at 4096 ids the group is BIG."""
    lists = [(D_EXT[q], spread(200 + 1000 * q, 585 + (total - 4095 if q == 6 else 0), 8192)) for q in range(7)]
    assert sum(len(i) for _, i in lists) == total
    return case_d(f"D_total{total}", lists)


def d_dups() -> Case:
    """The duplicate-heavy BIG group: ids repeated inside a list and across lists, members (peers 1, 2, taught
    externals), peer 0 itself, other lists' senders (arm-then-prologue: Known(now), not Known(r - 10)), a stopped
    id (3) and external ids."""
    s = D_EXT[:12]
    common = spread(500, 300, 8192, 13)
    lists = []
    for q, x in enumerate(s):
        ids = common + common[:50] + [0, 1, 2, 3] + s + D_EXT[20:24] + spread(40 * q, 40, 8192, 3)
        lists.append((x, ids))
    assert sum(len(i) for _, i in lists) >= KP_BIG
    return case_d("D_dups", lists, ext=D_EXT, stopped=(3,), taught=D_EXT[:4])


def d_colsplit() -> Case:
    """Capacity 8192: the row is NWR = 256 words, a BIG group's two workgroups own words [0, 128) and [128, 256).
    Ids in words 127 and 128 (4064..4127), senders below 4096 that list only ids at or above 4096 and the
    converse, every id of both border words, and enough further ids for a BIG group.  The suspect slot whose peer lies
    in the second part is not drawn here (a suspicion depends on the A3 draw, so it needs a reactive script): F_kp_big
    has it, at capacity 8192 with the suspected peers at ids 5000.. and a BIG group over both parts."""
    lo_s, hi_s = [4000, 4063, 4095], [4096, 4127, 8191]
    lists = [(x, list(range(4096, 4128)) + spread(4200 + 700 * q, 700, 8192 - 4200, 1)) for q, x in enumerate(lo_s)]
    lists = [(x, [4096 + (i - 4096) % 4096 for i in ids]) for x, ids in lists]
    lists += [(x, list(range(4064, 4096)) + spread(100 + 700 * q, 700, 4000, 1)) for q, x in enumerate(hi_s)]
    for x, ids in lists:
        assert all((i >= 4096) != (x >= 4096) for i in ids)
    assert sum(len(i) for _, i in lists) >= KP_BIG
    return case_d("D_colsplit", lists)


D_LENGTHS = (1, 63, 64, 65, 639, 640, 641, 1281)


def d_lengths(big: bool) -> Case:
    """One list of each length (the oracle delivers an injected list of any length: the datagram limit of 10240 B,
    kp_cap_uniform = 568 ids of 18 B, binds what a simulated peer sends, src/kaboodle.rs KnownPeersRequest reply,
    not what an external peer injects): 1, 63, 64, 65, and 639, 640, 641, 1281 around the BIG body's 640-id chunk.
    3394 ids in all: a small group; big adds the longest list there is, every id of the row (8192)."""
    lists = [(D_EXT[q], spread(37 * q, n, 8192, 5)) for q, n in enumerate(D_LENGTHS)]
    if big:
        lists.append((D_EXT[8], list(range(8192))))
    return case_d("D_lengths_big" if big else "D_lengths_small", lists)


D_COUNTS = (1, 16, 17, 1024, 1025)


def d_count(m: int) -> Case:
    """m lists in one BIG group (32 externals x 33 records reach 1025 > the 64 x 16 messages a BIG workgroup fetches
    per step), each of ceil(4096 / m) ids (at least 4)."""
    n = max(4, -(-KP_BIG // m))
    ext = D_EXT[:32] if m > 1 else D_EXT[:1]
    lists = [(ext[q % len(ext)], spread(11 * q, n, 8192, 17)) for q in range(m)]
    return case_d(f"D_count{m}", lists)


def d_small(m: int) -> Case:
    """The small-group body: m lists of 3 ids to peer 0, the first of them the next list's sender (arm, then
    prologue: Known(now))."""
    lists = [(D_EXT[q % 33], [D_EXT[(q + 1) % 33]] + spread(50 * q, 2, 8192, 9)) for q in range(m)]
    return case_d(f"D_small{m}", lists, cap=8192)


def d_many_dests(ndest: int = 1100) -> Case:
    """More than 1024 destinations with a small group each in one wave (one fill of the small body's LDS list is
    1024): a converged mesh of ndest peers, 34 externals x 33 lists of 2 ids, one list per destination."""
    cap = ndest + 100
    ext = list(range(ndest + 10, ndest + 44))
    per = {x: [] for x in ext}
    for dst in range(ndest):
        x = ext[dst % len(ext)]
        per[x].append((x, dst, K_KP, 0, 0, 0, [ext[(dst + 1) % len(ext)], (dst + 500) % ndest]))
    cfg = SimConfig(capacity=cap, initial_nodes=ndest, init_mode=KB_INIT_CONVERGED, seed=5)
    return Case("D_many_dests", cfg, ext, {0: interleave(per)}, rounds=2, dests=tuple(range(ndest)),
                lacks={1: {d: ext for d in (0, 1023, 1024, ndest - 1)}})


E_PINGS = (1, 8, 9, 65)
E_JOINER = 7801                        # the external peer whose Join is injected: named by no list of the group


def case_e(m: int, join: bool) -> Case:
    """Group E: a BIG KnownPeers group (8 lists of 600 ids) and m Pings of taught members reach peer 0 in the same
    wave 0.  join: an external peer's Join broadcast is injected in the same gap, so the round has a Join list and
    wave 0 splits (the BIG group on the side stream, peer 0's in-order inbox in the deferred k_proc pass)."""
    kp = [(D_EXT[q], spread(300 + 900 * q, 600, 8192)) for q in range(8)]
    pingers = list(range(7000, 7000 + m))
    per = {x: [ping(x)] for x in pingers}
    for s, ids in kp:
        per.setdefault(s, []).append((s, 0, K_KP, 0, 0, 0, ids))
    recs = interleave(per)
    assert all(E_JOINER not in ids for _, ids in kp)
    if join:
        recs.append((E_JOINER, 0, K_JOIN, 0, 0, 0, []))
    return Case(f"E{m}" + ("_join" if join else ""), base_cfg(8192, 1), sorted(set(D_EXT + pingers + [E_JOINER])),
                {0: teach(pingers), 1: recs}, rounds=4, contains={2: {0: pingers}}, may_drop=True)


F_KINDS = ("ack_fast", "ack_proc", "kp_small", "kp_big")


def case_f(kind: str) -> Case:
    """Group F: three running peers that know five external peers (second column part of a capacity-8192 row).  The
    A3 ping soon picks an external peer and marks it WaitingForPing; the reactive script answers one round late from
    exactly that peer: an Ack alone (fast lane), an Ack among 9 Pings of other members (k_proc), a KnownPeers
    envelope of 3 ids (k_kp's small body) or of 4096 ids (its BIG body).  The prologue frees the suspect slot and
    samples the latency: 1000 ms per round late plus the wave's millisecond."""
    ext = [5000, 5001, 5002, 5003, 5004]
    pad = list(range(6000, 6009)) if kind == "ack_proc" else []

    def script(r, o, exported):
        if r == 0:
            return [q for i in range(RUNNING) for q in teach(ext + pad, i)]
        out = []
        for i in range(RUNNING):
            for peer, _, since in o.suspects(i):
                if peer in ext and since == r and (peer, i) not in [(m[0], m[1]) for m in out]:
                    if kind.startswith("ack"):
                        out.append((peer, i, K_ACK, peer, 0xC0FFEE00 + peer, 1, []))
                    else:
                        out.append((peer, i, K_KP, 0, 0, 0, spread(17 * r, 3 if kind == "kp_small" else KP_BIG, 8192)))
        if out and pad:
            per = {p: [ping(p, i) for i in sorted({m[1] for m in out})] for p in pad}
            for m in out:
                per.setdefault(m[0], []).append(m)
            out = interleave(per)
        return out

    return Case(f"F_{kind}", base_cfg(8192, track_latency=1), ext + pad, script, rounds=8, dests=(0, 1, 2),
                may_drop=kind.startswith("kp"))
