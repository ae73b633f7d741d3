"""The sparse rows' list code on rows the scenarios never produce (kaboodle_amd/csrc/kb_sparse.h): a snapshot of a
reachable state is re-encoded row by row under the other value of `based` (tests/snapedit.py), restored, and must go
on in lock step with the sparse CPU oracle, which knows nothing of the edit.

`based` is a representation flag: `based = 1` rows hold x where membership differs from the base, `based = 0` rows
hold x on every member.  k_sp_init sets it once per id and it is only ever copied, so a run takes one branch per row:
the `based` branch on short rows (the base plus a few exceptions), the `!based` branch on the few joiner rows.
Re-encoded, the same views run sp_ins_at / sp_del_at, sp_lb / sp_look, sp_a2_select, sp_a3_range, sp_members, sp_fold,
k_sp_rebase and k_sp_jresp in the other branch, on lists hundreds of entries long.

Encodings: none_based (every row `based = 0`), all_based (every row 1, the joiners' too), flipped (every flag
inverted), odd_flipped (the odd ids').  With sparse_row_cap = 0 and these capacities ECAP = C: every encoding fits.
"""
from __future__ import annotations

import numpy as np
import pytest

import parity
import pyref
import snapedit
from kaboodle_amd._ffi import KB_CAPACITY, KB_INIT_CONVERGED, KB_VARIANT_SPARSE_ROWS, KbError, Sim, SimConfig
from test_gpu_snapshot import SPLITS, run_to
from test_gpu_sparse import TRUNC_CASES

pytestmark = pytest.mark.gpu

STD = {n: (c, r) for n, c, r in parity.standard_cases()}
# The two highest members of a loss-free converged mesh stop, one after the other: every row removes them at the end
# of its list (under none_based: entries 63 of 64, then 62 of 63), the deletes inside the last 16-byte group that the
# standard cases hardly ever make (tests/test_snapedit.py, test_shift_positions_are_covered)
EXTRA = {"tail_stops": ({"cfg": SimConfig(capacity=72, initial_nodes=64, init_mode=KB_INIT_CONVERGED, seed=5),
                         "events": {2: [("stop", 63, None)], 8: [("stop", 62, None)]}}, 16),
         # A row's entry for its own id is the Known stamp of its start; the stamp window's third rebase (round 192)
         # makes it implicit, and only from then on does a `based` row hold itself inside a gap between entries: the
         # self_in correction of sp_a2_select, which no shorter lossy run reaches.  Split just before that rebase; the
         # rows are all `based`, so all_based restores them as they are and none_based is the other branch.
         "late_self": ({"cfg": SimConfig(capacity=64, initial_nodes=64, init_mode=KB_INIT_CONVERGED, loss=0.1, seed=41)},
                       204)}
ALL4 = ("none_based", "all_based", "flipped", "odd_flipped")
TWO = ("none_based", "flipped")
# (case, the last round before the snapshot, encodings).  partition_heal is also split at round 2, the last round
# before the cut (partition_start = 3); trunc_1200 after round 1, with sampled Join responses still to come.
CASES = (("churn_loss_512", SPLITS["churn_loss_512"], ALL4), ("partition_heal", SPLITS["partition_heal"], ALL4),
         ("partition_heal", 2, TWO), ("stop_start", SPLITS["stop_start"], TWO), ("old_stamps", SPLITS["old_stamps"], TWO),
         ("identity_change", SPLITS["identity_change"], TWO), ("fresh_ids", SPLITS["fresh_ids"], TWO),
         ("probes", SPLITS["probes"], TWO), ("tail_stops", 1, TWO), ("late_self", 190, ("all_based", "none_based")),
         ("trunc_1200", 1, ("none_based",)))
PARAMS = [(n, s, e) for n, s, encs in CASES for e in encs]


def case_of(name: str) -> tuple[dict, int]:
    case, rounds = TRUNC_CASES[name] if name in TRUNC_CASES else EXTRA[name] if name in EXTRA else STD[name]
    return parity.with_cfg(case, variant=KB_VARIANT_SPARSE_ROWS, track_latency=0), rounds


def oracle_to(case: dict, split: int, drain: bool = True) -> Sim:
    """The oracle after round `split`; drained of its ProbeResponses, as a restored handle is (outputs do not travel)."""
    o = Sim(parity.oracle_lib(), case["cfg"])
    parity.setup(o, case)
    run_to((o,), case, 0, split)
    if drain:
        o.probe_responses()
    return o


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


_BLOBS: dict = {}


def source_blob(lib, name: str, split: int) -> bytes:
    """The GPU's own snapshot of the case after round `split` (equal to the oracle there), taken once per module."""
    if (name, split) not in _BLOBS:
        case, _ = case_of(name)
        o = oracle_to(case, split, drain=False)
        with Sim(lib, case["cfg"]) as a:
            parity.setup(a, case)
            run_to((a,), case, 0, split)
            assert parity.diff_states(parity.state_of(o), parity.state_of(a)) == []
            _BLOBS[name, split] = a.snapshot()
        o.close()
    return _BLOBS[name, split]


def reencoded(blob: bytes, enc: str, what: str) -> bytes:
    snap = snapedit.load(blob)
    flags = snapedit.encoding(snap, enc)
    out = snapedit.reencode(snap, flags)
    changed = sum(int(snap["sections"]["BASED"][i]) != f for i, f in flags.items())
    print(f"REENCODED {what} {enc}: {changed} of {len(snap['rows'])} rows change their flag, longest list "
          f"{max(len(r) for r in snap['rows'])} -> {max(len(r) for r in out['rows'])} entries, "
          f"{snap['entries']} -> {out['entries']} entries in all")
    return snapedit.dump(out)


def same_at_rest(o: Sim, b: Sim) -> None:
    """rows, suspects, curious, scalars, stats, fingerprints, true_fingerprint; peers and peer_states of every id."""
    assert parity.diff_states(parity.state_of(o), parity.state_of(b)) == []
    for i in range(o.capacity):
        assert o.peers(i) == b.peers(i), f"peers[{i}]"
    assert parity.diff_peer_states(o, b, range(o.capacity)) == []


def spare_id(blob: bytes):
    """The highest id that never started, has no identity set and is no external peer (None: every id is taken)."""
    s = snapedit.load(blob)["sections"]
    free = (s["START_ROUND"] == snapedit.NONE_ROUND) & (s["IDSET"].ravel() == 0) & (s["EXT"].ravel() == 0) & (s["MOVED"].ravel() == 0)
    ids = np.flatnonzero(free)
    return int(ids[-1]) if len(ids) else None


def folds_are_zlib(o: Sim, b: Sim, blob: bytes) -> None:
    """fingerprints() of the handle equal the oracle's, and for a dozen running rows (the joiners' among them) the
    literal zlib fold of peers(i): sp_fold read against generate_fingerprint, not against another fold."""
    fo, fb = o.fingerprints(), b.fingerprints()
    assert np.array_equal(fo, fb), np.flatnonzero(fo != fb)[:8]
    ident = [b.identity(j) for j in range(b.capacity)]
    nb = int(snapedit.base_bits(snapedit.load(blob)["cfg"]).sum())
    run = [i for i in range(b.capacity) if b.is_running(i)]
    low, high = [i for i in run if i < nb], [i for i in run if i >= nb]
    pick = high[:: max(1, len(high) // 6)][:6]
    pick += low[:: max(1, len(low) // (12 - len(pick)))][: 12 - len(pick)]
    assert len(pick) >= min(12, len(run))
    for i in pick:
        assert int(fb[i]) == pyref.fingerprint(b.peers(i), ident), f"row {i}"


def restore_and_follow(gpu, name: str, split: int, enc: str, shards: int = 0) -> None:
    """At rest the restored handle equals the oracle in everything the inspection surface reads.  Then every fold is
    forced: set_identity on a never-started spare id (an identity of the others' length) marks every row stale on both
    implementations, and fingerprints() must equal the oracle's and the zlib fold of peers(i).  Where every id is
    taken (partition_heal, and the churn cases once their fresh ids are used up) that call would be refused, and the
    same fold check runs after the first continued round instead, on the rows that round dirtied; it runs there in
    every case.  Then the case's remaining rounds in lock step: diff_states with full rows and diff_peer_states of
    every id, every round."""
    case, rounds = case_of(name)
    src = source_blob(gpu, name, split)
    o = oracle_to(case, split)
    b = Sim.restore(gpu, reencoded(src, enc, f"{name}@{split}"), shards=shards)
    assert b.stats()["round"] == split + 1
    before = o.stats()["join_responses"]
    same_at_rest(o, b)
    spare = spare_id(src)
    if spare is not None:
        for s in (o, b):
            s.set_identity(spare, bytes([0x51]) * case["cfg"].id_len)
        folds_are_zlib(o, b, src)
    for r in range(split + 1, rounds):
        run_to((o, b), case, r, r)
        assert parity.diff_states(parity.state_of(o), parity.state_of(b)) == [], f"round {r}"
        assert parity.diff_peer_states(o, b, range(o.capacity)) == [], f"round {r}"
        if r == split + 1:
            folds_are_zlib(o, b, src)
    if name in TRUNC_CASES:                            # sampled Join responses were walked on the re-encoded rows
        assert b.stats()["join_responses"] > before
    o.close()
    b.close()


@pytest.mark.parametrize("name,split,enc", PARAMS, ids=[f"{n}@{s}-{e}" for n, s, e in PARAMS])
def test_reencoded_continuation(gpu, name, split, enc):
    restore_and_follow(gpu, name, split, enc)


def test_reencoded_restart_across_shards(gpu):
    """stop_start, flipped, restored as 3 row shards: the restarts of rounds 14 move rows between shards, and
    k_sp_row_pack / k_sp_row_unpack carry the flag with the row."""
    restore_and_follow(gpu, "stop_start", SPLITS["stop_start"], "flipped", shards=3)


# ---- the row cap at its exact edge -------------------------------------------------------------------------------
# A converged, loss-free, churn-free mesh: nothing is ever removed, so entry lists only grow (until the stamp window's
# first rebase at round 64).  Id 70 starts before round 2 and id 71 before round 6; 71's Join is delivered in round 7,
# where every running row inserts it.  The snapshot is taken after round 6.
EDGE = {"cfg": SimConfig(capacity=72, initial_nodes=64, init_mode=KB_INIT_CONVERGED, seed=2, variant=KB_VARIANT_SPARSE_ROWS),
        "events": {2: [("start", 70, None)], 6: [("start", 71, None)]}}
EDGE_SPLIT = 6


def entry_ids(rows, flags, base) -> list:
    return [(snapedit.encode_row(rows[i], flags[i], base) >> 9).tolist() for i in range(len(rows))]


@pytest.mark.parametrize("enc", ["based", "none_based"])
def test_row_cap_edge(gpu, enc):
    """M = the longest entry list after round 7 under the encoding, counted by encode_row over the oracle's rows.
    Restored with sparse_row_cap = M the round runs in parity; with M - 1 the step is KB_CAPACITY and the handle
    does not step on.  `based`: the snapshot as the engine wrote it, the longest row a `based = 1` row (asserted).
    none_based: every row lists its 65 members and grows to M = 66; in round 8 every row is at its cap and only
    restamps entries it holds (asserted from the oracle), which is no error.  A `based = 1` row at the longest length
    has no such round: its A3 ping goes to an ancient member, which has no entry yet, so the row grows every round."""
    src = source_blob_edge(gpu)
    snap = snapedit.load(src)
    base = snapedit.base_bits(snap["cfg"])
    flags = [int(f) for f in snap["sections"]["BASED"]] if enc == "based" else [0] * 72
    edited = snapedit.reencode(snap, dict(enumerate(flags)))
    o = oracle_to(EDGE, EDGE_SPLIT)
    rows = [o.rows()]
    for r in (7, 8):
        run_to((o,), EDGE, r, r)
        rows.append(o.rows())
    ids = [entry_ids(rw, flags, base) for rw in rows]
    assert ids[0] == [(e >> 9).tolist() for e in edited["rows"]]          # the restored lists are the oracle's
    assert all(set(a) >= set(b) for a, b in zip(ids[1], ids[0])), "round 7 is not grow-only"
    longest = [max(len(x) for x in step) for step in ids]
    M = longest[1]
    assert M > longest[0], longest
    top = [i for i in range(72) if len(ids[1][i]) == M]
    if enc == "based":
        assert all(flags[i] == 1 for i in top), top
    print(f"ROW CAP {enc}: longest list {longest[0]} -> M = {M} (rows {top[:6]}), then {longest[2]}")

    o = oracle_to(EDGE, EDGE_SPLIT)
    b = Sim.restore(gpu, snapedit.dump(snapedit.with_row_cap(edited, M)))
    same_at_rest(o, b)
    run_to((o, b), EDGE, 7, 7)
    assert parity.diff_states(parity.state_of(o), parity.state_of(b)) == []
    assert parity.diff_peer_states(o, b, range(72)) == []
    if enc == "none_based":
        same = [i for i in top if ids[2][i] == ids[1][i] and (rows[2][i] != rows[1][i]).any()]
        assert longest[2] == M and same, (longest, same)
        i = same[0]
        j = int(np.flatnonzero(rows[2][i] != rows[1][i])[0])
        assert j in ids[1][i]                                             # row i, at its cap, restamps id j
        run_to((o, b), EDGE, 8, 8)
        assert parity.diff_states(parity.state_of(o), parity.state_of(b)) == []
        assert b.row(i)[j] == rows[2][i][j] != rows[1][i][j]
    b.close()
    o.close()

    b = Sim.restore(gpu, snapedit.dump(snapedit.with_row_cap(edited, M - 1)))
    for _ in range(2):                                                    # the round, then the refusal to step on
        with pytest.raises(KbError) as e:
            b.step(1)
        assert e.value.code == KB_CAPACITY
    b.close()


def source_blob_edge(lib) -> bytes:
    if "edge" not in _BLOBS:
        o = oracle_to(EDGE, EDGE_SPLIT)
        with Sim(lib, EDGE["cfg"]) as a:
            run_to((a,), EDGE, 0, EDGE_SPLIT)
            assert parity.diff_states(parity.state_of(o), parity.state_of(a)) == []
            _BLOBS["edge"] = a.snapshot()
        o.close()
    return _BLOBS["edge"]
