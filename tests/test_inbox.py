"""The crafted wave-0 inboxes of tests/inbox.py on the oracle alone: every case is what it claims.  Every injected
record is delivered (no drop counter moves in a delivering round, the sent counters rise by the number injected), the
destination's view before the round contains, or lacks, the senders the case needs, and the expected answers are
exported.  tests/test_gpu_inbox.py runs the same cases on the HIP library."""
import pytest

import inbox
from inbox import K_ACK, K_KP, K_KPR, K_PING, K_PINGREQ


def all_cases():
    """Every crafted case by name (the GPU file draws from the same table)."""
    cs = [inbox.case_a(n) for n in inbox.A_SIZES]
    cs += [inbox.case_a(n, mixed=True) for n in inbox.A_MIXED]
    cs += [inbox.case_a(8, flavor=f) for f in ("nonmember", "stale")]
    cs += [inbox.case_a(n, flavor="unsorted") for n in inbox.A_UNSORTED]
    cs += [inbox.case_b(*a) for a in B_ARGS]
    cs += [inbox.case_c(False), inbox.case_c(True)]
    cs += [inbox.d_total(4095), inbox.d_total(4096), inbox.d_dups(), inbox.d_colsplit(), inbox.d_lengths(False),
           inbox.d_lengths(True)]
    cs += [inbox.d_count(m) for m in inbox.D_COUNTS] + [inbox.d_small(m) for m in (1, 64, 65)] + [inbox.d_many_dests()]
    cs += [inbox.case_e(m, j) for m in inbox.E_PINGS for j in (True, False)]
    cs += [inbox.case_f(k) for k in inbox.F_KINDS]
    return {c.name: c for c in cs}


# group B: (k, placement, capacity, non-uniform identities, stale checkpoints).  Every k at the segment edges, every
# placement at the lane-parallel threshold (7, 8, 9) and past one wave (65), then the other capacity, the
# non-incremental path and the stale checkpoints at both sides of each threshold
B_ARGS = [(k, "edges", 8192, False, False) for k in inbox.B_COUNTS] + \
         [(k, p, 8192, False, False) for k in (7, 8, 9, 65) for p in ("block", "last")] + \
         [(k, "last", 8190, False, False) for k in (1, 8, 9, 200)] + \
         [(k, "edges", 8192, True, False) for k in (1, 8, 9, 65)] + [(9, "last", 8190, True, False)] + \
         [(k, "edges", 8192, False, True) for k in (7, 8, 64, 65)] + [(9, "block", 8192, False, True),
                                                                       (200, "last", 8190, False, True)]
# (no stale case with non-uniform identities: such a mesh keeps no checkpoints, there is nothing to be stale)
CASES = all_cases()


def test_case_names_are_unique():
    assert len(CASES) == len(inbox.A_SIZES) + len(inbox.A_MIXED) + 2 + len(inbox.A_UNSORTED) + len(B_ARGS) + 2 + 6 + len(inbox.D_COUNTS) + 3 + 1 + \
        2 * len(inbox.E_PINGS) + len(inbox.F_KINDS)


@pytest.mark.parametrize("name", list(CASES))
def test_conditions(name):
    """Delivered, membership before the round, nothing dropped: inbox.check_conditions."""
    got = inbox.check_conditions(CASES[name])
    assert got["injected"] > 0


@pytest.mark.parametrize("name", [n for n in CASES if n[0] == "A"])
def test_a_inbox_length_and_answers(name):
    """Peer 0's in-order inbox of round 2 is exactly the n crafted records (the oracle's Ack for every Ping comes
    back in wave 1 in (sender, seq) order), every KnownPeersRequest draws a KnownPeers reply, and before the round
    peer 0's fingerprint is current and every sender but the case's non-member is in its view."""
    case = CASES[name]
    tr = inbox.oracle_trace(case)
    recs = tr[1][3]
    n = int(name[1:].split("_")[0])
    recs = [m for m in recs if m[1] != case.sink]               # (the unsorted cases' fillers go to an external sink)
    assert sum(1 for m in recs if m[2] != K_KP) == n and all(m[1] == 0 for m in recs)
    if name.endswith("unsorted"):
        per = {}
        for m in recs:
            per[m[0]] = per.get(m[0], 0) + 1
        low, high = [x for x in per if x < 128], [x for x in per if x >= 128]
        # low senders behind 66 filler records in their scatter wave, high senders in other waves, several records each
        assert low and high and min(low) >= 66 and max(per.values()) >= min(3, n // 4)
        assert [m[0] for m in tr[1][3] if m[1] == case.sink] .count(64) == 33 == [m[0] for m in tr[1][3] if m[1] == case.sink].count(65)
    assert tr[2][1]["scalars"][:, 0].sum() == 1                  # peer 0 runs alone: nobody else can address it
    npings = inbox.acks_in_order(recs, tr[2][2])
    assert npings == sum(1 for m in recs if m[2] == K_PING) and (npings == n or "mixed" in name)
    kpr = sorted(m[0] for m in recs if m[2] == K_KPR)
    assert sorted(e[3] for e in tr[2][2] if e[1] == 1 and e[5] == K_KP) == kpr
    if "mixed" in name:
        kinds = {m[2] for m in recs}
        assert kinds == {K_PING, K_PINGREQ, K_ACK, K_KPR}
        per = {}
        for m in recs:
            per.setdefault(m[0], []).append(m[2])
        assert any(len(set(v)) > 1 for v in per.values())        # seq order inside a sender matters
        # every PingRequest was served: a Ping to its target, exported with the wave's other answers
        fwd = [e for e in tr[2][2] if e[1] == 1 and e[2] == 0 and e[5] == K_PING]
        assert len(fwd) == sum(1 for m in recs if m[2] == K_PINGREQ) > 0 and {e[3] for e in fwd} == {case.externals[0]}
    if name.endswith("stale"):
        assert tr[3][0][0] >= {case.cfg.capacity - 1}           # the list's id arrived


@pytest.mark.parametrize("name", [n for n in CASES if n[0] == "B"])
def test_b_insertions(name):
    """Every one of the k senders is new to peer 0 before the wave and a member after it; each Ping was answered."""
    case = CASES[name]
    tr = inbox.oracle_trace(case)
    r = 2 if name.endswith("stale") else 1
    recs = tr[r - 1][3]
    senders = {m[0] for m in recs if m[2] == K_PING}
    k = int(name[1:].split("_")[0])
    assert len(senders) == k and not senders & tr[r][0][0] and senders <= tr[r + 1][0][0]
    assert inbox.acks_in_order(recs, tr[r][2]) == k
    if name.endswith("stale"):
        news = next(m[6] for m in recs if m[2] == K_KP)
        assert len(news) == 2 and set(news) <= tr[r + 1][0][0] and not set(news) & tr[r][0][0]
        assert len({i // 128 for i in news} | {i // 128 for i in senders}) > 1
    if "nonuniform" in name:
        assert case.identities and len(next(iter(case.identities.values()))) != case.cfg.id_len


@pytest.mark.parametrize("name", ["C_fast", "C_slow"])
def test_c_curious_table(name):
    """The table holds 8 targets after round 2; round 3 overflows twice (9th target, 5th observer) and not for the
    repeated observer; round 4 forwards the two Acks to exactly the recorded observers (4 and 1) and frees the
    entries; the 9th target then fits (round 5) and its Ack is forwarded (round 6)."""
    case = CASES[name]
    tr = inbox.oracle_trace(case)
    assert tr[2][1]["scalars"][:, 0].sum() == 1                  # peer 0 runs alone: its inbox is the script's
    obs, tgt = case.externals[:5], case.externals[5:14]
    cur = lambda r: {e[0]: [x for x in e[2:] if x >= 0] for e in tr[r][1]["cur"][0]}
    assert cur(2) == {t: [obs[0]] for t in tgt[:8]}
    assert cur(3)[tgt[0]] == obs[:4] and tgt[8] not in cur(3) and len(cur(3)) == 8
    fwd = [(e[3], e[6]) for e in tr[4][2] if e[2] == 0 and e[5] == K_ACK and e[1] == 1 and e[6] != 0]
    assert fwd == [(o, tgt[0]) for o in obs[:4]] + [(obs[0], tgt[3])], fwd
    assert set(cur(4)) == set(tgt[1:8]) - {tgt[3]}
    assert cur(5)[tgt[8]] == [obs[2]]
    assert [(e[3], e[6]) for e in tr[6][2] if e[2] == 0 and e[5] == K_ACK and e[1] == 1 and e[6] != 0] == [(obs[2], tgt[8])]
    assert tgt[8] not in cur(6)
    for r in range(2, 7):
        n = len(tr[r - 1][3])
        assert (n > inbox.FAST_MAX) == (name == "C_slow"), (r, n)


@pytest.mark.parametrize("name", [n for n in CASES if n[0] == "D" and n != "D_many_dests"])
def test_d_groups(name):
    """The lists' total payload is on the side of KP_BIG the case names, and peer 0's view after the wave is its
    view before plus every sender and every listed id (itself included: it is a member of its own view)."""
    case = CASES[name]
    tr = inbox.oracle_trace(case)
    recs = tr[1][3]
    assert all(m[2] == K_KP and m[1] == 0 for m in recs)
    total = sum(len(m[6]) for m in recs)
    big = name in ("D_total4096", "D_dups", "D_colsplit", "D_lengths_big") or name.startswith("D_count")
    assert (total >= inbox.KP_BIG) == big, total
    if name.startswith("D_total"):
        assert total == int(name[7:])
    if name.startswith("D_count") or name.startswith("D_small"):
        assert len(recs) == int(name[7:])
    want = set(tr[2][0][0]) | {m[0] for m in recs} | {i for m in recs for i in m[6]}
    assert tr[3][0][0] == want
    if name == "D_dups":
        ids = [i for m in recs for i in m[6]]
        assert len(ids) > 2 * len(set(ids)) and {0, 1, 2, 3} <= set(ids) and {m[0] for m in recs} <= set(ids)
        assert not tr[3][1]["scalars"][3, 0]                      # id 3 is stopped
        row = inbox.row_of(tr[3][1], 0)
        assert len({int(row[m[0]]) for m in recs}) == 1 and row[recs[0][0]] != row[ids[0]]   # senders Known(now)
    if name == "D_colsplit":
        words = {i >> 5 for m in recs for i in m[6]}
        assert {127, 128} <= words and all((m[0] >= 4096) != (i >= 4096) for m in recs for i in m[6])


def test_d_many_destinations():
    case = CASES["D_many_dests"]
    tr = inbox.oracle_trace(case)
    assert len({m[1] for m in tr[0][3]}) > 1024 and all(len(m[6]) == 2 for m in tr[0][3])
    for m in tr[0][3][::97]:
        assert m[0] not in tr[1][0][m[1]] and m[0] in set(inbox.row_of(tr[1][1], m[1]).nonzero()[0])


@pytest.mark.parametrize("name", [n for n in CASES if n[0] == "E"])
def test_e_group_and_pings(name):
    case = CASES[name]
    tr = inbox.oracle_trace(case)
    recs = tr[1][3]
    m = int(name[1:].split("_")[0])
    assert sum(len(q[6]) for q in recs if q[2] == K_KP) >= inbox.KP_BIG and tr[2][1]["scalars"][:, 0].sum() == 1
    assert inbox.acks_in_order(recs, tr[2][2]) == m
    # round 2 has a Join list exactly in the join cases: the external joiner, named by no list and sender of no
    # record, is in peer 0's view after the round (the Join broadcast's insertion) and only then
    joiner = inbox.E_JOINER
    assert ("join" in name) == any(q[2] == inbox.K_JOIN and q[0] == joiner for q in recs)
    assert all(joiner not in q[6] and q[0] != joiner for q in recs if q[2] != inbox.K_JOIN)
    assert (joiner in tr[3][0][0]) == ("join" in name) and joiner not in tr[2][0][0]
    assert not [b for b in tr[2][1]["bcasts"] if b[0] == "Join"]     # (and peer 0 itself broadcasts none)


@pytest.mark.parametrize("name", [n for n in CASES if n[0] == "F"])
def test_f_late_answers(name):
    """The script answered at least one suspicion, the slot was free after the answer's round, and the oracle
    measured about 1000 ms (1000 per round late + the wave's millisecond)."""
    case = CASES[name]
    tr = inbox.oracle_trace(case)
    answered = [(r, m) for r in range(case.rounds - 1) for m in tr[r][3] if r > 0 and m[2] in (K_ACK, K_KP)]
    assert answered
    lat = set()
    for r, m in answered:
        x, i = m[0], m[1]
        assert (x, 1, r) in tr[r][1]["susp"][i], (r, m[:3], tr[r][1]["susp"][i])
        assert all(e[0] != x for e in tr[r + 1][1]["susp"][i])
        lat |= {e[3] for e in tr[r + 1][1]["peer_states"][i] if e[0] == x}
    assert lat and all(1001 <= v <= 1009 for v in lat), lat
    kind = name[2:]
    for r, m in answered:
        n = sum(1 for q in tr[r][3] if q[1] == m[1] and q[2] != K_KP)
        if kind == "ack_fast":        # the two other running peers may each ping this one in the same wave
            assert n + (inbox.RUNNING - 1) <= inbox.FAST_MAX
        elif kind == "ack_proc":
            assert n > inbox.FAST_MAX
        else:
            assert (len(m[6]) >= inbox.KP_BIG) == (kind == "kp_big")
