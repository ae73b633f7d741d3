"""tests/snapedit.py, the plain-Python reader and writer of snapshot format 1, without a GPU: the committed golden
snapshot round-trips byte for byte and decodes to the oracle's rows; encode_row / logical_row are inverse under both
values of `based`; every re-encoding of the golden file passes the library's validation; the rows a restore refuses
(kb_snapshot.h, sn_check_values); and the condition on the inputs of tests/test_gpu_sparse_reencoded.py, computed
from the oracle alone: its continuation cases shift rows at every position modulo a 16-byte group."""
from __future__ import annotations

import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest

import parity
import snapedit
from kaboodle_amd._ffi import KB_INVALID_ARGUMENT, KB_NO_DEVICE, KB_VARIANT_SPARSE_ROWS, KbError, Sim
from kaboodle_amd import snapshot
from parity import GPU_SO
from test_gpu_snapshot import run_to
from test_gpu_sparse_reencoded import ALL4, CASES, case_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "snapshot_v1_fresh_ids.bin")
built = pytest.mark.skipif(not os.path.exists(GPU_SO), reason="HIP library not built (run __graft_entry__.build())")


def golden() -> bytes:
    with open(GOLDEN, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    return parity.gpu_lib()


def test_round_trip():
    blob = golden()
    snap = snapedit.load(blob)
    assert snapedit.dump(snap) == blob
    assert snap["round"] == 7 and snap["entries"] == sum(len(r) for r in snap["rows"])
    assert len(snapedit.SECTIONS) == 24 and set(snap["sections"]) | {"ENTRIES"} == set(snapedit.NAMES)
    # the engine's own encoding is encode_row's: rewriting every row under the flag it has changes no byte
    same = snapedit.reencode(snap, {i: int(f) for i, f in enumerate(snap["sections"]["BASED"])})
    assert snapedit.dump(same) == blob


def test_sections_are_sn_layout():
    """The element sizes against the table in sn_layout (kb_snapshot.h), read from the source."""
    import re
    text = open(os.path.join(ROOT, "kaboodle_amd", "csrc", "kb_snapshot.h")).read()
    names = re.search(r"enum SnId : uint32_t \{(.*?)\};", text, re.S).group(1).replace("\n", " ")
    assert [n.strip()[3:] for n in names.split(",")][:-1] == list(snapedit.NAMES)
    elems = re.search(r"const uint32_t elem\[SN_NSEC\] = \{(.*?)\};", text, re.S).group(1)
    consts = {"sizeof(SnScalars)": 56, "kb::SLOTS": 8, "kb::CSLOTS": 8, "kb::PAQ": 8, "kb::MAXID": 32}
    got = []
    for term in elems.replace("\n", " ").split(","):
        v = 1
        for f in term.split("*"):
            v *= consts.get(f.strip()) or int(f)
        got.append(v)
    assert got == [e for _, e in snapedit.SECTIONS]


def test_decoder_against_the_oracle():
    """logical_row of every row of the golden file = the sparse oracle's rows() after round 6 of fresh_ids."""
    snap = snapedit.load(golden())
    case, _ = case_of("fresh_ids")
    with Sim(parity.oracle_lib(), case["cfg"]) as o:
        parity.setup(o, case)
        run_to((o,), case, 0, 6)
        want = o.rows()
    base = snapedit.base_bits(snap["cfg"])
    assert base.sum() == 48 and base[:48].all()          # a converged start: ids < initial_nodes
    for i in range(64):
        assert np.array_equal(snapedit.logical_row(snap, i), want[i]), i


def test_base_bits():
    cfg = snapedit.load(golden())["cfg"]
    assert snapedit.base_bits(cfg).tolist() == [True] * 48 + [False] * 16
    cfg.init_mode = 0                                    # a join start: every row is "based" on an empty base
    assert not snapedit.base_bits(cfg).any()


def edge_rows(Cn: int, base: np.ndarray, rng) -> dict:
    nb = np.flatnonzero(base)
    out = {"empty": np.zeros(Cn, np.uint8), "full": np.full(Cn, 2, np.uint8)}
    out["only 0"] = out["empty"].copy(); out["only 0"][0] = 77
    out["only C-1"] = out["empty"].copy(); out["only C-1"][Cn - 1] = 2
    out["every base id removed"] = np.where(base, 0, 2).astype(np.uint8)
    out["members only outside the base"] = np.where(base, 0, rng.integers(2, 256, Cn)).astype(np.uint8)
    sus = np.where(base, 2, 0).astype(np.uint8)
    if len(nb):
        sus[nb[len(nb) // 2]] = 1                        # suspect on a base id
    off = np.flatnonzero(~base)
    if len(off):
        sus[off[0]] = 1                                  # and on a non-base id
    out["suspects"] = sus
    for k in range(6):                                   # random rows: every kind of byte, dense and thin
        p = (0.02, 0.3, 0.9)[k % 3]
        r = rng.integers(1, 256, Cn).astype(np.uint8)
        r[rng.random(Cn) > p] = 0
        r[rng.random(Cn) < 0.3] &= 3                     # many 0 / 1 / 2 / 3
        out[f"random {k}"] = r
    return out


@pytest.mark.parametrize("Cn", [1, 5, 64, 131])
def test_encode_decode_identity(Cn):
    rng = np.random.default_rng(Cn)
    bases = {"empty": np.zeros(Cn, bool), "all": np.ones(Cn, bool), "prefix": np.arange(Cn) < (2 * Cn) // 3,
             "random": rng.random(Cn) < 0.5}
    for bname, base in bases.items():
        for rname, row in edge_rows(Cn, base, rng).items():
            for based in (0, 1):
                e = snapedit.encode_row(row, based, base)
                assert np.array_equal(snapedit.decode_row(e, based, base), row), (bname, rname, based)
                ids = (e >> 9).astype(np.int64)
                assert (np.diff(ids) > 0).all() and ((e & 0x1FF) != 0).all(), (bname, rname, based)
                assert not ((e & 255) == 2).any()        # ancient is never written
                if not based:
                    assert len(e) == int((row != 0).sum())   # x on every member, nothing else


def restore_rc(lib, blob: bytes) -> int:
    h = C.c_void_p()
    rc = lib.fn["sim_restore"](blob, len(blob), 0, -1, C.byref(h))
    if rc == 0:
        lib.call("sim_destroy", h)
    return rc


def have_gpu() -> bool:
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


@built
def test_validation_accepts_legal_edits(lib):
    snap = snapedit.load(golden())
    first = {r.tobytes() for r in (snapedit.logical_row(snap, i) for i in range(64))}
    for enc in ALL4:
        out = snapedit.reencode(snap, snapedit.encoding(snap, enc))
        for k in snapedit.NAMES:                         # BASED, NE and the entries change; nothing else
            if k not in ("BASED", "NE", "ENTRIES"):
                assert np.array_equal(out["sections"][k], snap["sections"][k]), (enc, k)
        assert all(np.array_equal(snapedit.logical_row(out, i), snapedit.logical_row(snap, i)) for i in range(64))
        blob = snapedit.dump(out)
        assert blob != golden()
        info = snapshot.info(blob, lib)
        assert info["entries"] == out["entries"] and info["bytes"] == len(blob) and info["round"] == 7
        rc = restore_rc(lib, blob)
        assert rc == (0 if have_gpu() else KB_NO_DEVICE), (enc, rc, lib.fn["last_error"]())
    longest = max(len(r) for r in snap["rows"])
    capped = snapedit.dump(snapedit.with_row_cap(snap, longest))
    assert snapshot.info(capped, lib)["cfg"]["sparse_row_cap"] == longest
    with pytest.raises(KbError) as e:                    # one entry fewer than the longest row holds
        snapshot.info(snapedit.dump(snapedit.with_row_cap(snap, longest - 1)), lib)
    assert e.value.code == KB_INVALID_ARGUMENT and "sparse_row_cap" in str(e.value)
    assert len(first) > 1


def corrupt_rows(snap: dict) -> dict:
    long_row = max(range(len(snap["rows"])), key=lambda i: len(snap["rows"][i]))
    assert len(snap["rows"][long_row]) >= 3
    out = {}
    s = snapedit.reencode(snap, {})
    r = s["rows"][long_row].copy(); r[[1, 2]] = r[[2, 1]]
    s["rows"][long_row] = r
    out["swapped"] = (s, "ascending")
    s = snapedit.reencode(snap, {})
    r = s["rows"][long_row].copy(); r[1] = (r[0] & ~np.uint32(0x1FF)) | (r[1] & np.uint32(0x1FF))
    s["rows"][long_row] = r
    out["repeated id"] = (s, "ascending")
    s = snapedit.reencode(snap, {})
    r = s["rows"][long_row].copy(); r[1] &= ~np.uint32(0x1FF)
    s["rows"][long_row] = r
    out["empty entry"] = (s, "neither x nor a stamp")
    s = snapedit.reencode(snap, {})
    s["sections"]["BASED"][3] = 2
    out["based 2"] = (s, "based flag")
    return out


@built
def test_rows_the_engine_never_writes_are_refused(lib):
    """ids out of order or repeated, an entry with neither x nor a stamp, a based byte above 1: each refused, with
    its own text, by kb_snapshot_info_of and kb_sim_restore alike, before a device is asked for."""
    texts = {}
    for what, (snap, word) in corrupt_rows(snapedit.load(golden())).items():
        bad = snapedit.dump(snap)                        # a well-formed file: layout and checksum are right
        seen = []
        for call in ("info", "restore"):
            with pytest.raises(KbError) as e:
                if call == "info":
                    snapshot.info(bad, lib)
                else:
                    lib.call("sim_restore", bad, len(bad), 0, -1, C.byref(C.c_void_p()))
            assert e.value.code == KB_INVALID_ARGUMENT, (what, call)
            seen.append(str(e.value).split("(", 1)[1])
        assert seen[0] == seen[1] and word in seen[0], (what, seen)
        texts[what] = seen[0]
    assert len(set(texts.values())) == 3 and texts["swapped"] == texts["repeated id"], texts


# ---- the inputs of the re-encoding tests shift rows at every position ------------------------------------------------
def test_shift_positions_are_covered():
    """Under none_based a row's entry ids are its members, so the oracle's rows() before and after a round give every
    insert and delete of the list.  Over the continued rounds of test_gpu_sparse_reencoded.py's cases: the list length
    before (mod 4) over rows that gained / lost an id, and for rows with exactly one change the index (mod 4) and
    whether the 16-byte shift of sp_ins_at / sp_del_at crosses a group (an insert at k of n entries moves groups
    k/4 .. n/4, a delete groups k/4 .. (n-1)/4).  A condition on the case list, not on the engine."""
    ins_len, del_len, ins_at, del_at = Counter(), Counter(), Counter(), Counter()
    for name, split in sorted({(n, s) for n, s, _ in CASES}):
        case, rounds = case_of(name)
        with Sim(parity.oracle_lib(), case["cfg"]) as o:
            parity.setup(o, case)
            run_to((o,), case, 0, split)
            mem = o.rows() != 0
            for r in range(split + 1, rounds):
                run_to((o,), case, r, r)
                now = o.rows() != 0
                for i in np.flatnonzero((mem != now).any(axis=1)):
                    gained, lost = np.flatnonzero(now[i] & ~mem[i]), np.flatnonzero(mem[i] & ~now[i])
                    n = int(mem[i].sum())
                    if len(gained):
                        ins_len[n & 3] += 1
                    if len(lost):
                        del_len[n & 3] += 1
                    if len(gained) + len(lost) != 1:
                        continue
                    j = int(gained[0] if len(gained) else lost[0])
                    k = int(mem[i][:j].sum())
                    if len(gained):
                        ins_at[k & 3, (n >> 2) > (k >> 2)] += 1
                    else:
                        del_at[k & 3, ((n - 1) >> 2) > (k >> 2)] += 1
                mem = now
    report = f"insert lengths {dict(ins_len)}, delete lengths {dict(del_len)}, inserts at {dict(ins_at)}, deletes at {dict(del_at)}"
    print(report)
    assert set(ins_len) == set(del_len) == {0, 1, 2, 3}, report
    want = {(k, x) for k in range(4) for x in (False, True)}
    assert set(ins_at) == want and set(del_at) == want, report
