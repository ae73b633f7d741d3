"""A reader and writer of snapshot format 1 in plain Python (include/kaboodle_snapshot.h), for tests
that edit a snapshot between kb_sim_snapshot and kb_sim_restore.  numpy, zlib and the ctypes mirror of kb_config
only: no call into either library, so what it decodes is an independent reading of the bytes.

    SnHdr (144 bytes) | SnSec[24] (24 bytes each) | the sections, each on an 8-byte boundary, padding zero

A row's view is stored as one sorted list of packed entries  id << 9 | x << 8 | stamp  and one `based` byte:
`based = 1` rows are the base set with the x entries' membership inverted, `based = 0` rows are their x entries.
The flag is a choice of representation: reencode() rewrites a row under the other choice and leaves the view, and
every other table, as it was.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib

import numpy as np

from kaboodle_amd._ffi import KbConfig

MAGIC = b"KBSNAPLE"
HDR_BYTES = 24 + C.sizeof(KbConfig) + 32       # magic, versions and sizes | kb_config | round .. nsect
SEC_BYTES = 24
KB_INIT_CONVERGED = 1
ST_UNKNOWN, ST_SUSPECT, ST_ANCIENT = 0, 1, 2
NONE_ROUND = -2**31
XF = 1 << 8

# the sections in file order: name, bytes per element (sn_layout in kaboodle_amd/csrc/kb_snapshot.h)
SECTIONS = (("SCALARS", 56), ("STATS", 8), ("NE", 4), ("BASED", 1), ("N", 4), ("FP", 4), ("LAST_BCAST", 4),
            ("A3CUR", 4), ("SUSP", 16 * 8), ("CUR", 32 * 8), ("PAQ", 4 * 8), ("PAQ_N", 4), ("ALIVE", 1),
            ("START_ROUND", 4), ("IDSET", 1), ("EXT", 1), ("IDENT", 32), ("IDLEN", 1), ("PEND", 32), ("PENDLEN", 2),
            ("MOVED", 1), ("BJOIN", 16), ("BFAIL", 16), ("ENTRIES", 4))
NAMES = tuple(n for n, _ in SECTIONS)
# sections read as numbers; the others stay rows of bytes, one row per element
DTYPES = {"STATS": "<u8", "NE": "<u4", "N": "<u4", "FP": "<u4", "LAST_BCAST": "<i4", "A3CUR": "<u4", "PAQ_N": "<u4",
          "START_ROUND": "<i4", "PENDLEN": "<i2", "ENTRIES": "<u4"}
_HDR_TAIL = "<iIQQII"                          # round, alive, entries, bytes, payload_crc32, nsect


def load(blob: bytes) -> dict:
    """{"format_version", "abi_version", "cfg" (a KbConfig), "round", "alive", "entries", "bytes", "payload_crc32",
    "sections": {name: array}, "rows": [per-row entry arrays]}.  ENTRIES is split per row by NE into "rows"."""
    assert len(blob) >= HDR_BYTES + SEC_BYTES * len(SECTIONS) and blob[:8] == MAGIC, "not a snapshot"
    fv, abi, hb, cb = struct.unpack_from("<IIII", blob, 8)
    assert fv == 1 and hb == HDR_BYTES and cb == C.sizeof(KbConfig), (fv, hb, cb)
    cfg = KbConfig.from_buffer_copy(blob, 24)
    rnd, alive, entries, nbytes, crc, nsect = struct.unpack_from(_HDR_TAIL, blob, 24 + cb)
    assert nsect == len(SECTIONS) and nbytes == len(blob), (nsect, nbytes, len(blob))
    assert crc == zlib.crc32(blob[HDR_BYTES:]), "payload checksum"
    snap = {"format_version": fv, "abi_version": abi, "cfg": cfg, "round": rnd, "alive": alive, "entries": entries,
            "bytes": nbytes, "payload_crc32": crc, "sections": {}}
    for k, (name, elem) in enumerate(SECTIONS):
        sid, el, off, count = struct.unpack_from("<IIQQ", blob, HDR_BYTES + SEC_BYTES * k)
        assert (sid, el) == (k, elem) and off % 8 == 0 and off + el * count <= len(blob), (name, sid, el, off, count)
        raw = np.frombuffer(blob, np.uint8, el * count, off)
        snap["sections"][name] = (raw.view(DTYPES[name]) if name in DTYPES else raw.reshape(count, el)).copy()
    s = snap["sections"]
    s["BASED"] = s["BASED"].reshape(-1)
    ne = s["NE"]
    assert len(ne) == cfg.capacity and int(ne.sum()) == entries == len(s["ENTRIES"])
    cut = np.concatenate(([0], np.cumsum(ne, dtype=np.int64)))
    snap["rows"] = [s["ENTRIES"][cut[i]:cut[i + 1]].copy() for i in range(len(ne))]
    del s["ENTRIES"]
    return snap


def dump(snap: dict) -> bytes:
    """The snapshot's bytes: offsets recomputed (8-byte alignment, zero padding), then entries, bytes and the CRC."""
    s = dict(snap["sections"])
    s["ENTRIES"] = (np.concatenate(snap["rows"]) if len(snap["rows"]) else np.zeros(0)).astype("<u4")
    table, body = [], []
    at = HDR_BYTES + SEC_BYTES * len(SECTIONS)
    for k, (name, elem) in enumerate(SECTIONS):
        raw = np.ascontiguousarray(s[name]).view(np.uint8).reshape(-1).tobytes()
        assert len(raw) % elem == 0, name
        table.append(struct.pack("<IIQQ", k, elem, at, len(raw) // elem))
        pad = -len(raw) % 8
        body.append(raw + b"\0" * pad)
        at += len(raw) + pad
    payload = b"".join(table) + b"".join(body)
    hdr = MAGIC + struct.pack("<IIII", snap["format_version"], snap["abi_version"], HDR_BYTES, C.sizeof(KbConfig))
    hdr += bytes(snap["cfg"])
    hdr += struct.pack(_HDR_TAIL, snap["round"], snap["alive"], len(s["ENTRIES"]), HDR_BYTES + len(payload),
                       zlib.crc32(payload), len(SECTIONS))
    return hdr + payload


def base_bits(cfg) -> np.ndarray:
    """The base set as sp_create builds it (d.nb): ids < initial_nodes of a converged start, empty otherwise."""
    base = np.zeros(cfg.capacity, bool)
    if cfg.init_mode == KB_INIT_CONVERGED:
        base[: cfg.initial_nodes] = True
    return base


def decode_row(entries, based, base) -> np.ndarray:
    """read_row of kb_sparse_host.h: 0 not a member, 1 suspect, 2 ancient, above 2 an explicit Known stamp."""
    row = np.where(base, ST_ANCIENT, ST_UNKNOWN).astype(np.uint8) if based else np.zeros(len(base), np.uint8)
    for e in np.asarray(entries, np.uint32).tolist():
        j, b = e >> 9, e & 255
        mem = bool(based and base[j]) != bool(e & XF)
        row[j] = (b if b else ST_ANCIENT) if mem else ST_UNKNOWN
    return row


def logical_row(snap: dict, i: int) -> np.ndarray:
    return decode_row(snap["rows"][i], int(snap["sections"]["BASED"][i]), base_bits(snap["cfg"]))


def encode_row(row, based, base) -> np.ndarray:
    """The sorted packed entries of a view under `based`: an entry only where x or the stamp is nonzero, ancient
    stored as stamp 0."""
    row = np.asarray(row, np.uint8)
    mem = row != ST_UNKNOWN
    x = mem != (np.asarray(base, bool) if based else np.zeros(len(row), bool))
    stamp = np.where((row == ST_ANCIENT) | ~mem, 0, row).astype(np.uint32)
    ids = np.flatnonzero(x | (stamp != 0)).astype(np.uint32)
    return ((ids << 9) | (x[ids].astype(np.uint32) << 8) | stamp[ids]).astype("<u4")


def reencode(snap: dict, based_of: dict) -> dict:
    """A copy with rows {id: based} rewritten under the given flag: BASED, NE and the entries change, nothing else."""
    out = {**snap, "sections": {k: v.copy() for k, v in snap["sections"].items()}, "rows": list(snap["rows"])}
    base = base_bits(snap["cfg"])
    for i, based in based_of.items():
        e = encode_row(logical_row(snap, i), int(based), base)
        out["rows"][i] = e
        out["sections"]["BASED"][i] = int(based)
        out["sections"]["NE"][i] = len(e)
    out["entries"] = int(out["sections"]["NE"].sum())
    return out


def with_row_cap(snap: dict, cap: int) -> dict:
    cfg = KbConfig.from_buffer_copy(bytes(snap["cfg"]))
    cfg.sparse_row_cap = cap
    return {**snap, "cfg": cfg}


# ---- the encodings the re-encoding tests use --------------------------------------------------------------------
def encoding(snap: dict, name: str) -> dict:
    """{id: based} of every row the named encoding rewrites."""
    now = snap["sections"]["BASED"]
    n = len(now)
    if name == "none_based":
        return {i: 0 for i in range(n)}
    if name == "all_based":
        return {i: 1 for i in range(n)}
    if name == "flipped":
        return {i: 1 - int(now[i]) for i in range(n)}
    if name == "odd_flipped":
        return {i: 1 - int(now[i]) for i in range(1, n, 2)}
    raise KeyError(name)
