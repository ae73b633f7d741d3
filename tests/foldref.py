"""A plain reference of the fingerprint fold, zlib only.

A row's fingerprint is generate_fingerprint over its members in address order (src/kaboodle.rs:71-83): one CRC-32
over the concatenation of address || identity.  The HIP library keeps it as 64 checkpoints per row, one per segment
of SEGW = W/64 ids (W = capacity rounded up to 8192): the CRC register of the segment's bytes started from zero and
without the final xor, plus the segment's length, and combines them with GF(2) polynomial arithmetic modulo the CRC
polynomial.  This module states both from their definitions: the checkpoints through zlib.crc32, the arithmetic as
zlib's multmodp / x2nmodp in plain Python.  Nothing here is imported from the library or the oracle.
"""
from __future__ import annotations

import functools
import zlib

import pyref

MASK = 0xFFFFFFFF
POLY = 0xEDB88320                # the CRC-32 polynomial, reflected: bit 31 is x^0
NSEG = 64
POISON = (0xA5A5A5A5, 0x5A5A5A5A)   # what the tests store in a stale checkpoint


def row_width(capacity: int) -> int:
    return (capacity + 8191) // 8192 * 8192


def segw(capacity: int) -> int:
    return row_width(capacity) // NSEG


def multmodp(a: int, b: int) -> int:
    """a(x) * b(x) mod P(x), reflected representation (x^0 = 0x80000000)."""
    p = 0
    m = 1 << 31
    while a:
        if a & m:
            p ^= b
            if not a & (m - 1):
                break
        m >>= 1
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


@functools.lru_cache(maxsize=None)
def xpow8(nbytes: int) -> int:
    """x^(8 * nbytes) mod P(x) by square and multiply."""
    res, sq = 0x80000000, 0x00800000          # x^0, x^8
    while nbytes:
        if nbytes & 1:
            res = multmodp(sq, res)
        sq = multmodp(sq, sq)
        nbytes >>= 1
    return res


def seg_bytes(ids, identity) -> bytes:
    """addr(p) || identity[p] over ascending ids."""
    return b"".join(pyref.addr(p).encode() + identity[p] for p in sorted(ids))


def raw_crc(b: bytes) -> int:
    """The CRC register after b, started from zero, no final xor, in zlib's reflected representation."""
    return zlib.crc32(b, MASK) ^ MASK


def checkpoint(ids_in_segment, identity, uniform: bool = True):
    """(raw, cnt) of one segment's members; cnt = the member count, or the byte length when identities are not all
    of one length (as fold_segment documents)."""
    b = seg_bytes(ids_in_segment, identity)
    return raw_crc(b), (len(ids_in_segment) if uniform else len(b))


def checkpoints(ids, identity, seg_width: int, uniform: bool = True):
    """The 64 checkpoints of a member set."""
    per = [[] for _ in range(NSEG)]
    for p in ids:
        per[p // seg_width].append(p)
    return [checkpoint(m, identity, uniform) for m in per]


def combine(cps, unit_len: int | None = None) -> int:
    """The fingerprint of 64 checkpoints in address order: raw = raw * x^(8 len) ^ raw_k, then the init and final
    xor terms.  unit_len: bytes per member when cnt counts members (uniform identities); None: cnt is bytes."""
    raw, total = 0, 0
    for r, c in cps:
        n = c * unit_len if unit_len is not None else c
        raw = multmodp(xpow8(n), raw) ^ r
        total += n
    return raw ^ multmodp(xpow8(total), MASK) ^ MASK
