"""tests/foldref.py pinned to itself: the checkpoint-and-combine form of a fingerprint equals generate_fingerprint
computed literally (pyref.fingerprint, zlib over the concatenated bytes) and the oracle's kbo_fingerprint_of_set, at
the three segment widths tests/test_gpu_fold.py drives the kernels at, with uniform and mixed identity lengths."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import foldref
import pyref
from parity import oracle_lib

CAPS = {128: 200, 256: 8197, 384: 16390}      # SEGW: capacity (the handles of tests/test_gpu_fold.py)


def identities(cap, kind):
    if kind == "uniform0":
        return [b""] * cap
    if kind == "uniform5":
        return [pyref.default_identity(i, 5) for i in range(cap)]
    lens = (0, 1, 5, 13, 3, 32)
    return [pyref.default_identity(i, lens[(i * 7 + i // 5) % len(lens)]) for i in range(cap)]


def member_sets(cap, sw):
    rng = random.Random(cap)
    sets = {"empty": [], "full": list(range(cap))}
    for j in (0, sw - 1, sw, 32 * sw - 1, 32 * sw, cap - 1):
        if j < cap:
            sets[f"one_{j}"] = [j]
    sets["seg_edges"] = [j for j in range(cap) if j % sw in (0, sw - 1)]
    for dens in (0.01, 0.5, 0.99):
        sets[f"random_{dens}"] = [j for j in range(cap) if rng.random() < dens]
    return sets


def oracle_fp(ids, ident):
    f = oracle_lib().lib.kbo_fingerprint_of_set
    f.restype = C.c_uint32
    f.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8)]
    stride = 32
    tab = np.zeros((len(ident), stride), dtype=np.uint8)
    lens = np.array([len(b) for b in ident], dtype=np.uint8)
    for i, b in enumerate(ident):
        tab[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    arr = np.asarray(ids, dtype=np.uint32)
    return f(arr.ctypes.data_as(C.POINTER(C.c_uint32)), len(ids), tab.ctypes.data_as(C.POINTER(C.c_uint8)), stride,
             lens.ctypes.data_as(C.POINTER(C.c_uint8)))


def test_arithmetic_is_crc_concatenation():
    """x^0 is the identity, x^(8(a+b)) = x^(8a) x^(8b), and the register after a || b is the register after a
    advanced by len(b) bytes, xor the register after b: what combine() rests on."""
    rng = random.Random(5)
    one = 0x80000000
    for _ in range(50):
        a, b = rng.getrandbits(32), rng.getrandbits(32)
        assert foldref.multmodp(one, a) == a == foldref.multmodp(a, one)
        assert foldref.multmodp(a, b) == foldref.multmodp(b, a)
        assert foldref.multmodp(a, 0) == 0 == foldref.multmodp(0, a)
    assert foldref.xpow8(0) == one and foldref.xpow8(1) == 0x00800000
    for la, lb in ((0, 0), (1, 0), (0, 7), (20, 33), (3000, 1), (65536, 4097)):
        assert foldref.xpow8(la + lb) == foldref.multmodp(foldref.xpow8(la), foldref.xpow8(lb))
        x, y = rng.randbytes(la), rng.randbytes(lb)
        assert foldref.raw_crc(x + y) == foldref.multmodp(foldref.xpow8(lb), foldref.raw_crc(x)) ^ foldref.raw_crc(y)
    msg = b"123456789"
    assert foldref.raw_crc(msg) ^ foldref.multmodp(foldref.xpow8(len(msg)), foldref.MASK) ^ foldref.MASK == zlib.crc32(msg) == 0xCBF43926


@pytest.mark.parametrize("kind", ["uniform0", "uniform5", "mixed"])
@pytest.mark.parametrize("sw", sorted(CAPS))
def test_combine_of_checkpoints_is_the_fingerprint(sw, kind):
    cap = CAPS[sw]
    assert foldref.segw(cap) == sw and foldref.row_width(cap) == 64 * sw
    ident = identities(cap, kind)
    uniform = kind != "mixed"
    unit = 20 + len(ident[0]) if uniform else None
    for name, ids in member_sets(cap, sw).items():
        cps = foldref.checkpoints(ids, ident, sw, uniform)
        assert len(cps) == foldref.NSEG
        assert sum(c for _, c in cps) == (len(ids) if uniform else sum(20 + len(ident[p]) for p in ids)), name
        got = foldref.combine(cps, unit)
        assert got == pyref.fingerprint(ids, ident), f"SEGW {sw} {kind} {name}: combine {got:#x}"
        assert got == oracle_fp(ids, ident), f"SEGW {sw} {kind} {name}: oracle"
        shuffled = list(ids)
        random.Random(1).shuffle(shuffled)
        assert foldref.checkpoints(shuffled, ident, sw, uniform) == cps, name


def test_empty_segments_and_counts():
    ident = identities(200, "uniform0")
    assert foldref.checkpoint([], ident) == (0, 0)
    assert foldref.combine([(0, 0)] * 64, 20) == 0 == pyref.fingerprint([], ident)
    assert foldref.checkpoint([7], ident) == (foldref.raw_crc(pyref.addr(7).encode()), 1)
    assert foldref.checkpoint([7], ident, uniform=False)[1] == 20
