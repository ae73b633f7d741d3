"""The fingerprint fold on an MI355X against tests/foldref.py (zlib): every place that computes a checkpoint or
combines checkpoints into a fingerprint, at three row geometries, every column split, on crafted rows.

Probe tests (kb_sim_debug_fold) write rows of their own (member bits, stored checkpoints, stale
masks) and launch one path: KB_FOLD_TICK = k_fold + k_fp_rows, KB_FOLD_FP_ALL / FP_ONE = wave_fp (refold_stale's
few-stale branch up to 4 stale segments, its lane-per-segment branch above, wave_combine), KB_FOLD_THREAD = the
tick's thread-per-row refresh (thread_fp; the serial refold with non-uniform identities).  Stale checkpoints are
stored poisoned, fresh ones hold the reference value; a failure names the handle, the path, the row and the segment.

    capacity 200    W 8192   SEGW 128  one 128-id step per segment, 62 of 64 segments pure padding
    capacity 8197   W 16384  SEGW 256  segq 2; C mod 8 = 5: the last 8-id block is partly valid
    capacity 16390  W 24576  SEGW 384  segq 3: the multiply-high seg_of, a middle step with prefetch

The invariant tests run real rounds and read the checkpoints as stored (kb_sim_dump_checkpoints) after every round:
the paths a probe cannot isolate (the KnownPeers group's refold from LDS, k_proc's wave_fp with `extra`) and the
marks that broadcasts, A2, churn and restarts set.  The receive window runs after the tick, so a round ends with
marks on the rows its last handlers touched: what holds as stored is that every unmarked checkpoint
is right and an unflagged cached fingerprint is right; after kb_sim_fingerprints every flagged row is clean."""
import zlib

import numpy as np
import pytest

import foldref
import parity
import pyref
from kaboodle_amd._ffi import (KB_DBG_ALL, KB_FOLD_FP_ALL, KB_FOLD_FP_ONE, KB_FOLD_THREAD, KB_FOLD_TICK, KB_INIT_CONVERGED,
                               KB_INVALID_ARGUMENT, KB_INVALID_OPERATION, KB_VARIANT_SPARSE_ROWS, KbError, Sim, SimConfig,
                               rccl_unique_id)

pytestmark = pytest.mark.gpu

NSEG = foldref.NSEG
PATH_NAMES = {KB_FOLD_TICK: "TICK", KB_FOLD_FP_ALL: "FP_ALL", KB_FOLD_FP_ONE: "FP_ONE", KB_FOLD_THREAD: "THREAD"}
HANDLES = {"c200": (200, 0), "c8197": (8197, 0), "c16390": (16390, 0), "c8197x3": (8197, 3)}
SPLITS = (1, 2, 4, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


@pytest.fixture(scope="module")
def handles(gpu):
    """The probe handles, created on first use and kept for the module (the probe is repeatable)."""
    made = {}

    def get(name):
        if name not in made:
            cap, shards = HANDLES[name]
            made[name] = Sim(gpu, SimConfig(capacity=cap, initial_nodes=0), shards=shards)
        return made[name]

    yield get
    for s in made.values():
        s.close()


# ---- crafted rows ----------------------------------------------------------------------------------------------
def patterns(cap):
    """name -> ascending member ids"""
    sw = foldref.segw(cap)
    rng = np.random.default_rng(cap)
    p = {"empty": [], "full": list(range(cap))}
    for j in (0, sw - 1, sw, 32 * sw - 1, 32 * sw, cap - 1):
        if j < cap:
            p[f"one_{j}"] = [j]
    for dens in (0.01, 0.5, 0.99):
        p[f"random_{dens}"] = np.flatnonzero(rng.random(cap) < dens).tolist()
    p["every_byte"] = [8 * h + t for h in range((cap + 7) // 8) for t in range(8)
                       if ((37 * h + 11) % 256 >> t) & 1 and 8 * h + t < cap]
    return p


def stale_masks(cap):
    last = (cap - 1) // foldref.segw(cap)
    m = {"all": (1 << 64) - 1, "none": 0, "bit0": 1, "bit31": 1 << 31, "bit32": 1 << 32, "bit63": 1 << 63,
         "four": sum(1 << k for k in (0, 1, 32, 63)), "five": sum(1 << k for k in (0, 1, 31, 32, 63)),
         "last_id": 1 << last}
    assert bin(m["four"]).count("1") == 4 and bin(m["five"]).count("1") == 5     # refold_stale's branch is at 4 | 5
    return m


def probe_rows(cap, shards):
    """(rows, running): the ids 0, 63, 64, 255, 256, C-1; 165 alone running in its 64-row group (lane 37); 256 alone
    listed in its 256-row workgroup; two stopped rows between running ones; each shard's first and last row."""
    rows = {0, 63, 64, 255, 256, cap - 1, 165, 600, 1000, cap - 2, cap - 64} | set(range(1, 13)) | set(range(65, 71))
    if shards:
        per = (cap + shards - 1) // shards
        for k in range(shards):
            rows |= {k * per, min(cap, (k + 1) * per) - 1}
    rows = sorted(r for r in rows if 0 <= r < cap and (r == 165 or not 128 <= r < 192) and not 256 < r < 512)
    assert len(rows) <= 40 and 165 in rows
    stopped = {5, 66}
    return rows, [r not in stopped for r in rows]


class Crafted:
    """Reference values per capacity, computed once: per pattern the member bitset, the 64 checkpoints, their
    combine and the zlib fingerprint."""

    def __init__(self, cap, ident=None):
        self.cap, self.sw, self.W = cap, foldref.segw(cap), foldref.row_width(cap)
        self.ident = ident if ident is not None else [b""] * cap
        self.uniform = len({len(b) for b in self.ident}) == 1
        self.unit = 20 + len(self.ident[0]) if self.uniform else None
        self.pats = patterns(cap)
        self.bits, self.cps, self.fp = {}, {}, {}
        for name, ids in self.pats.items():
            b = np.zeros(self.W, dtype=np.uint8)
            b[ids] = 1
            self.bits[name] = np.packbits(b, bitorder="little").view(np.uint32)
            cp = foldref.checkpoints(ids, self.ident, self.sw, self.uniform)
            self.cps[name] = np.array(cp, dtype=np.uint32)
            self.fp[name] = foldref.combine(cp, self.unit)
            assert self.fp[name] == pyref.fingerprint(ids, self.ident) == zlib.crc32(foldref.seg_bytes(ids, self.ident))
        self.masks = stale_masks(cap)


_CRAFTED = {}


def crafted(cap):
    if cap not in _CRAFTED:
        _CRAFTED[cap] = Crafted(cap)
    return _CRAFTED[cap]


def layout(cr, rows, shift, offset=0, stale_kinds=None):
    """Row q of a probe call: pattern (q + offset) mod 12, stale mask (q + shift) mod 9: nine shifts give a row's
    pattern every mask; the offset moves the patterns to other rows."""
    pn, mn = list(cr.pats), stale_kinds or list(cr.masks)
    return [(pn[(q + offset) % len(pn)], mn[(q + shift) % len(mn)]) for q in range(len(rows))]


def popcount(x):
    return bin(int(x)).count("1")


def run_probe(sim, cr, tag, path, rows, running, lay, split=0, refolds_stopped=False):
    """One kb_sim_debug_fold call with stale checkpoints poisoned and fresh ones at the reference value, and the
    assertions of every listed row.  refolds_stopped: the path does not look at `alive` (k_fp_all, k_fp_one)."""
    n = len(rows)
    bits = np.stack([cr.bits[p] for p, _ in lay])
    stale = np.array([cr.masks[m] for _, m in lay], dtype=np.uint64)
    want = np.stack([cr.cps[p] for p, _ in lay])
    segp_in = want.copy()
    for q in range(n):
        for k in range(NSEG):
            if (int(stale[q]) >> k) & 1:
                segp_in[q, k] = foldref.POISON
    sout, stout, dout, fout, fbytes = sim.fold_probe(path, rows, running, bits, stale, segp_in, split=split)
    where = f"{tag} path {PATH_NAMES[path]} split {split}"
    exp_bytes = 0
    for q, i in enumerate(rows):
        pat, mk = lay[q]
        at = f"{where} row {i} (pattern {pat}, stale {mk}, {'running' if running[q] else 'stopped'})"
        if not running[q] and not refolds_stopped:
            assert np.array_equal(sout[q], segp_in[q]) and stout[q] == stale[q] and dout[q] == 1, \
                f"{at}: a stopped row was touched"
            continue
        bad = np.flatnonzero((sout[q] != want[q]).any(axis=1))
        if len(bad):
            k = int(bad[0])
            kind = "stale (refolded)" if (int(stale[q]) >> k) & 1 else "fresh (must come back as given)"
            raise AssertionError(f"{at}: segment {k}, {kind}: got ({sout[q, k, 0]:#x}, {sout[q, k, 1]}) want "
                                 f"({want[q, k, 0]:#x}, {want[q, k, 1]}); {len(bad)} segments differ")
        assert stout[q] == 0 and dout[q] == 0, f"{at}: stale_out {int(stout[q]):#x} dirty_out {dout[q]}"
        assert fout[q] == cr.fp[pat], f"{at}: fp {fout[q]:#x}, combine of the checkpoints = zlib = {cr.fp[pat]:#x}"
        if running[q]:
            exp_bytes += popcount(stale[q]) * cr.sw // 8
    if path == KB_FOLD_TICK and cr.uniform:
        assert fbytes == exp_bytes, f"{where}: fold_bytes {fbytes}, the running rows' stale segments hold {exp_bytes}"
    else:
        assert fbytes == 0, f"{where}: fold_bytes {fbytes} without k_fold"


def test_layouts_cover_every_pattern_and_mask():
    """Nine probe calls give every (bit pattern, stale mask) pair to a running row, at every capacity and offset."""
    for name, (cap, shards) in HANDLES.items():
        rows, running = probe_rows(cap, shards)
        pats, masks = patterns(cap), stale_masks(cap)
        for offset in range(len(SPLITS)):
            seen = set()
            for shift in range(9):
                pn, mn = list(pats), list(masks)
                seen |= {(pn[(q + offset) % len(pn)], mn[(q + shift) % len(mn)]) for q in range(len(rows)) if running[q]}
            assert len(seen) == len(pats) * len(masks), f"{name} offset {offset}: {len(seen)} of {len(pats) * len(masks)}"


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", list(HANDLES))
def test_probe_tick(handles, name, split):
    """k_fold at every column split, then k_fp_rows."""
    cap, shards = HANDLES[name]
    cr, sim = crafted(cap), handles(name)
    rows, running = probe_rows(cap, shards)
    for shift in range(9):
        run_probe(sim, cr, name, KB_FOLD_TICK, rows, running, layout(cr, rows, shift, SPLITS.index(split)), split=split)


@pytest.mark.parametrize("name", list(HANDLES))
def test_probe_tick_own_split(handles, name):
    cap, shards = HANDLES[name]
    cr, sim = crafted(cap), handles(name)
    rows, running = probe_rows(cap, shards)
    run_probe(sim, cr, name, KB_FOLD_TICK, rows, running, layout(cr, rows, 0), split=0)


@pytest.mark.parametrize("path", [KB_FOLD_FP_ALL, KB_FOLD_FP_ONE], ids=["fp_all", "fp_one"])
@pytest.mark.parametrize("name", list(HANDLES))
def test_probe_wave_fp(handles, name, path):
    """wave_fp: refold_stale's two branches and wave_combine.  Neither kernel looks at `alive` (a stopped peer's
    fingerprint is its frozen view's), so the stopped rows are refolded like the others."""
    cap, shards = HANDLES[name]
    cr, sim = crafted(cap), handles(name)
    rows, running = probe_rows(cap, shards)
    for shift in range(9):
        run_probe(sim, cr, name, path, rows, running, layout(cr, rows, shift, int(path == KB_FOLD_FP_ONE)), refolds_stopped=True)


@pytest.mark.parametrize("name", list(HANDLES))
def test_probe_thread(handles, name):
    """thread_fp over fresh checkpoints (uniform identities: nothing stale is allowed)."""
    cap, shards = HANDLES[name]
    cr, sim = crafted(cap), handles(name)
    rows, running = probe_rows(cap, shards)
    for shift in range(3):
        run_probe(sim, cr, name, KB_FOLD_THREAD, rows, running, layout(cr, rows, 0, 4 * shift, ["none"]))


@pytest.mark.parametrize("name", list(HANDLES))
def test_fresh_is_trusted(handles, name):
    """Only stale segments are read: a fresh checkpoint that holds another member set's value comes back unchanged
    and the fingerprint is the combine of the checkpoints as given, on every path and split."""
    cap, shards = HANDLES[name]
    cr, sim = crafted(cap), handles(name)
    ids = cr.pats["random_0.5"]
    seg0 = [j for j in ids if j < cr.sw]
    lie = foldref.checkpoint(seg0[: len(seg0) // 2], cr.ident)          # fewer members: the counts stay <= capacity
    given = [tuple(int(x) for x in c) for c in cr.cps["random_0.5"]]
    assert lie != given[0]
    given[0] = lie
    want_fp = foldref.combine(given, cr.unit)
    assert want_fp != cr.fp["random_0.5"]
    rows = [r for r in (3, 64, cap - 1) if r < cap]
    stale_mask = (1 << 1) | cr.masks["last_id"]
    runs = [(KB_FOLD_TICK, s, stale_mask) for s in SPLITS] + [(KB_FOLD_FP_ALL, 0, stale_mask), (KB_FOLD_FP_ONE, 0, stale_mask),
                                                               (KB_FOLD_FP_ALL, 0, (cr.masks["five"] | 4) & ~1),   # 5 stale
                                                               (KB_FOLD_THREAD, 0, 0)]
    for path, split, sm in runs:
        segp_in = np.array([given] * len(rows), dtype=np.uint32)
        for k in range(NSEG):
            if (sm >> k) & 1:
                segp_in[:, k] = foldref.POISON
        sout, stout, dout, fout, _ = sim.fold_probe(path, rows, [1] * len(rows), np.stack([cr.bits["random_0.5"]] * len(rows)),
                                                    [sm] * len(rows), segp_in, split=split)
        for q, i in enumerate(rows):
            at = f"{name} path {PATH_NAMES[path]} split {split} row {i}"
            assert tuple(int(x) for x in sout[q, 0]) == lie, f"{at}: the fresh checkpoint of segment 0 was rewritten"
            assert [tuple(int(x) for x in c) for c in sout[q]] == given, f"{at}: checkpoints"
            assert stout[q] == 0 and dout[q] == 0 and fout[q] == want_fp, f"{at}: fp {fout[q]:#x} want {want_fp:#x}"


# ---- non-uniform identities ---------------------------------------------------------------------------------------
NONUNIFORM_IDS = {3: b"x", 64: b"fives", 65: b"thirteen-byte", 127: b"y", 128: b"sixes", 159: b"z"}


@pytest.fixture(scope="module")
def nonuniform(gpu):
    sim = Sim(gpu, SimConfig(capacity=160, initial_nodes=0))
    ident = [b""] * 160
    for i, b in NONUNIFORM_IDS.items():
        assert len(b) in (1, 5, 13)
        sim.set_identity(i, b)
        ident[i] = b
    cr = Crafted(160, ident)
    assert not cr.uniform
    yield sim, cr
    sim.close()


NU_ROWS, NU_RUNNING = [0, 5, 63, 64, 70, 100, 128, 159], [1, 1, 1, 1, 0, 1, 1, 1]


@pytest.mark.parametrize("path", [KB_FOLD_FP_ALL, KB_FOLD_FP_ONE, KB_FOLD_THREAD], ids=["fp_all", "fp_one", "thread"])
def test_probe_nonuniform(nonuniform, path):
    """Identity lengths 0, 1, 5 and 13: checkpoints carry byte lengths; fold_segment's per-member branch (wave_fp) and
    the thread path's serial refold."""
    sim, cr = nonuniform
    for shift in range(9):
        run_probe(sim, cr, "c160 non-uniform", path, NU_ROWS, NU_RUNNING, layout(cr, NU_ROWS, shift),
                  refolds_stopped=path != KB_FOLD_THREAD)


def test_probe_nonuniform_tick_is_inert(nonuniform):
    """k_fold and k_fp_rows are for uniform identities only: the tick's two launches leave everything as it was."""
    sim, cr = nonuniform
    lay = layout(cr, NU_ROWS, 1)
    run_probe(sim, cr, "c160 non-uniform", KB_FOLD_FP_ALL, NU_ROWS, NU_RUNNING, lay, refolds_stopped=True)
    before = [sim.checkpoints(i)[3] for i in NU_ROWS]
    lay = layout(cr, NU_ROWS, 2)
    bits = np.stack([cr.bits[p] for p, _ in lay])
    stale = np.array([cr.masks[m] for _, m in lay], dtype=np.uint64)
    segp_in = np.full((len(NU_ROWS), NSEG, 2), 0x1234567, dtype=np.uint32)
    for split in (0, 1, 64):
        sout, stout, dout, fout, fbytes = sim.fold_probe(KB_FOLD_TICK, NU_ROWS, NU_RUNNING, bits, stale, segp_in, split=split)
        assert np.array_equal(sout, segp_in) and np.array_equal(stout, stale) and (dout == 1).all() and fbytes == 0
        assert list(fout) == before


# ---- refusals -------------------------------------------------------------------------------------------------------
def refused(code, fn, *a, **kw):
    with pytest.raises(KbError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


def test_refusals(gpu, handles):
    sim, cr = handles("c200"), crafted(200)
    W = cr.W
    ok = dict(rows=[0, 1], running=[1, 1], bits=np.zeros((2, W // 32), np.uint32), stale=[0, 0],
              segp_in=np.zeros((2, NSEG, 2), np.uint32))
    sim.fold_probe(KB_FOLD_TICK, **ok)
    for bad_id in (200, 223, 224, W - 1):                       # a member bit at an id >= capacity
        b = ok["bits"].copy()
        b[1, bad_id // 32] = 1 << (bad_id % 32)
        refused(KB_INVALID_ARGUMENT, sim.fold_probe, KB_FOLD_TICK, **{**ok, "bits": b})
    b = ok["bits"].copy()
    b[1, 199 // 32] = 1 << (199 % 32)                           # the last valid id is accepted
    sim.fold_probe(KB_FOLD_TICK, **{**ok, "bits": b, "stale": [0, 2]})
    refused(KB_INVALID_ARGUMENT, sim.fold_probe, KB_FOLD_TICK, **{**ok, "rows": [1, 0]})
    refused(KB_INVALID_ARGUMENT, sim.fold_probe, KB_FOLD_TICK, **{**ok, "rows": [1, 1]})
    refused(KB_INVALID_ARGUMENT, sim.fold_probe, KB_FOLD_TICK, **{**ok, "rows": [0, 200]})
    refused(KB_INVALID_ARGUMENT, sim.fold_probe, KB_FOLD_TICK, split=3, **ok)
    refused(KB_INVALID_ARGUMENT, sim.fold_probe, KB_FOLD_TICK, split=128, **ok)
    refused(KB_INVALID_ARGUMENT, sim.fold_probe, 4, **ok)
    refused(KB_INVALID_ARGUMENT, sim.fold_probe, KB_FOLD_THREAD, **{**ok, "stale": [0, 1]})
    claims = ok["segp_in"].copy()
    claims[0, :, 1] = 4                                         # fresh checkpoints that claim 256 members of 200 ids
    refused(KB_INVALID_ARGUMENT, sim.fold_probe, KB_FOLD_FP_ALL, **{**ok, "segp_in": claims})
    with Sim(gpu, SimConfig(capacity=64, initial_nodes=0)) as s:
        tiny = dict(rows=[0], running=[1], bits=np.zeros((1, 256), np.uint32), stale=[0], segp_in=np.zeros((1, NSEG, 2), np.uint32))
        s.fold_probe(KB_FOLD_FP_ALL, **tiny)
        refused(KB_INVALID_OPERATION, s.step, 1)                # no round after a probe
        s.fold_probe(KB_FOLD_TICK, **tiny)                      # but the probe again
        s.checkpoints(0)
    with Sim(gpu, SimConfig(capacity=64, initial_nodes=0), shards=2) as s:
        s.fold_probe(KB_FOLD_FP_ALL, **tiny)
        refused(KB_INVALID_OPERATION, s.step, 1)
    with Sim(gpu, SimConfig(capacity=64, initial_nodes=0)) as s:
        s.step(1)
        refused(KB_INVALID_OPERATION, s.fold_probe, KB_FOLD_FP_ALL, **tiny)       # a stepped handle
    with Sim(gpu, SimConfig(capacity=64, initial_nodes=8)) as s:
        refused(KB_INVALID_OPERATION, s.fold_probe, KB_FOLD_FP_ALL, **tiny)       # created with peers
    with Sim(gpu, SimConfig(capacity=64, initial_nodes=0, variant=KB_VARIANT_SPARSE_ROWS)) as s:
        refused(KB_INVALID_OPERATION, s.fold_probe, KB_FOLD_FP_ALL, **tiny)       # sparse rows
        refused(KB_INVALID_OPERATION, s.checkpoints, 0)
    with Sim(gpu, SimConfig(capacity=64, initial_nodes=0), rank=0, world=1, uid=rccl_unique_id(gpu)) as s:
        refused(KB_INVALID_OPERATION, s.fold_probe, KB_FOLD_FP_ALL, **tiny)       # a rank of a multi-process mesh
        refused(KB_INVALID_OPERATION, s.checkpoints, 0)


# ---- the checkpoint invariant under real rounds ------------------------------------------------------------------
POLY = np.uint32(foldref.POLY)


def multmodp_rows(a, b):
    """foldref.multmodp over uint32 arrays, element by element (the same 32 shift-and-xor steps)."""
    a, b = a.astype(np.uint32), b.astype(np.uint32).copy()
    p = np.zeros_like(b)
    for k in range(31, -1, -1):
        p ^= np.where(a & np.uint32(1 << k), b, np.uint32(0))
        b = (b >> np.uint32(1)) ^ np.where(b & np.uint32(1), POLY, np.uint32(0))
    return p


def combine_rows(cps, unit):
    """foldref.combine of many rows at once: cps uint32 [n, 64, 2]."""
    n = len(cps)
    raw, total = np.zeros(n, np.uint32), np.zeros(n, np.int64)
    xp = lambda v: np.array([foldref.xpow8(int(x)) for x in v], dtype=np.uint32)
    for k in range(NSEG):
        nb = cps[:, k, 1].astype(np.int64) * (unit if unit is not None else 1)
        if not nb.any() and not cps[:, k, 0].any():
            continue
        raw = multmodp_rows(xp(nb), raw) ^ cps[:, k, 0]
        total += nb
    return raw ^ multmodp_rows(xp(total), np.full(n, foldref.MASK, np.uint32)) ^ np.uint32(foldref.MASK)


class RowRef:
    """Reference checkpoints of the rows of a running mesh: the member ids of a row (its non-zero stamp bytes) cut at
    the segment borders, each piece's bytes through zlib.  Identities are re-read every round (set_identity)."""

    def __init__(self, sim):
        self.sim, self.cap = sim, sim.capacity
        self.sw = foldref.segw(self.cap)
        self.edges = np.arange(NSEG + 1) * self.sw
        self.refresh()

    def refresh(self):
        ident = [self.sim.identity(i) for i in range(self.cap)] if self.sim.cfg.id_len or self.cap <= 200 else [b""] * self.cap
        self.ident = ident
        self.uniform = all(len(b) == self.sim.cfg.id_len for b in ident)
        self.unit = 20 + self.sim.cfg.id_len if self.uniform else None
        self.rec = [pyref.addr(p).encode() + ident[p] for p in range(self.cap)]
        self.tab = np.frombuffer(b"".join(self.rec), np.uint8).reshape(self.cap, self.unit) if self.uniform else None

    def cps(self, ids):
        out = np.zeros((NSEG, 2), dtype=np.uint32)
        cut = np.searchsorted(ids, self.edges)
        rows = np.ascontiguousarray(self.tab[ids]) if self.uniform else None
        for k in range(NSEG):
            a, b = cut[k], cut[k + 1]
            if a == b:
                continue
            if self.uniform:
                out[k] = (foldref.raw_crc(rows[a:b]), b - a)
            else:
                bs = b"".join(self.rec[p] for p in ids[a:b])
                out[k] = (foldref.raw_crc(bs), len(bs))
        return out


def check_round(sim, ref, tag, counts):
    """The invariant as stored, then after kb_sim_fingerprints (k_fp_all)."""
    ref.refresh()
    running = np.flatnonzero(sim.scalars()[:, 0])
    want, flagged = {}, []
    got = np.zeros((len(running), NSEG, 2), np.uint32)
    cached = np.zeros(len(running), np.uint32)
    clean = np.zeros(len(running), bool)
    for q, i in enumerate(running):
        i = int(i)
        ids = np.flatnonzero(sim.row(i))
        want[i] = ref.cps(ids)
        if q == 0:                                    # the fast cut above against foldref itself
            assert [tuple(int(x) for x in c) for c in want[i]] == foldref.checkpoints(ids.tolist(), ref.ident, ref.sw, ref.uniform)
        seg, stale, dirty, fp = sim.checkpoints(i)
        bad = [k for k in np.flatnonzero((seg != want[i]).any(axis=1)) if not (stale >> int(k)) & 1]
        assert not bad, (f"{tag} row {i}: unmarked checkpoint of segment {bad[0]} is ({seg[bad[0], 0]:#x}, {seg[bad[0], 1]}), "
                         f"its members give ({want[i][bad[0], 0]:#x}, {want[i][bad[0], 1]}); stale mask {stale:#x} dirty {dirty}")
        got[q], cached[q], clean[q] = want[i], fp, not dirty
        if stale or dirty:
            flagged.append(i)
        counts["rows"] += 1
        counts["marked"] += bool(stale)
        counts["dirty"] += bool(dirty)
    fps = combine_rows(got, ref.unit)                 # of the reference checkpoints: what every cached fp must be
    if len(running):
        i0 = int(running[0])
        assert int(fps[0]) == foldref.combine([tuple(int(x) for x in c) for c in want[i0]], ref.unit) \
            == zlib.crc32(b"".join(ref.rec[p] for p in np.flatnonzero(sim.row(i0))))
    wrong = np.flatnonzero(clean & (cached != fps))
    assert not len(wrong), f"{tag} row {int(running[wrong[0]])}: cached fp {cached[wrong[0]]:#x} is not flagged stale, want {fps[wrong[0]]:#x}"
    all_fps = sim.fingerprints()                      # k_fp_all: refolds what is marked of every flagged row
    assert np.array_equal(all_fps[running], fps), f"{tag}: fingerprints differ at rows {running[all_fps[running] != fps][:4]}"
    for i in flagged:
        seg, stale, dirty, fp = sim.checkpoints(i)
        assert dirty == 0 and fp == all_fps[i], f"{tag} row {i} after fingerprints(): dirty {dirty} fp {fp:#x}"
        bad = [k for k in np.flatnonzero((seg != want[i]).any(axis=1)) if not (stale >> int(k)) & 1]
        assert not bad, f"{tag} row {i} after fingerprints(): unmarked checkpoint of segment {bad[0]} is wrong (stale mask {stale:#x})"


BY_NAME = {n: (c, r) for n, c, r in parity.standard_cases()}
BIG_8197 = ({"cfg": SimConfig(capacity=8197, initial_nodes=8000, init_mode=KB_INIT_CONVERGED, loss=0.01, churn=0.002, seed=61)}, 6)
INVARIANT = {
    "churn_loss_512": (*BY_NAME["churn_loss_512"], 0),
    "churn_loss_512_x3": (*BY_NAME["churn_loss_512"], 3),
    "config2_join_1k": (*BY_NAME["config2_join_1k"], 0),
    "config2_join_1k_dbg_all": (parity.with_cfg(BY_NAME["config2_join_1k"][0], debug_flags=KB_DBG_ALL), BY_NAME["config2_join_1k"][1], 0),
    "stop_start": (*BY_NAME["stop_start"], 0),
    "partition_heal": (*BY_NAME["partition_heal"], 0),
    "identity_change": (*BY_NAME["identity_change"], 0),
    "converged_8197": (*BIG_8197, 0),
}


@pytest.mark.parametrize("name", list(INVARIANT))
def test_checkpoint_invariant(gpu, name):
    """After every round, every running row: an unmarked checkpoint equals the reference of the row's members in that
    segment; a cached fingerprint not flagged stale equals the combine of the reference checkpoints; after
    kb_sim_fingerprints every row's cached fingerprint does, its flag is clear, and the checkpoints the refold
    stored are right.  (Marks at a round's end are by design: the receive window runs after the tick.)"""
    case, rounds, shards = INVARIANT[name]
    counts = {"rows": 0, "marked": 0, "dirty": 0}
    with Sim(gpu, case["cfg"], shards=shards) as g:
        parity.setup(g, case)
        ref = RowRef(g)
        for r in range(rounds):
            parity.apply_events((g,), case, r)
            g.step(1)
            check_round(g, ref, f"{name} round {r}", counts)
    print(f"{name}: {counts['rows']} rows checked, {counts['marked']} with stale marks and {counts['dirty']} with a stale "
          f"cached fingerprint at a round's end")
    assert counts["rows"] > 0
