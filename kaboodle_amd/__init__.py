"""kaboodle_amd — MI355X-native bulk-synchronous simulator of serval/kaboodle's SWIM round.

The product is the HIP library `libkaboodle_sim.so` (C ABI: include/kaboodle_sim.h).  This package is
its Python host mirror: `Mesh` owns one simulated mesh on one GPU, `Kaboodle` is a per-peer view with the
reference's method names (src/lib.rs:65-369).  There is no CPU fallback: without the built library or
a GPU every entry point raises.
"""
from __future__ import annotations

import collections
import os

from ._ffi import (KB_FAILED_SIM_SENDER, KB_FAILED_SOCKET_FAITHFUL, KB_INIT_CONVERGED, KB_INIT_JOIN,  # noqa: F401
                   KbError, Sim, SimConfig, SimLib, STATE_NAMES)

LIB_PATH = os.environ.get("KB_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libkaboodle_sim.so")
# (KB_LIB_PATH: an alternative build of the same library, for A/B timing experiments only)
_LIB = None


def lib() -> SimLib:
    """The loaded HIP library (raises if it has not been built)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"HIP library not built: {LIB_PATH} (run __graft_entry__.build())")
        # torch's wheel carries its own HIP runtime.  Loaded first, it satisfies the library's libamdhip64
        # dependency; loaded after the library, it maps a second runtime next to /opt/rocm's, and the one that
        # initialises second finds no device (kb_sim_create: "no HIP device", tools/diag/hip_load_order.py).
        import torch  # noqa: F401
        _LIB = SimLib(LIB_PATH, "kb_")
    return _LIB


def require_gpu() -> None:
    """Fail loudly when there is no GPU (the product has no CPU path)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("kaboodle_amd needs an MI355X (HIP device); none is visible")
    lib()


def rccl_unique_id() -> bytes:
    """RCCL unique id for kb_sim_create_rank (made on rank 0, broadcast by the host)."""
    from ._ffi import rccl_unique_id as _uid
    return _uid(lib())


class Mesh(Sim):
    """One simulated mesh on the GPU, or one row shard of it.

    Mesh(cfg)                              the whole mesh on this process's GPU
    Mesh(cfg, shards=k)                    k row shards inside this process (one GPU; exchange by copies)
    Mesh(cfg, rank=r, world=w, uid=u)      this process's shard of a mesh over w GPUs (RCCL exchange)
    """

    def __init__(self, cfg: SimConfig | None = None, shards: int = 0, rank: int | None = None,
                 world: int | None = None, uid: bytes | None = None, **kw):
        super().__init__(lib(), cfg or SimConfig(**kw), shards=shards, rank=rank, world=world, uid=uid)
        self._subs: dict[int, dict[str, list[Channel]]] = {}

    def node(self, i: int) -> "Kaboodle":
        return Kaboodle(self, i)

    def subscribe(self, node: int, kind: str, ch: "Channel") -> "Channel":
        """Add a discover_* channel of `node` (kind: peers | departures | fingerprints).  The first one
        attaches the device observer and drains it, so channels see only later changes, as a channel
        created on a running Kaboodle does (src/lib.rs:186-263)."""
        if node not in self._subs:
            self.watch(node)
            self.events(node)
            self._subs[node] = {"peers": [], "departures": [], "fingerprints": []}
        self._subs[node][kind].append(ch)
        return ch

    def step(self, rounds: int = 1) -> None:
        """Advance `rounds` rounds, then fan one event batch per observed node out to its channels
        (handle_known_peers_events, src/events.rs:49-123)."""
        super().step(rounds)
        for node, subs in self._subs.items():
            if not any(subs.values()):
                continue
            disc, dep, fp, changed = self.events(node)
            for x in disc:
                for c in subs["peers"]:
                    c.send((self.format_addr(x), self.identity(x)))
            for x in dep:
                for c in subs["departures"]:
                    c.send(self.format_addr(x))
            if changed:
                for c in subs["fingerprints"]:
                    c.send(fp)
            for k in subs:                        # closed channels are dropped (events.rs:29-38)
                subs[k] = [c for c in subs[k] if not c.closed]

    def save(self, path: str) -> int:
        """Write the mesh's snapshot (Sim.snapshot) to `path`; returns its length.  The bytes go to a
        temporary name in the same directory and are renamed, so a killed process never leaves half a file under
        the final name."""
        blob = self.snapshot()
        tmp = f"{path}.tmp.{os.getpid()}"
        try:
            with open(tmp, "wb") as f:
                f.write(blob)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise
        return len(blob)

    @classmethod
    def load(cls, path: str, shards: int = 0, device: int = -1) -> "Mesh":
        """A new mesh in the state `save` wrote, unsharded or as `shards` in-process row shards (any layout may
        have written the file).  Channels and observers are not carried: subscribe again."""
        with open(path, "rb") as f:
            blob = f.read()
        m = cls.restore(lib(), blob, shards=shards, device=device)
        m._subs = {}
        return m

    def fp_classes(self, top: int = 16, arrays: bool = True):
        """Which camps the views fall into (include/kaboodle_classes.h): the running rows grouped
        by equal fingerprint on the GPU.  Returns a `classes.FpClasses`: the summary (classes, largest,
        singletons, the true class's size and rank, the size histogram), the `top` largest classes as (fp, size,
        rep) and per id the representative and size of its class.  Rank shards raise KbError: a class spans ranks."""
        return super().fp_classes(top, arrays)

    def latency_census(self, arrays: bool = True):
        """The ping-latency table mesh-wide (include/kaboodle_latency.h) in one pass on the GPU: per
        peer how many observers measured it first-hand and the sum, minimum and maximum of their latencies, per row
        how many of its entries are measured, a log2 histogram of all measured values and the table's orphan
        count.  Returns a `latency.LatencyCensus`.  Needs track_latency; sparse rows and rank shards raise KbError."""
        return super().latency_census(arrays)

    def age_census(self, arrays: bool = True):
        """The stamp table mesh-wide (include/kaboodle_age.h) in one pass on the GPU: per peer how many
        observers hold it as suspect, ancient (older than the 1-byte window), windowed and fresh (stamped within
        SHARE_AGE rounds, so gossiped) and the latest instant any of them heard from it, per row the same four counts
        over its view, and a histogram of the windowed entries by age.  Returns an `age.AgeCensus`.  Sparse rows,
        unsharded or in-process shards; dense rows and rank shards raise KbError."""
        return super().age_census(arrays)

    def delta_mark(self) -> None:
        """Take (or replace) the baseline of the view-delta census (include/kaboodle_delta.h): a
        device-side copy of the member bits and the running set as they are now.  Dense rows, unsharded or
        in-process shards; sparse rows and rank shards raise KbError."""
        super().delta_mark()

    def delta_census(self, advance: bool = True, arrays: bool = True):
        """What every view gained and lost since the mark, in one pass on the GPU: per id how many continuing rows
        (running at the mark and now) gained and lost it, per row how many ids its view gained, lost, and lost
        although they still run, and the sums by kind of id (learned, ghost_adds, detections, false_drops).  Returns a
        `delta.DeltaCensus`.  advance=True makes the current state the baseline in the same pass, so one call per
        round gives per-round deltas (delta.PairTracker); advance=False reads only."""
        return super().delta_census(advance, arrays)

    def delta_release(self) -> None:
        """Free the baseline; delta_census raises KbError until the next delta_mark."""
        super().delta_release()

    def islands(self, arrays: bool = True):
        """Which peers can still reach each other (include/kaboodle_islands.h): the connected
        components of the "i holds j" graph over the running peers, labelled on the GPU with their lowest id.  Two
        islands never learn of each other again without a new joiner, a restart, ping_addrs or an external peer.
        Returns an `islands.Islands`: the summary (islands, singletons, those that broadcast Join again, the largest
        and second largest, the unreachable ordered pairs, the eight largest as (label, size)) and per id the label
        and size of its island.  Dense rows, unsharded or in-process shards; sparse rows and rank shards raise
        KbError."""
        return super().islands(arrays)

    def gaps(self, max_pairs: int = 65536) -> dict:
        """Which rows lack or still hold which ids (include/kaboodle_gaps.h): the cells the view census
        counts as `missing` and `stale`, listed on the GPU as (row, id) pairs in ascending order.  Returns the fields
        of kb_gaps and `missing_pairs` / `stale_pairs` as (n, 2) uint32 arrays; a list of more than max_pairs pairs
        is None and only counted.  Dense rows, unsharded or in-process shards; sparse rows and rank shards raise
        KbError."""
        return super().gaps(max_pairs)

    def holders(self, ids, max_rows: int | None = None):
        """Who holds these ids (include/kaboodle_gaps.h): for each of up to 1,024 ids the running rows
        whose view contains it, cut out of the member table as columns on the GPU.  Returns (offsets, rows); query q's
        holders are rows[offsets[q]:offsets[q + 1]], ascending.  Dense rows, unsharded or in-process shards; sparse
        rows and rank shards raise KbError."""
        return super().holders(ids, max_rows)


def latency_census_of(lat, member, running, arrays: bool = True, device: int = 0):
    """The latency census's GPU kernel over host arrays (kb_latency_census_of, a test surface): `lat` peer-major
    [n_ids][n_rows] uint16, `member` [n_rows][n_ids], `running` [n_rows]; a `latency.LatencyCensus`."""
    from ._ffi import latency_census_of as _of
    return _of(lib(), lat, member, running, arrays, device)


def fp_classes_of(fps, running, true_fp: int, top: int = 16, arrays: bool = True, device: int = 0):
    """The class census's GPU kernels over host arrays (kb_fp_classes_of, a test surface): `classes.FpClasses`."""
    from ._ffi import fp_classes_of as _of
    return _of(lib(), fps, running, true_fp, top, arrays, device)


def delta_of(bits_base, run_base, bits_now, run_now, external, row_lo: int = 0, rpw: int = 0, arrays: bool = True,
             device: int = 0):
    """The delta census's GPU kernel over host arrays (kb_delta_of, a test surface): member bits [rows][W/32] at the
    mark and now, the two running sets and the external ids per id; a `delta.DeltaCensus`."""
    from ._ffi import delta_of as _of
    return _of(lib(), bits_base, run_base, bits_now, run_now, external, row_lo, rpw, arrays, device)


def islands_of(bits, running, arrays: bool = True, device: int = 0):
    """The island census's GPU kernels over host arrays (kb_islands_of, a test surface): member bits
    [capacity][W/32] of every row and the running set per id; an `islands.Islands`."""
    from ._ffi import islands_of as _of
    return _of(lib(), bits, running, arrays, device)


def discover_mesh_member(mesh: "Mesh", prober=("192.0.2.1", 40000), max_rounds: int = 64):
    """Kaboodle::discover_mesh_member (src/lib.rs, src/discovery.rs:30-89) against a simulated mesh: broadcast
    Probe(prober), wait for a ProbeResponse, re-broadcast with the reference's back-off (1 s, x1.25, at most
    10 s; one protocol period = one round = 1000 ms).  Steps the mesh.  Returns (responder address,
    identity) of the first response (canonical order), or None after max_rounds."""
    interval_ms, last_ms, now_ms, waited = 1000, None, 0, 0
    for _ in range(max_rounds):
        if last_ms is None or last_ms <= now_ms - interval_ms:
            mesh.probe(prober)
            last_ms, waited = now_ms, 0
        mesh.step(1)
        now_ms += 1000
        waited += 1000
        got = [r for r in mesh.probe_responses() if r[3] == tuple(prober)]
        if got:
            return mesh.format_addr(got[0][1]), got[0][4]
        if waited >= interval_ms:                  # timeout: longer wait, then probe again (discovery.rs:62-73)
            interval_ms = min(10000, int(interval_ms * 1.25))
            waited = 0
    return None


class Channel:
    """The receiving end of a discover_* channel (tokio UnboundedReceiver / oneshot Receiver in the
    reference, src/lib.rs:186-263), filled by Mesh.step."""

    def __init__(self, oneshot: bool = False):
        self._q: collections.deque = collections.deque()
        self.oneshot, self.closed = oneshot, False

    def send(self, item) -> None:
        if self.closed:
            return
        self._q.append(item)
        if self.oneshot:
            self.closed = True

    def try_recv(self):
        """The next item, or None when nothing is pending."""
        return self._q.popleft() if self._q else None

    def drain(self) -> list:
        out = list(self._q)
        self._q.clear()
        return out

    def close(self) -> None:
        self.closed = True


class Kaboodle:
    """Per-peer view mirroring the reference `Kaboodle` struct (src/lib.rs:65-369)."""

    def __init__(self, mesh: Mesh, node: int):
        self.mesh, self.id = mesh, node
        self._identity = None                     # set while stopped: announced from the next start

    def start(self) -> None:                      # src/lib.rs:136-156 (effective next round)
        """Start, or restart after stop: the reference binds a fresh ephemeral socket on every start
        (src/kaboodle.rs:138-152) and keeps its known_peers map, so a restarted peer has a new address
        (kb_sim_restart_node); its event channels follow it."""
        old = self.id
        self.id = self.mesh.restart_node(old)
        self._identity = None
        if self.id != old and old in self.mesh._subs:
            self.mesh._subs[self.id] = self.mesh._subs.pop(old)

    def stop(self) -> None:                       # src/lib.rs:159-183
        self.mesh.stop_node(self.id)

    def is_running(self) -> bool:                 # src/lib.rs:307-309
        return self.mesh.is_running(self.id)

    def self_addr(self):                          # src/lib.rs:312-314
        return self.mesh.format_addr(self.id) if self.is_running() else None

    def ping_addrs(self, peers) -> None:          # src/lib.rs:268-297
        self.mesh.ping_addrs(self.id, list(peers))

    def set_identity(self, identity: bytes) -> None:   # src/lib.rs:323-336
        self.mesh.set_identity(self.id, identity)
        self._identity = bytes(identity)

    def fingerprint(self) -> int:                 # src/lib.rs:301-304
        return self.mesh.fingerprint(self.id)

    def peers(self) -> dict:                      # src/lib.rs:339-345: addr -> identity
        return {self.mesh.format_addr(p): self.mesh.identity(p) for p in self.mesh.peers(self.id)}

    def identity(self) -> bytes:                  # the identity this peer announces (Kaboodle.identity)
        return self._identity if self._identity is not None else self.mesh.identity(self.id)

    def discover_peers(self) -> Channel:          # src/lib.rs:221-236: (addr, identity) per new peer
        return self.mesh.subscribe(self.id, "peers", Channel())

    def discover_next_peer(self) -> Channel:      # src/lib.rs:238-263: the next one only
        return self.mesh.subscribe(self.id, "peers", Channel(oneshot=True))

    def discover_departures(self) -> Channel:     # src/lib.rs:185-199: addr per departed peer
        return self.mesh.subscribe(self.id, "departures", Channel())

    def discover_fingerprint_changes(self) -> Channel:   # src/lib.rs:201-219
        return self.mesh.subscribe(self.id, "fingerprints", Channel())

    def peer_states(self) -> dict:                # src/lib.rs:348-354: addr -> PeerInfo
        """PeerInfo per known peer (src/structs.rs:18-22): identity bytes, state name, round of its Instant
        (None = older than the stamp window), latency in simulated ms (None = never measured)."""
        out = {}
        for p, s, since, lat, ident in self.mesh.peer_states(self.id):
            out[self.mesh.format_addr(p)] = PeerInfo(ident, STATE_NAMES[s], None if since == -2**31 else since,
                                                     None if lat == 0xFFFFFFFF else lat)
        return out


class PeerInfo(collections.namedtuple("PeerInfo", "identity state since latency")):
    """PeerInfo {identity, state, latency} (src/structs.rs:18-22), the state's Instant as a round."""
