"""ctypes binding of the C ABI declared in include/kaboodle_sim.h.

`SimLib(path, prefix)` binds one shared library that implements the ABI.  The product binds the
in-tree HIP library (`kaboodle_amd/libkaboodle_sim.so`, prefix ``kb_``); the test suite uses the same
class to bind the CPU oracle (prefix ``kbo_``) so both are driven through identical calls.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

KB_ABI_VERSION = 3
KB_OK, KB_INVALID_OPERATION, KB_IO_ERROR, KB_NO_DEVICE, KB_STOPPING_FAILED, KB_INVALID_ARGUMENT, KB_CAPACITY = range(7)
KB_INIT_JOIN, KB_INIT_CONVERGED = 0, 1
KB_FAILED_SIM_SENDER, KB_FAILED_SOCKET_FAITHFUL = 0, 1
KB_DBG_PHASEB_HBM, KB_DBG_RESP_HBM, KB_DBG_KP_HBM, KB_DBG_KP_BIG_SMALL, KB_DBG_PROC_UNSORTED = 1, 2, 4, 8, 16
KB_DBG_ALL = 31                  # every wide-row variant
KB_DBG_WAVE_GRAPH = 32           # the receive window as a replayed HIP graph
KB_DBG_RESP_WAVE_HBM = 64        # Join responses by wave, rows read in place (rows > 110K ids)
KB_DBG_NO_UNION = 128            # row shards: Join responses as id lists, not one union per (source shard, joiner)
KB_DBG_A3X_KPL8 = 256            # exact A3 order by the kernel of 128K-512K-id rows, at any width
KB_DBG_A3X_WIDE = 512            # exact A3 order by the one-pass kernel of rows above 512K ids, at any width
KB_DBG_WAVE0_SERIAL = 1024       # wave 0 with joiners: one KnownPeers launch, no BIG groups on the side stream
KB_DBG_RESP_SERIAL = 2048        # Join responses all before the tick, in one phase, none beside it on the third stream
KB_VARIANT_SAME_WINDOW_BCAST, KB_VARIANT_EXACT_LRU = 1, 2  # the first oracle-only; the second on the GPU too (bench default)
KB_STAT_NO_SF_FAILED_DROPS = 1
KB_VARIANT_SPARSE_ROWS = 4       # the configs[4] layout: oracle and the HIP library (unsharded or row shards)
KB_LATENCY_NONE = 0xFFFFFFFF
KT_ROWPASS, KT_ROUND, KT_FOLD, KT_RESP, KT_PROC = 0, 1, 2, 3, 4   # kb_sim_kernel_time / kb_sim_kernel_bytes kinds
KB_WAVE_SLOTS = 9
STATE_NAMES = {0: "Known", 1: "WaitingForPing", 2: "WaitingForIndirectPing"}


class KbConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("capacity", C.c_uint32), ("initial_nodes", C.c_uint32),
        ("init_mode", C.c_uint32), ("seed", C.c_uint64), ("loss_threshold", C.c_uint32),
        ("churn_threshold", C.c_uint32), ("fault_end_round", C.c_int32), ("max_waves", C.c_uint32),
        ("failed_mode", C.c_uint32), ("id_len", C.c_uint32), ("partition_groups", C.c_uint32),
        ("partition_start", C.c_int32), ("partition_end", C.c_int32), ("device", C.c_int32),
        ("debug_flags", C.c_uint32), ("track_latency", C.c_uint32), ("variant", C.c_uint32),
        ("sparse_row_cap", C.c_uint32), ("stat_flags", C.c_uint32), ("reserved", C.c_uint32 * 1),
    ]


class KbPeerState(C.Structure):
    _fields_ = [("peer", C.c_uint32), ("state", C.c_uint32), ("since", C.c_int32), ("latency_ms", C.c_uint32),
                ("identity_len", C.c_uint32), ("identity", C.c_uint8 * 32)]


PEER_STATE_DTYPE = [("peer", "<u4"), ("state", "<u4"), ("since", "<i4"), ("latency_ms", "<u4"), ("identity_len", "<u4"),
                    ("identity", "u1", (32,))]    # KbPeerState's layout (52 B, no padding)


class KbStats(C.Structure):
    _fields_ = [
        ("round", C.c_int32), ("alive", C.c_uint32), ("agree", C.c_uint32),
        ("first_converged_round", C.c_int32), ("last_converged_round", C.c_int32), ("next_free_id", C.c_uint32),
        ("sent_ping", C.c_uint64), ("sent_ping_req", C.c_uint64), ("sent_ack", C.c_uint64),
        ("sent_known_peers", C.c_uint64), ("sent_kpr", C.c_uint64),
        ("bcast_join", C.c_uint64), ("bcast_failed", C.c_uint64),
        ("drop_dead", C.c_uint64), ("drop_loss", C.c_uint64), ("drop_window", C.c_uint64),
        ("drop_oversize", C.c_uint64), ("drop_partition", C.c_uint64), ("drop_bcast", C.c_uint64),
        ("removed_timeout", C.c_uint64), ("removed_failed", C.c_uint64), ("join_responses", C.c_uint64),
        ("curious_overflow", C.c_uint64), ("churn_leaves", C.c_uint64), ("churn_joins", C.c_uint64),
        ("sent_kp_ids", C.c_uint64), ("alive_rounds", C.c_uint64), ("probe_responses", C.c_uint64),
        ("exported", C.c_uint64), ("reserved", C.c_uint64 * 4),
    ]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class KbKernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 24), ("ms", C.c_double), ("launches", C.c_uint64), ("bytes", C.c_uint64),
                ("has_bytes", C.c_uint32), ("pad", C.c_uint32), ("wave_ms", C.c_double * KB_WAVE_SLOTS)]


KB_CENSUS_NONE = 0xFFFFFFFF      # "no such id" in every census summary (the result modules import it from here)


def _summary(st: C.Structure, lists=()) -> dict:
    """A census summary struct as a dict in field order: ints, and lists of ints for the array fields in `lists`."""
    return {n: [int(x) for x in getattr(st, n)] if n in lists else int(getattr(st, n))
            for n, _ in st._fields_ if n not in ("reserved", "pad")}


def diff_results(a, b, array_names) -> list[str]:
    """What differs between two census results: the summary fields first, then each named array (None on both sides
    is equal).  A per-id array reports how many entries differ and the first; a list ([n, k] rows) or arrays of
    different lengths their lengths."""
    import numpy as np
    out = [f"summary.{k}: {v} != {b.summary[k]}" for k, v in a.summary.items() if b.summary[k] != v]
    for name in array_names:
        x, y = getattr(a, name), getattr(b, name)
        if (x is None) != (y is None):
            out.append(f"{name}: only one side has the array")
        elif x is not None and not np.array_equal(x, y):
            if x.ndim > 1 or x.shape != y.shape:
                out.append(f"{name}: {len(x)} listed != {len(y)} listed, or other entries")
            else:
                bad = np.flatnonzero(x != y)
                out.append(f"{name}: {len(bad)} differ, first id {bad[0]}: {x[bad[0]]} != {y[bad[0]]}")
    return out


_PTR = {"u4": C.POINTER(C.c_uint32), "i4": C.POINTER(C.c_int32), "u8": C.POINTER(C.c_uint64)}


def _out_arrays(arrays: bool, *groups):
    """The output arrays of a census call.  A group is ([dtype, ...], n): arrays of n entries that share one capacity
    argument.  Returns the numpy arrays, flat, and the call's arguments (each group's pointers, then its capacity);
    with arrays=False a None per array, NULL pointers and zero capacities."""
    import numpy as np
    outs, args = [], []
    for dtypes, n in groups:
        made = [np.zeros(n, dtype=dt) if arrays else None for dt in dtypes]
        outs += made
        args += [m.ctypes.data_as(_PTR[dt]) if arrays else None for m, dt in zip(made, dtypes)]
        args.append(n if arrays else 0)
    return outs, args


class KbCensus(C.Structure):
    """kb_census (include/kaboodle_census.h)."""
    _fields_ = [("round", C.c_int32), ("observers", C.c_uint32), ("running", C.c_uint32), ("exact_views", C.c_uint32),
                ("pairs", C.c_uint64), ("missing", C.c_uint64), ("stale", C.c_uint64),
                ("full_ids", C.c_uint32), ("ghost_ids", C.c_uint32), ("least_known", C.c_uint32),
                ("least_known_by", C.c_uint32), ("top_ghost", C.c_uint32), ("top_ghost_by", C.c_uint32),
                ("reserved", C.c_uint64 * 4)]

    def as_dict(self) -> dict:
        return _summary(self)


class KbReciprocity(C.Structure):
    """kb_reciprocity (include/kaboodle_reciprocity.h)."""
    _fields_ = [("round", C.c_int32), ("observers", C.c_uint32), ("mutual_pairs", C.c_uint64),
                ("oneway_pairs", C.c_uint64), ("rows_mutual", C.c_uint32), ("rows_oneway", C.c_uint32),
                ("max_mutual_row", C.c_uint32), ("max_mutual", C.c_uint32), ("pairs_listed", C.c_uint64),
                ("reserved", C.c_uint64 * 4)]

    def as_dict(self) -> dict:
        return _summary(self)


class KbFpClass(C.Structure):
    """kb_fp_class (include/kaboodle_classes.h)."""
    _fields_ = [("fp", C.c_uint32), ("size", C.c_uint32), ("rep", C.c_uint32), ("pad", C.c_uint32)]


class KbFpClasses(C.Structure):
    """kb_fp_classes (include/kaboodle_classes.h)."""
    _fields_ = [("round", C.c_int32), ("observers", C.c_uint32), ("classes", C.c_uint32), ("largest", C.c_uint32),
                ("singletons", C.c_uint32), ("true_fp", C.c_uint32), ("true_size", C.c_uint32),
                ("true_rank", C.c_uint32), ("size_hist", C.c_uint32 * 32), ("listed", C.c_uint32),
                ("listed_observers", C.c_uint32), ("reserved", C.c_uint64 * 4)]

    def as_dict(self) -> dict:
        d = _summary(self, ("size_hist",))
        d["size_hist"] = d.pop("size_hist")              # after listed and listed_observers
        return d


KB_FPC_LIST_MAX = 1024
_FPC_OUT = [C.POINTER(KbFpClasses), C.POINTER(KbFpClass), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32),
            C.POINTER(C.c_uint32), C.c_size_t]


class KbLatCensus(C.Structure):
    """kb_lat_census (include/kaboodle_latency.h)."""
    _fields_ = [("round", C.c_int32), ("observers", C.c_uint32), ("measured", C.c_uint64), ("sum_ms", C.c_uint64),
                ("min_ms", C.c_uint32), ("max_ms", C.c_uint32), ("max_peer", C.c_uint32), ("measured_ids", C.c_uint32),
                ("hist", C.c_uint64 * 17), ("orphans", C.c_uint64), ("reserved", C.c_uint64 * 4)]

    def as_dict(self) -> dict:
        return _summary(self, ("hist",))


_LATC_OUT = [C.POINTER(KbLatCensus), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
             C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_size_t]


class KbAgeCensus(C.Structure):
    """kb_age_census (include/kaboodle_age.h)."""
    _fields_ = [("round", C.c_int32), ("observers", C.c_uint32), ("cells", C.c_uint64), ("suspects", C.c_uint64),
                ("ancient", C.c_uint64), ("windowed", C.c_uint64), ("fresh", C.c_uint64), ("dead_suspects", C.c_uint64),
                ("dead_ancient", C.c_uint64), ("dead_windowed", C.c_uint64), ("dead_fresh", C.c_uint64),
                ("unheard_ids", C.c_uint32), ("oldest_heard_id", C.c_uint32), ("oldest_heard", C.c_int32),
                ("pad", C.c_uint32), ("hist", C.c_uint64 * 256), ("reserved", C.c_uint64 * 4)]

    def as_dict(self) -> dict:
        return _summary(self, ("hist",))


_AGEC_OUT = [C.POINTER(KbAgeCensus), *[C.POINTER(C.c_uint32)] * 4, C.POINTER(C.c_int32), C.c_size_t,
             *[C.POINTER(C.c_uint32)] * 4, C.c_size_t]


KB_DELTA_ADVANCE = 1             # kb_sim_delta_census flags


class KbDelta(C.Structure):
    """kb_delta (include/kaboodle_delta.h)."""
    _fields_ = [("round_base", C.c_int32), ("round", C.c_int32), ("continuing", C.c_uint32), ("new_rows", C.c_uint32),
                ("ended_rows", C.c_uint32), ("changed_rows", C.c_uint32), ("changed_ids", C.c_uint32),
                ("top_false_drop", C.c_uint32), ("top_false_drop_by", C.c_uint32), ("pad", C.c_uint32),
                ("learned", C.c_uint64), ("ghost_adds", C.c_uint64), ("detections", C.c_uint64),
                ("false_drops", C.c_uint64), ("ext_gained", C.c_uint64), ("ext_lost", C.c_uint64),
                ("reserved", C.c_uint64 * 4)]

    def as_dict(self) -> dict:
        return _summary(self)


_DELTA_OUT = [C.POINTER(KbDelta), *[C.POINTER(C.c_uint32)] * 2, C.c_size_t, *[C.POINTER(C.c_uint32)] * 3, C.c_size_t]


KB_ISLANDS_TOP = 8               # islands listed in kb_islands.top


class KbIslands(C.Structure):
    """kb_islands (include/kaboodle_islands.h)."""
    _fields_ = [("round", C.c_int32), ("observers", C.c_uint32), ("islands", C.c_uint32), ("singletons", C.c_uint32),
                ("rebroadcasting", C.c_uint32), ("largest", C.c_uint32), ("largest_label", C.c_uint32),
                ("second", C.c_uint32), ("unreachable_pairs", C.c_uint64), ("top", C.c_uint32 * 2 * KB_ISLANDS_TOP),
                ("sweeps", C.c_uint32), ("pad", C.c_uint32), ("reserved", C.c_uint64 * 4)]

    def as_dict(self) -> dict:
        top = [[int(e[0]), int(e[1])] for e in self.top]
        return {n: top if n == "top" else int(getattr(self, n)) for n, _ in self._fields_ if n not in ("reserved", "pad")}


_ISLANDS_OUT = [C.POINTER(KbIslands), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t]


KB_HOLDERS_MAX = 1024            # ids one kb_sim_holders call answers


class KbGaps(C.Structure):
    """kb_gaps (include/kaboodle_gaps.h)."""
    _fields_ = [("round", C.c_int32), ("observers", C.c_uint32), ("missing", C.c_uint64), ("stale", C.c_uint64),
                ("missing_listed", C.c_uint64), ("stale_listed", C.c_uint64), ("rows_missing", C.c_uint32),
                ("rows_stale", C.c_uint32), ("reserved", C.c_uint64 * 4)]

    def as_dict(self) -> dict:
        return _summary(self)


KB_SNAPSHOT_VERSION = 1


class KbSnapshotInfo(C.Structure):
    """kb_snapshot_info (include/kaboodle_snapshot.h)."""
    _fields_ = [("format_version", C.c_uint32), ("abi_version", C.c_uint32), ("cfg", KbConfig), ("round", C.c_int32),
                ("alive", C.c_uint32), ("entries", C.c_uint64), ("bytes", C.c_uint64), ("payload_crc32", C.c_uint32),
                ("reserved", C.c_uint32 * 7)]

    def as_dict(self) -> dict:
        d = {n: int(getattr(self, n)) for n, _ in self._fields_ if n not in ("reserved", "cfg")}
        d["cfg"] = {n: int(getattr(self.cfg, n)) for n, _ in KbConfig._fields_ if n != "reserved"}
        return d


KB_FOLD_TICK, KB_FOLD_FP_ALL, KB_FOLD_FP_ONE, KB_FOLD_THREAD = 0, 1, 2, 3   # kb_fold_probe.path
NSEG = 64                        # fingerprint checkpoints per row


class KbFoldProbe(C.Structure):
    """kb_fold_probe (include/kaboodle_sim.h)."""
    _fields_ = [("path", C.c_uint32), ("split", C.c_uint32), ("nrows", C.c_uint32), ("pad", C.c_uint32),
                ("rows", C.POINTER(C.c_uint32)), ("running", C.POINTER(C.c_uint8)), ("bits", C.POINTER(C.c_uint32)),
                ("stale", C.POINTER(C.c_uint64)), ("segp_in", C.POINTER(C.c_uint32)),
                ("segp_out", C.POINTER(C.c_uint32)), ("stale_out", C.POINTER(C.c_uint64)),
                ("dirty_out", C.POINTER(C.c_uint32)), ("fp_out", C.POINTER(C.c_uint32)),
                ("fold_bytes", C.POINTER(C.c_uint64))]


class KbWireAddrC(C.Structure):
    _fields_ = [("ip", C.c_uint8 * 4), ("port", C.c_uint16), ("pad", C.c_uint16)]


class KbProbeResponse(C.Structure):
    _fields_ = [("responder", C.c_uint32), ("probe", C.c_uint32), ("round", C.c_int32), ("prober", KbWireAddrC),
                ("identity_len", C.c_uint32), ("identity", C.c_uint8 * 32)]


class KbUnicast(C.Structure):
    _fields_ = [("round", C.c_int32), ("wave", C.c_uint32), ("sender", C.c_uint32), ("dest", C.c_uint32),
                ("seq", C.c_uint32), ("kind", C.c_uint32), ("a", C.c_uint32), ("fp", C.c_uint32), ("n", C.c_uint32),
                ("pay_off", C.c_uint32), ("pay_len", C.c_uint32), ("pad", C.c_uint32)]


class KbBroadcast(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("sender", C.c_uint32), ("peer", C.c_uint32), ("pad", C.c_uint32)]


def wire_addr(addr) -> KbWireAddrC:
    """("a.b.c.d", port) -> kb_wire_addr"""
    ip, port = addr
    a = KbWireAddrC()
    for k, part in enumerate(ip.split(".")):
        a.ip[k] = int(part)
    a.port = port
    return a


class KbError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what} failed with status {code}")
        self.code = code


@dataclass
class SimConfig:
    """Python-side mirror of kb_config (defaults as kb_config_default)."""
    capacity: int = 1024
    initial_nodes: int = 1024
    init_mode: int = KB_INIT_JOIN
    seed: int = 1
    loss: float = 0.0            # per-delivery loss probability
    churn: float = 0.0           # per-node per-round leave probability
    fault_end_round: int = -1
    max_waves: int = 8
    failed_mode: int = KB_FAILED_SIM_SENDER
    id_len: int = 0
    partition_groups: int = 0
    partition_start: int = 0
    partition_end: int = 0
    device: int = -1
    debug_flags: int = 0         # KB_DBG_*: force the wide-row kernel variants (test surface)
    track_latency: int = 0       # 1: keep the ping-latency EWMA reported by peer_states
    variant: int = 0             # KB_VARIANT_*: SAME_WINDOW_BCAST (oracle-only deviation measurement), EXACT_LRU
                                 # (the reference's exact A3 order, oracle and GPU), SPARSE_ROWS (the configs[4]
                                 # layout, oracle and GPU, unsharded or as row shards)
    sparse_row_cap: int = 0      # KB_VARIANT_SPARSE_ROWS on the GPU: entries per row (0: min(capacity, 4096))
    stat_flags: int = 0          # KB_STAT_*: KB_STAT_NO_SF_FAILED_DROPS skips socket_faithful Failed drop counts

    def to_c(self) -> KbConfig:
        c = KbConfig()
        c.abi_version = KB_ABI_VERSION
        c.capacity, c.initial_nodes, c.init_mode = self.capacity, self.initial_nodes, self.init_mode
        c.seed = self.seed
        c.loss_threshold = min(int(round(self.loss * 2**32)), 2**32 - 1)
        c.churn_threshold = min(int(round(self.churn * 2**32)), 2**32 - 1)
        c.fault_end_round, c.max_waves, c.failed_mode = self.fault_end_round, self.max_waves, self.failed_mode
        c.id_len = self.id_len
        c.partition_groups, c.partition_start, c.partition_end = (
            self.partition_groups, self.partition_start, self.partition_end)
        c.device = self.device
        c.debug_flags, c.track_latency, c.variant = self.debug_flags, self.track_latency, self.variant
        c.sparse_row_cap, c.stat_flags = self.sparse_row_cap, self.stat_flags
        return c

    @classmethod
    def from_c(cls, c: KbConfig) -> "SimConfig":
        """The mirror of a kb_config (a snapshot's): to_c() of the result gives the same thresholds back."""
        return cls(capacity=c.capacity, initial_nodes=c.initial_nodes, init_mode=c.init_mode, seed=c.seed,
                   loss=c.loss_threshold / 2**32, churn=c.churn_threshold / 2**32, fault_end_round=c.fault_end_round,
                   max_waves=c.max_waves, failed_mode=c.failed_mode, id_len=c.id_len, partition_groups=c.partition_groups,
                   partition_start=c.partition_start, partition_end=c.partition_end, device=c.device,
                   debug_flags=c.debug_flags, track_latency=c.track_latency, variant=c.variant,
                   sparse_row_cap=c.sparse_row_cap, stat_flags=c.stat_flags)


_SIGS = {
    "sim_create": (C.c_int, [C.POINTER(KbConfig), C.POINTER(C.c_void_p)]),
    "sim_destroy": (C.c_int, [C.c_void_p]),
    "sim_step": (C.c_int, [C.c_void_p, C.c_uint32]),
    "sim_start_node": (C.c_int, [C.c_void_p, C.c_uint32]),
    "sim_stop_node": (C.c_int, [C.c_void_p, C.c_uint32]),
    "sim_is_running": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]),
    "sim_ping_addrs": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_size_t]),
    "sim_set_identity": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]),
    "sim_identity": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "sim_fingerprint": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "sim_fingerprints": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t]),
    "sim_true_fingerprint": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "sim_peers": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "sim_peer_states": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(KbPeerState), C.c_size_t,
                                  C.POINTER(C.c_size_t)]),
    "sim_stats": (C.c_int, [C.c_void_p, C.POINTER(KbStats)]),
    "sim_dump_row": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint8), C.c_size_t]),
    "sim_dump_scalars": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_size_t]),
    "sim_dump_suspects": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), C.c_size_t,
                                    C.POINTER(C.c_size_t)]),
    "sim_dump_curious": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), C.c_size_t,
                                   C.POINTER(C.c_size_t)]),
    "sim_watch": (C.c_int, [C.c_void_p, C.c_uint32]),
    "sim_events": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t),
                             C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32),
                             C.POINTER(C.c_int)]),
    "sim_probe": (C.c_int, [C.c_void_p, C.POINTER(KbWireAddrC)]),
    "sim_probe_responses": (C.c_int, [C.c_void_p, C.POINTER(KbProbeResponse), C.c_size_t, C.POINTER(C.c_size_t)]),
    "sim_broadcasts": (C.c_int, [C.c_void_p, C.POINTER(KbBroadcast), C.c_size_t, C.POINTER(C.c_size_t)]),
    "sim_set_external": (C.c_int, [C.c_void_p, C.c_uint32]),
    "sim_inject": (C.c_int, [C.c_void_p, C.POINTER(KbUnicast), C.POINTER(C.c_uint32)]),
    "sim_exported": (C.c_int, [C.c_void_p, C.POINTER(KbUnicast), C.c_size_t, C.POINTER(C.c_size_t),
                               C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "format_addr": (C.c_int, [C.c_uint32, C.c_char_p, C.c_size_t]),
    "last_error": (C.c_char_p, []),
}
_OPTIONAL = {
    "sim_restart_node": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    # sharding (HIP library only; the oracle is the unsharded mesh every shard layout must reproduce)
    "rccl_unique_id": (C.c_int, [C.POINTER(C.c_uint8), C.c_size_t]),
    "ipc_unique_id": (C.c_int, [C.POINTER(C.c_uint8), C.c_size_t]),
    "sim_create_rank": (C.c_int, [C.POINTER(KbConfig), C.c_int32, C.c_int32, C.POINTER(C.c_uint8),
                                  C.POINTER(C.c_void_p)]),
    "sim_create_local": (C.c_int, [C.POINTER(KbConfig), C.c_int32, C.POINTER(C.c_void_p)]),
    "sim_shard_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint32)]),
    "sim_kernel_time": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "sim_reset_kernel_time": (C.c_int, [C.c_void_p]),
    "sim_kernel_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "sim_debug_paths": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "sim_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "sim_kernel_breakdown": (C.c_int, [C.c_void_p, C.POINTER(KbKernelTime), C.c_size_t, C.POINTER(C.c_size_t)]),
    "sim_host_syncs": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "sim_sparse_footprint": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]),
    # the fingerprint checkpoints as stored and the fold probe (test surface; HIP library only)
    "sim_dump_checkpoints": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "sim_debug_fold": (C.c_int, [C.c_void_p, C.POINTER(KbFoldProbe)]),
    # the view census (include/kaboodle_census.h; HIP library only, the oracle answers through census.census_ref)
    "sim_census": (C.c_int, [C.c_void_p, C.POINTER(KbCensus), C.POINTER(C.c_uint32), C.c_size_t,
                             C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t]),
    "sim_census_device_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    # the reciprocity census (include/kaboodle_reciprocity.h; HIP library only, the oracle answers through
    # reciprocity.reciprocity_ref)
    "sim_reciprocity": (C.c_int, [C.c_void_p, C.POINTER(KbReciprocity), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t]),
    "sim_reciprocity_device_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    # the fingerprint-class census (include/kaboodle_classes.h; HIP library only, the oracle answers through
    # classes.fp_classes_ref)
    "sim_fp_classes": (C.c_int, [C.c_void_p, *_FPC_OUT]),
    "sim_fp_classes_device_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fp_classes_of": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_size_t, C.c_uint32, *_FPC_OUT]),
    # the latency census (include/kaboodle_latency.h; HIP library only, the oracle answers through
    # latency.latency_census_ref)
    "sim_latency_census": (C.c_int, [C.c_void_p, *_LATC_OUT]),
    "sim_latency_census_device_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "latency_census_of": (C.c_int, [C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_size_t,
                                    C.c_size_t, *_LATC_OUT]),
    # the contact-age census (include/kaboodle_age.h; HIP library only, the oracle answers through age.age_census_ref)
    "sim_age_census": (C.c_int, [C.c_void_p, *_AGEC_OUT]),
    "sim_age_census_device_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    # the view-delta census (include/kaboodle_delta.h; HIP library only, the oracle answers through delta.delta_ref)
    "sim_delta_mark": (C.c_int, [C.c_void_p]),
    "sim_delta_census": (C.c_int, [C.c_void_p, *_DELTA_OUT, C.c_uint32]),
    "sim_delta_release": (C.c_int, [C.c_void_p]),
    "sim_delta_device_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "delta_of": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32),
                           C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32,
                           *_DELTA_OUT]),
    # the island census (include/kaboodle_islands.h; HIP library only, the oracle answers through
    # islands.islands_of_sim)
    "sim_islands": (C.c_int, [C.c_void_p, *_ISLANDS_OUT]),
    "sim_islands_device_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "islands_of": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_size_t, *_ISLANDS_OUT]),
    # the gap list and the holders query (include/kaboodle_gaps.h; HIP library only, the oracle answers through
    # gaps.gaps_of_sim / gaps.holders_of_sim)
    "sim_gaps": (C.c_int, [C.c_void_p, C.POINTER(KbGaps), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32),
                           C.c_size_t]),
    "sim_gaps_device_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "sim_holders": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                              C.c_size_t, C.POINTER(C.c_uint64)]),
    "sim_holders_device_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    # snapshot and restore (include/kaboodle_snapshot.h; HIP library only)
    "snapshot_info_of": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(KbSnapshotInfo)]),
    "sim_snapshot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "sim_restore": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "sim_snapshot_device_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
}


class SimLib:
    """One loaded implementation of the ABI (functions named `<prefix><name>`)."""

    def __init__(self, path: str, prefix: str = "kb_"):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.path, self.prefix = path, prefix
        self.lib = C.CDLL(path)
        self.fn = {}
        for name, (res, args) in _SIGS.items():
            f = getattr(self.lib, prefix + name)
            f.restype, f.argtypes = res, args
            self.fn[name] = f
        for name, (res, args) in _OPTIONAL.items():
            f = getattr(self.lib, prefix + name, None)
            if f is not None:
                f.restype, f.argtypes = res, args
                self.fn[name] = f

    def call(self, name: str, *args) -> None:
        rc = self.fn[name](*args)
        if rc != KB_OK:
            err = self.fn["last_error"]()
            raise KbError(rc, f"{self.prefix}{name} ({err.decode(errors='replace') if err else ''})")


KB_UNIQUE_ID_BYTES = 128


def rccl_unique_id(lib: SimLib) -> bytes:
    """A fresh RCCL unique id (rank 0 makes it; the host broadcasts it to the other ranks)."""
    buf = (C.c_uint8 * KB_UNIQUE_ID_BYTES)()
    lib.call("rccl_unique_id", buf, KB_UNIQUE_ID_BYTES)
    return bytes(buf)


def ipc_unique_id(lib: SimLib) -> bytes:
    """A unique id for ranks in separate processes sharing one device (the IPC test transport)."""
    buf = (C.c_uint8 * KB_UNIQUE_ID_BYTES)()
    lib.call("ipc_unique_id", buf, KB_UNIQUE_ID_BYTES)
    return bytes(buf)


def _fp_classes_call(lib: SimLib, name: str, head: tuple, top: int, arrays: bool, n: int):
    """kb_sim_fp_classes / kb_fp_classes_of with the outputs of Sim.fp_classes: a list of `top` entries and, with
    arrays, rep and size over `n` rows."""
    import numpy as np
    from .classes import FpClasses
    out, got = KbFpClasses(), C.c_size_t(0)
    lst = (KbFpClass * max(top, 1))()
    outs, args = _out_arrays(arrays, (["u4", "u4"], n))
    lib.call(name, *head, C.byref(out), lst if top else None, top, C.byref(got), *args)
    cls = np.array([(e.fp, e.size, e.rep) for e in lst[: got.value]], dtype=np.uint32).reshape(-1, 3)
    return FpClasses(out.as_dict(), cls, *outs)


def fp_classes_of(lib: SimLib, fps, running, true_fp: int, top: int = 16, arrays: bool = True, device: int = 0):
    """kb_fp_classes_of: the class census's kernels over host arrays of fingerprints and running flags (a test
    surface, include/kaboodle_classes.h); an `FpClasses` with round -1.  KbError(KB_NO_DEVICE) without a GPU."""
    import numpy as np
    fps = np.ascontiguousarray(fps, dtype=np.uint32)
    run = np.ascontiguousarray(np.asarray(running) != 0, dtype=np.uint8)
    if len(fps) != len(run):
        raise ValueError("fps and running differ in length")
    head = (device, fps.ctypes.data_as(C.POINTER(C.c_uint32)), run.ctypes.data_as(C.POINTER(C.c_uint8)), len(fps),
            int(true_fp) & 0xFFFFFFFF)
    return _fp_classes_call(lib, "fp_classes_of", head, top, arrays, len(fps))


def _latency_census_call(lib: SimLib, name: str, head: tuple, arrays: bool, n_ids: int, n_rows: int):
    """kb_sim_latency_census / kb_latency_census_of with the outputs of Sim.latency_census: with arrays, the four
    arrays over `n_ids` ids and the two over `n_rows` rows."""
    from .latency import LatencyCensus
    out = KbLatCensus()
    outs, args = _out_arrays(arrays, (["u4", "u8", "u4", "u4"], n_ids), (["u4", "u8"], n_rows))
    lib.call(name, *head, C.byref(out), *args)
    return LatencyCensus(out.as_dict(), *outs)


def latency_census_of(lib: SimLib, lat, member, running, arrays: bool = True, device: int = 0):
    """kb_latency_census_of: the latency census's kernel over host arrays (a test surface,
    include/kaboodle_latency.h): `lat` peer-major [n_ids][n_rows] uint16 (0xFFFF = None), `member` [n_rows][n_ids],
    `running` [n_rows]; a `LatencyCensus` with round -1.  KbError(KB_NO_DEVICE) without a GPU."""
    import numpy as np
    lat = np.ascontiguousarray(lat, dtype=np.uint16)
    n_ids, n_rows = lat.shape
    mem = np.ascontiguousarray(np.asarray(member).reshape(n_rows, n_ids) != 0, dtype=np.uint8)
    run = np.ascontiguousarray(np.asarray(running).reshape(n_rows) != 0, dtype=np.uint8)
    p8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    head = (device, lat.ctypes.data_as(C.POINTER(C.c_uint16)), p8(mem), p8(run), n_ids, n_rows)
    return _latency_census_call(lib, "latency_census_of", head, arrays, n_ids, n_rows)


def _age_census_call(lib: SimLib, name: str, head: tuple, arrays: bool, n_ids: int, n_rows: int):
    """kb_sim_age_census with the outputs of Sim.age_census: with arrays, the five arrays over
    `n_ids` ids and the four over `n_rows` rows."""
    from .age import AgeCensus
    out = KbAgeCensus()
    outs, args = _out_arrays(arrays, (["u4"] * 4 + ["i4"], n_ids), (["u4"] * 4, n_rows))
    lib.call(name, *head, C.byref(out), *args)
    return AgeCensus(out.as_dict(), *outs)


def delta_of(lib: SimLib, bits_base, run_base, bits_now, run_now, external, row_lo: int = 0, rpw: int = 0,
             arrays: bool = True, device: int = 0):
    """kb_delta_of: the delta census's kernel over host arrays (a test surface, include/kaboodle_delta.h).  bits_base /
    bits_now: uint32 [rows, W/32] member bits of the ids row_lo onwards (W = capacity rounded up to 8192); run_base /
    run_now / external: a flag per id ([capacity]); rpw: rows per wave (0: the default).  A `DeltaCensus` with rounds
    -1.  KbError(KB_NO_DEVICE) without a GPU."""
    import numpy as np
    from .delta import DeltaCensus
    rb, rn, ex = (np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8) for a in (run_base, run_now, external))
    cap = len(rn)
    b0, b1 = (np.ascontiguousarray(a, dtype=np.uint32) for a in (bits_base, bits_now))
    nwr = (cap + 8191) // 8192 * 8192 // 32
    if len(rb) != cap or len(ex) != cap or b0.shape != b1.shape or b0.ndim != 2 or b0.shape[1] != nwr:
        raise ValueError("delta_of: array shapes do not match the capacity")
    p8, p32 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)))
    out = KbDelta()
    outs, args = _out_arrays(arrays, (["u4"] * 2, cap), (["u4"] * 3, cap))
    lib.call("delta_of", device, p32(b0), p8(rb), p32(b1), p8(rn), p8(ex), cap, row_lo, b0.shape[0], rpw,
             C.byref(out), *args)
    return DeltaCensus(out.as_dict(), *outs)


def islands_of(lib: SimLib, bits, running, arrays: bool = True, device: int = 0):
    """kb_islands_of: the island census's kernels over host arrays (a test surface, include/kaboodle_islands.h).  bits:
    uint32 [capacity, W/32] member bits of every row (W = capacity rounded up to 8192); running: a flag per id
    ([capacity]).  An `Islands` with round -1.  KbError(KB_NO_DEVICE) without a GPU."""
    import numpy as np
    from .islands import Islands
    run = np.ascontiguousarray(np.asarray(running) != 0, dtype=np.uint8)
    cap = len(run)
    b = np.ascontiguousarray(bits, dtype=np.uint32)
    if b.ndim != 2 or b.shape != (cap, (cap + 8191) // 8192 * 8192 // 32):
        raise ValueError("islands_of: array shapes do not match the capacity")
    out = KbIslands()
    outs, args = _out_arrays(arrays, (["u4"] * 2, cap))
    lib.call("islands_of", device, b.ctypes.data_as(C.POINTER(C.c_uint32)), run.ctypes.data_as(C.POINTER(C.c_uint8)),
             cap, C.byref(out), *args)
    return Islands(out.as_dict(), *outs)


class Sim:
    """A simulated mesh (one handle) bound to a SimLib.

    shards=k (k >= 1): the mesh split into k row shards inside this process (kb_sim_create_local);
    rank/world/uid: this process's shard of a mesh spread over `world` processes (kb_sim_create_rank).
    A library without the sharding entry points (the oracle) always builds the unsharded mesh, which
    every shard layout must reproduce bit for bit.
    """

    def __init__(self, lib: SimLib, cfg: SimConfig, shards: int = 0, rank: int | None = None,
                 world: int | None = None, uid: bytes | None = None):
        self.lib, self.cfg = lib, cfg
        self._c = cfg.to_c()
        h = C.c_void_p()
        if world is not None and "sim_create_rank" in lib.fn:
            ub = (C.c_uint8 * KB_UNIQUE_ID_BYTES).from_buffer_copy(uid)
            lib.call("sim_create_rank", C.byref(self._c), rank, world, ub, C.byref(h))
        elif shards and "sim_create_local" in lib.fn:
            lib.call("sim_create_local", C.byref(self._c), shards, C.byref(h))
        else:
            lib.call("sim_create", C.byref(self._c), C.byref(h))
        self.h = h
        self.capacity = cfg.capacity
        self.external: set[int] = set()      # ids marked by set_external (census_ref needs them on the oracle)
        self._delta_base = None              # the host baseline of a library without kb_sim_delta_mark (the oracle)

    def shard_info(self):
        """(rank, world, lo, hi): the rows this handle holds."""
        if "sim_shard_info" not in self.lib.fn:
            return 0, 1, 0, self.capacity
        r, w, lo, hi = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32()
        self.lib.call("sim_shard_info", self.h, C.byref(r), C.byref(w), C.byref(lo), C.byref(hi))
        return r.value, w.value, lo.value, hi.value

    def close(self) -> None:
        if self.h:
            self.lib.call("sim_destroy", self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- lifecycle --
    def step(self, rounds: int = 1) -> None:
        self.lib.call("sim_step", self.h, rounds)

    def start_node(self, node: int) -> None:
        self.lib.call("sim_start_node", self.h, node)

    def stop_node(self, node: int) -> None:
        self.lib.call("sim_stop_node", self.h, node)

    def restart_node(self, node: int) -> int:
        """Kaboodle::start for the instance at `node`: returns its address from then on (a fresh id when it
        had run and is stopped; kb_sim_restart_node)."""
        v = C.c_uint32()
        self.lib.call("sim_restart_node", self.h, node, C.byref(v))
        return v.value

    def is_running(self, node: int) -> bool:
        v = C.c_int()
        self.lib.call("sim_is_running", self.h, node, C.byref(v))
        return bool(v.value)

    def ping_addrs(self, node: int, peers) -> None:
        arr = (C.c_uint32 * len(peers))(*peers)
        self.lib.call("sim_ping_addrs", self.h, node, arr, len(peers))

    def set_identity(self, node: int, identity: bytes) -> None:
        self.lib.call("sim_set_identity", self.h, node, identity, len(identity))

    # -- inspection --
    def identity(self, node: int) -> bytes:
        """The identity bytes of id `node` (what every view reports for it)."""
        n = C.c_size_t()
        buf = (C.c_uint8 * 32)()
        self.lib.call("sim_identity", self.h, node, buf, 32, C.byref(n))
        return bytes(buf[: n.value])

    def fingerprint(self, node: int) -> int:
        v = C.c_uint32()
        self.lib.call("sim_fingerprint", self.h, node, C.byref(v))
        return v.value

    def fingerprints(self):
        import numpy as np
        out = np.zeros(self.capacity, dtype=np.uint32)
        self.lib.call("sim_fingerprints", self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), self.capacity)
        return out

    def true_fingerprint(self) -> int:
        v = C.c_uint32()
        self.lib.call("sim_true_fingerprint", self.h, C.byref(v))
        return v.value

    def peers(self, node: int):
        n = C.c_size_t()
        self.lib.call("sim_peers", self.h, node, None, 0, C.byref(n))
        arr = (C.c_uint32 * max(n.value, 1))()
        self.lib.call("sim_peers", self.h, node, arr, n.value, C.byref(n))
        return list(arr[: n.value])

    # -- event streams (src/events.rs:18-125) --
    def watch(self, node: int) -> None:
        """Attach an observer to `node` (empty, as Kaboodle::new does, src/lib.rs:112)."""
        self.lib.call("sim_watch", self.h, node)

    def events(self, node: int):
        """Drain one batch: (discovered, departed, fingerprint, fingerprint_changed)."""
        nd, npp, fp, ch = C.c_size_t(), C.c_size_t(), C.c_uint32(), C.c_int()
        self.lib.call("sim_events", self.h, node, None, 0, C.byref(nd), None, 0, C.byref(npp), C.byref(fp),
                      C.byref(ch))
        d = (C.c_uint32 * max(nd.value, 1))()
        p = (C.c_uint32 * max(npp.value, 1))()
        self.lib.call("sim_events", self.h, node, d, nd.value, C.byref(nd), p, npp.value, C.byref(npp),
                      C.byref(fp), C.byref(ch))
        return list(d[: nd.value]), list(p[: npp.value]), fp.value, bool(ch.value)

    def peer_states(self, node: int):
        n = C.c_size_t()
        self.lib.call("sim_peer_states", self.h, node, None, 0, C.byref(n))
        arr = (KbPeerState * max(n.value, 1))()
        self.lib.call("sim_peer_states", self.h, node, arr, n.value, C.byref(n))
        return [(a.peer, a.state, a.since, a.latency_ms, bytes(a.identity[: a.identity_len])) for a in arr[: n.value]]

    def peer_states_array(self, node: int):
        """peer_states as one numpy record array (the fields of kb_peer_state): peer_states() without a Python
        tuple per entry (64K-entry rows).  Identity bytes past identity_len are whatever the library wrote there
        (zero-filled buffer), so equal arrays mean equal peer_states(), not the converse."""
        import numpy as np
        n = C.c_size_t()
        self.lib.call("sim_peer_states", self.h, node, None, 0, C.byref(n))
        a = np.zeros(max(n.value, 1), dtype=PEER_STATE_DTYPE)
        self.lib.call("sim_peer_states", self.h, node, C.cast(a.ctypes.data, C.POINTER(KbPeerState)), n.value,
                      C.byref(n))
        return a[: n.value]

    # -- discovery (src/discovery.rs:30-89, src/kaboodle.rs:305-331) --
    def probe(self, prober) -> None:
        """Queue SwimBroadcast::Probe(prober) for the next round; prober = ("a.b.c.d", port) outside the mesh."""
        self.lib.call("sim_probe", self.h, C.byref(wire_addr(prober)))

    def probe_responses(self):
        """Drain the ProbeResponses: [(round, responder id, probe index, prober addr, identity)] in canonical order."""
        n = C.c_size_t()
        self.lib.call("sim_probe_responses", self.h, None, 0, C.byref(n))
        arr = (KbProbeResponse * max(n.value, 1))()
        self.lib.call("sim_probe_responses", self.h, arr, n.value, C.byref(n))
        return [(a.round, a.responder, a.probe, (".".join(str(a.prober.ip[k]) for k in range(4)), a.prober.port),
                 bytes(a.identity[: a.identity_len])) for a in arr[: n.value]]

    def broadcasts(self):
        """The last round's Join / Failed broadcasts: [("Join" | "Failed", sender id, peer id)], sender order."""
        n = C.c_size_t()
        self.lib.call("sim_broadcasts", self.h, None, 0, C.byref(n))
        arr = (KbBroadcast * max(n.value, 1))()
        self.lib.call("sim_broadcasts", self.h, arr, n.value, C.byref(n))
        return [("Join" if a.kind == 16 else "Failed", a.sender, a.peer) for a in arr[: n.value]]

    # -- external peers: real instances attached through a bridge --
    def set_external(self, node: int) -> None:
        """Mark a never-bound address as an external peer (kb_sim_set_external)."""
        self.lib.call("sim_set_external", self.h, node)
        self.external.add(node)

    def inject(self, sender: int, dest: int, kind: int, a: int = 0, fp: int = 0, n: int = 0, ids=()) -> None:
        """Queue a record from external peer `sender` to `dest` for the next round's wave 0 (kb_sim_inject);
        kind = wire kind 0..4 (Ping, PingRequest, Ack, KnownPeers, KnownPeersRequest), or 16: the external peer's
        Join broadcast, delivered in the next round's broadcast phase (dest unused)."""
        m = KbUnicast(sender=sender, dest=dest, kind=kind, a=a, fp=fp, n=n, pay_len=len(ids))
        arr = (C.c_uint32 * max(1, len(ids)))(*ids)
        self.lib.call("sim_inject", self.h, C.byref(m), arr)

    def exported(self):
        """Drain the records routed to external peers: [(round, wave, sender, dest, seq, kind, a, fp, n, ids)]."""
        n, ni = C.c_size_t(), C.c_size_t()
        self.lib.call("sim_exported", self.h, None, 0, C.byref(n), None, 0, C.byref(ni))
        arr = (KbUnicast * max(n.value, 1))()
        ids = (C.c_uint32 * max(ni.value, 1))()
        self.lib.call("sim_exported", self.h, arr, n.value, C.byref(n), ids, ni.value, C.byref(ni))
        return [(u.round, u.wave, u.sender, u.dest, u.seq, u.kind, u.a, u.fp, u.n, list(ids[u.pay_off:u.pay_off + u.pay_len]))
                for u in arr[: n.value]]

    def stats(self) -> dict:
        st = KbStats()
        self.lib.call("sim_stats", self.h, C.byref(st))
        return st.as_dict()

    def census(self, arrays: bool = True):
        """The view census (include/kaboodle_census.h): a `Census` with `summary` (dict of kb_census) and the
        uint32 arrays `known_by`, `missing`, `stale` over all ids (None with arrays=False: the summary alone).
        Computed on the device by kb_sim_census; a library without it (the CPU oracle) answers the same call
        through census.census_ref, so both are compared through identical calls.  With arrays the Census also
        carries `running` (for the Tracker), which costs one scalars() download per call (kb_sim_census does not
        return the running set); arrays=False skips it."""
        from .census import Census, census_ref
        if "sim_census" not in self.lib.fn:
            return census_ref(self)
        out = KbCensus()
        outs, args = _out_arrays(arrays, (["u4"], self.capacity), (["u4", "u4"], self.capacity))
        self.lib.call("sim_census", self.h, C.byref(out), *args)
        return Census(out.as_dict(), *outs, self.scalars()[:, 0] != 0 if arrays else None)

    def _device_ms(self, name: str) -> float:
        """Device time in ms of the last call of census `name` on this handle (kb_sim_<name>_device_ms)."""
        v = C.c_double(0)
        self.lib.call(f"sim_{name}_device_ms", self.h, C.byref(v))
        return v.value

    def census_device_ms(self) -> float:
        """Device time of the last census() in ms (kb_sim_census_device_ms; HIP library only)."""
        return self._device_ms("census")

    def reciprocity(self, arrays: bool = True, max_pairs: int = 65536):
        """The reciprocity census (include/kaboodle_reciprocity.h): a `Reciprocity` with `summary` (dict of
        kb_reciprocity), the uint32 arrays `mutual`, `lacks`, `lacked_by` over all ids and `pairs`, the mutual
        pairs (i, j), i < j, ascending, as an [n, 2] array (empty when their number is above max_pairs: the
        summary's mutual_pairs has the total).  arrays=False: the summary alone, nothing listed.  Computed on the
        device by kb_sim_reciprocity; a library without it (the CPU oracle) answers the same call through
        reciprocity.reciprocity_ref, so both are compared through identical calls."""
        from .reciprocity import Reciprocity, reciprocity_ref
        if "sim_reciprocity" not in self.lib.fn:
            return reciprocity_ref(self, max_pairs, arrays)
        import numpy as np
        out = KbReciprocity()
        (mu, lk, lb), args = _out_arrays(arrays, (["u4"] * 3, self.capacity))
        pairs = np.zeros((max(max_pairs, 1), 2), dtype=np.uint32) if arrays else None
        self.lib.call("sim_reciprocity", self.h, C.byref(out), *args,
                      pairs.ctypes.data_as(C.POINTER(C.c_uint32)) if arrays else None, max_pairs if arrays else 0)
        return Reciprocity(out.as_dict(), mu, lk, lb, pairs[: out.pairs_listed].copy() if arrays else None)

    def reciprocity_device_ms(self) -> float:
        """Device time of the last reciprocity() in ms (kb_sim_reciprocity_device_ms; HIP library only)."""
        return self._device_ms("reciprocity")

    def fp_classes(self, top: int = 16, arrays: bool = True):
        """The fingerprint-class census (include/kaboodle_classes.h): an `FpClasses` with `summary` (dict of
        kb_fp_classes), `classes` (the first `top` <= 1024 classes in canonical order as an [n, 3] array of fp, size,
        rep) and the uint32 arrays `rep` and `size` over all ids (None with arrays=False).  Computed on the device by
        kb_sim_fp_classes; a library without it (the CPU oracle) answers the same call through
        classes.fp_classes_ref, so both are compared through identical calls."""
        if "sim_fp_classes" not in self.lib.fn:
            from .classes import fp_classes_ref
            return fp_classes_ref(self, top, arrays)
        return _fp_classes_call(self.lib, "sim_fp_classes", (self.h,), top, arrays, self.capacity)

    def fp_classes_device_ms(self) -> float:
        """Device time of the last fp_classes() in ms (kb_sim_fp_classes_device_ms; HIP library only)."""
        return self._device_ms("fp_classes")

    def latency_census(self, arrays: bool = True):
        """The latency census (include/kaboodle_latency.h): a `LatencyCensus` with `summary` (dict of
        kb_lat_census) and, over all ids, `measured_by`, `sum_ms`, `min_ms`, `max_ms` per peer and `measured`,
        `row_sum_ms` per row (None with arrays=False: the summary alone).  Computed on the device by
        kb_sim_latency_census (dense handles with track_latency); a library without it (the CPU oracle) answers the
        same call through latency.latency_census_ref, so both are compared through identical calls."""
        if "sim_latency_census" not in self.lib.fn:
            from .latency import latency_census_ref
            return latency_census_ref(self, arrays)
        return _latency_census_call(self.lib, "sim_latency_census", (self.h,), arrays, self.capacity, self.capacity)

    def latency_census_device_ms(self) -> float:
        """Device time of the last latency_census() in ms (kb_sim_latency_census_device_ms; HIP library only)."""
        return self._device_ms("latency_census")

    def age_census(self, arrays: bool = True):
        """The contact-age census (include/kaboodle_age.h): an `AgeCensus` with `summary` (dict of kb_age_census)
        and, over all ids, `suspected_by`, `ancient_by`, `windowed_by`, `fresh_by`, `last_heard` per peer and
        `suspects`, `ancient`, `windowed`, `fresh` per row (None with arrays=False).  Computed on the device by
        kb_sim_age_census (sparse rows; dense handles raise KbError); a library without it (the CPU oracle) answers the same call through age.age_census_ref,
        so both are compared through identical calls."""
        if "sim_age_census" not in self.lib.fn:
            from .age import age_census_ref
            return age_census_ref(self, arrays)
        return _age_census_call(self.lib, "sim_age_census", (self.h,), arrays, self.capacity, self.capacity)

    def age_census_device_ms(self) -> float:
        """Device time of the last age_census() in ms (kb_sim_age_census_device_ms; HIP library only)."""
        return self._device_ms("age_census")

    def delta_mark(self) -> None:
        """Take or replace the baseline of the view-delta census (kb_sim_delta_mark, include/kaboodle_delta.h): a
        device-side copy of the member bits and the running set as they are now.  A library without it (the CPU
        oracle) keeps the same baseline on the host, from row() and scalars()."""
        if "sim_delta_mark" not in self.lib.fn:
            from .delta import host_state
            self._delta_base = host_state(self)
            return
        self.lib.call("sim_delta_mark", self.h)

    def delta_census(self, advance: bool = True, arrays: bool = True):
        """The view-delta census (include/kaboodle_delta.h): a `DeltaCensus` with `summary` (dict of kb_delta) and,
        over all ids, `gained_by`, `lost_by` per id and `gained`, `lost`, `lost_live` per row (None with
        arrays=False: the summary alone), against the baseline of delta_mark().  advance=True (KB_DELTA_ADVANCE): the
        baseline becomes the current state in the same pass; advance=False: strictly read-only.  KbError
        (KB_INVALID_OPERATION, "no baseline") before a mark.  Computed on the device by kb_sim_delta_census (dense
        handles, unsharded or in-process shards); a library without it (the CPU oracle) answers the same call through
        delta.delta_ref from its host baseline, so both are compared through identical calls."""
        if "sim_delta_census" not in self.lib.fn:
            import numpy as np
            from .delta import DeltaCensus, delta_ref, host_state
            if self._delta_base is None:
                raise KbError(KB_INVALID_OPERATION, "delta_census (no baseline)")
            now = host_state(self)
            ext = np.zeros(self.capacity, dtype=bool)
            ext[list(self.external)] = True
            (b0, r0, t0), (b1, r1, t1) = self._delta_base, now
            d = delta_ref(b0, r0, b1, r1, ext, self.shard_info()[2], t0, t1)
            if advance:
                self._delta_base = now
            return d if arrays else DeltaCensus(d.summary, None, None, None, None, None)
        from .delta import DeltaCensus
        out = KbDelta()
        outs, args = _out_arrays(arrays, (["u4"] * 2, self.capacity), (["u4"] * 3, self.capacity))
        self.lib.call("sim_delta_census", self.h, C.byref(out), *args, KB_DELTA_ADVANCE if advance else 0)
        return DeltaCensus(out.as_dict(), *outs)

    def delta_release(self) -> None:
        """Free the baseline (kb_sim_delta_release); nothing happens when there is none."""
        if "sim_delta_release" not in self.lib.fn:
            self._delta_base = None
            return
        self.lib.call("sim_delta_release", self.h)

    def delta_census_device_ms(self) -> float:
        """Device time of the last delta_census() in ms (kb_sim_delta_device_ms; HIP library only); 0.0 before the
        first answer."""
        return self._device_ms("delta")

    def islands(self, arrays: bool = True):
        """The island census (include/kaboodle_islands.h): an `Islands` with `summary` (dict of kb_islands) and the
        uint32 arrays `label` (the lowest id of the id's island, KB_CENSUS_NONE where it does not run) and `size` over
        all ids (None with arrays=False: the summary alone).  Computed on the device by kb_sim_islands (dense handles,
        unsharded or in-process shards); a library without it (the CPU oracle) answers the same call through
        islands.islands_of_sim, so both are compared through identical calls."""
        if "sim_islands" not in self.lib.fn:
            from .islands import islands_of_sim
            return islands_of_sim(self, arrays)
        from .islands import Islands
        out = KbIslands()
        outs, args = _out_arrays(arrays, (["u4"] * 2, self.capacity))
        self.lib.call("sim_islands", self.h, C.byref(out), *args)
        return Islands(out.as_dict(), *outs)

    def islands_device_ms(self) -> float:
        """Device time of the last islands() in ms (kb_sim_islands_device_ms; HIP library only); 0.0 before the
        first answer."""
        return self._device_ms("islands")

    def gaps(self, max_pairs: int = 65536) -> dict:
        """The gap list (include/kaboodle_gaps.h): the fields of kb_gaps and `missing_pairs` / `stale_pairs`, the
        cells the view census counts as missing and stale as (n, 2) uint32 arrays of (row, id), ascending; None for a
        list of more than max_pairs pairs (the totals are still there).  max_pairs=0: the totals alone.  Computed on
        the device by kb_sim_gaps (dense handles, unsharded or in-process shards); a library without it (the CPU
        oracle) answers the same call through gaps.gaps_of_sim, so both are compared through identical calls."""
        if "sim_gaps" not in self.lib.fn:
            from .gaps import gaps_of_sim
            return gaps_of_sim(self, max_pairs)
        import numpy as np
        out = KbGaps()
        bufs = [np.empty((max_pairs, 2), dtype=np.uint32) if max_pairs else None for _ in range(2)]
        args = [a for b in bufs for a in (b.ctypes.data_as(C.POINTER(C.c_uint32)) if max_pairs else None, max_pairs)]
        self.lib.call("sim_gaps", self.h, C.byref(out), *args)
        d = out.as_dict()
        for name, b in zip(("missing", "stale"), bufs):
            listed = max_pairs and d[name] <= max_pairs
            d[name + "_pairs"] = b[: d[name]].copy() if listed else None
        return d

    def gaps_device_ms(self) -> float:
        """Device time of the last gaps() in ms (kb_sim_gaps_device_ms; HIP library only); 0.0 before the first
        answer."""
        return self._device_ms("gaps")

    def holders(self, ids, max_rows: int | None = None):
        """The holders query (include/kaboodle_gaps.h): for each of 1 .. KB_HOLDERS_MAX ids the observers whose view
        holds it.  Returns (offsets, rows): offsets uint64 [len(ids) + 1], rows uint32 with query q's observers
        ascending at rows[offsets[q]:offsets[q + 1]]; rows is None when there are more than max_rows of them (default:
        no limit).  Computed on the device by kb_sim_holders (dense handles, unsharded or in-process shards); a
        library without it (the CPU oracle) answers the same call through gaps.holders_of_sim."""
        if "sim_holders" not in self.lib.fn:
            from .gaps import holders_of_sim
            return holders_of_sim(self, ids, max_rows)
        import numpy as np
        q = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        cap = len(q) * self.capacity if max_rows is None else int(max_rows)
        off = np.zeros(len(q) + 1, dtype=np.uint64)
        rows = np.empty(cap, dtype=np.uint32) if cap else None        # untouched pages cost nothing
        n = C.c_uint64(0)
        self.lib.call("sim_holders", self.h, q.ctypes.data_as(C.POINTER(C.c_uint32)), len(q),
                      off.ctypes.data_as(C.POINTER(C.c_uint64)),
                      rows.ctypes.data_as(C.POINTER(C.c_uint32)) if cap else None, cap, C.byref(n))
        return off, (rows[: n.value].copy() if cap and n.value <= cap else None)

    def holders_device_ms(self) -> float:
        """Device time of the last holders() in ms (kb_sim_holders_device_ms; HIP library only); 0.0 before the first
        answer."""
        return self._device_ms("holders")

    def snapshot(self) -> bytes:
        """The mesh's state after the last completed round as one byte string (kb_sim_snapshot,
        include/kaboodle_snapshot.h): canonical, the same bytes from an unsharded handle and a group of shards.
        Sparse rows; dense rows, rank shards and a handle with calls queued for the next round raise KbError."""
        n = C.c_uint64(0)
        self.lib.call("sim_snapshot", self.h, None, 0, C.byref(n))
        buf = C.create_string_buffer(n.value)
        self.lib.call("sim_snapshot", self.h, buf, n.value, C.byref(n))
        return buf.raw[: n.value]

    @classmethod
    def restore(cls, lib: SimLib, blob: bytes, shards: int = 0, device: int = -1) -> "Sim":
        """A new handle in the state of `blob` (kb_sim_restore): shards 0 or 1 unsharded, 2..8 an in-process group
        of row shards, whatever layout wrote the snapshot.  It continues bit for bit as the source would; observers
        (watch) and undrained outputs are not carried."""
        info = KbSnapshotInfo()
        lib.call("snapshot_info_of", blob, len(blob), C.byref(info))
        h = C.c_void_p()
        lib.call("sim_restore", blob, len(blob), shards, device, C.byref(h))
        self = cls.__new__(cls)
        self.lib, self.cfg = lib, SimConfig.from_c(info.cfg)
        self.cfg.device = device
        self._c = self.cfg.to_c()
        self.h = h
        self.capacity = self.cfg.capacity
        self.external = set()
        self._delta_base = None
        return self

    def snapshot_device_ms(self) -> float:
        """Device time of the last snapshot()'s pack, or of the restore that made this handle, in ms
        (kb_sim_snapshot_device_ms)."""
        return self._device_ms("snapshot")

    def row(self, node: int):
        import numpy as np
        out = np.zeros(self.capacity, dtype=np.uint8)
        self.lib.call("sim_dump_row", self.h, node, out.ctypes.data_as(C.POINTER(C.c_uint8)), self.capacity)
        return out

    def rows(self):
        import numpy as np
        return np.stack([self.row(i) for i in range(self.capacity)])

    def scalars(self):
        import numpy as np
        out = np.zeros((self.capacity, 4), dtype=np.int32)
        self.lib.call("sim_dump_scalars", self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size)
        return out

    def suspects(self, node: int):
        n = C.c_size_t()
        buf = (C.c_int32 * (3 * 8))()
        self.lib.call("sim_dump_suspects", self.h, node, buf, len(buf), C.byref(n))
        return [tuple(buf[3 * k: 3 * k + 3]) for k in range(n.value)]

    def curious(self, node: int):
        n = C.c_size_t()
        buf = (C.c_int32 * (6 * 8))()
        self.lib.call("sim_dump_curious", self.h, node, buf, len(buf), C.byref(n))
        return [tuple(buf[6 * k: 6 * k + 6]) for k in range(n.value)]

    def checkpoints(self, node: int):
        """The fingerprint checkpoints of `node` as stored, nothing refolded (kb_sim_dump_checkpoints): (seg, stale,
        dirty, fp_cached) with seg a uint32 [64, 2] array of (raw, cnt), stale the mask of stale checkpoints, dirty
        the cached fingerprint's stale flag."""
        import numpy as np
        seg = np.zeros((NSEG, 2), dtype=np.uint32)
        stale, dirty, fp = C.c_uint64(), C.c_uint32(), C.c_uint32()
        self.lib.call("sim_dump_checkpoints", self.h, node, seg.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(stale),
                      C.byref(dirty), C.byref(fp))
        return seg, stale.value, dirty.value, fp.value

    def fold_probe(self, path: int, rows, running, bits, stale, segp_in, split: int = 0):
        """kb_sim_debug_fold: the fingerprint kernels of `path` (KB_FOLD_*) over the caller's rows.  rows: ascending
        ids; running: a flag per row; bits: uint32 [nrows, W/32] member bitsets (W = capacity rounded up to 8192);
        stale: a uint64 mask per row; segp_in: uint32 [nrows, 64, 2] checkpoints, stored verbatim.  Returns (segp_out
        [nrows, 64, 2], stale_out, dirty_out, fp_out, fold_bytes).  The handle never steps afterwards."""
        import numpy as np
        n = len(rows)
        W = (self.capacity + 8191) // 8192 * 8192
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        run = np.ascontiguousarray(np.asarray(running) != 0, dtype=np.uint8)
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        st = np.ascontiguousarray(stale, dtype=np.uint64)
        sin = np.ascontiguousarray(segp_in, dtype=np.uint32)
        if run.shape != (n,) or st.shape != (n,) or bits.shape != (n, W // 32) or sin.shape != (n, NSEG, 2):
            raise ValueError("fold_probe: array shapes do not match the rows")
        sout = np.zeros((n, NSEG, 2), dtype=np.uint32)
        stout = np.zeros(n, dtype=np.uint64)
        dout, fout = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        fb = C.c_uint64()
        u32, u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        p = KbFoldProbe(path=path, split=split, nrows=n, rows=rows.ctypes.data_as(u32),
                        running=run.ctypes.data_as(C.POINTER(C.c_uint8)), bits=bits.ctypes.data_as(u32),
                        stale=st.ctypes.data_as(u64), segp_in=sin.ctypes.data_as(u32), segp_out=sout.ctypes.data_as(u32),
                        stale_out=stout.ctypes.data_as(u64), dirty_out=dout.ctypes.data_as(u32),
                        fp_out=fout.ctypes.data_as(u32), fold_bytes=C.pointer(fb))
        self.lib.call("sim_debug_fold", self.h, C.byref(p))
        return sout, stout, dout, fout, fb.value

    def format_addr(self, node: int) -> str:
        buf = C.create_string_buffer(32)
        self.lib.call("format_addr", node, buf, 32)
        return buf.value.decode()

    # -- bench surface (HIP library only) --
    def kernel_time(self, kind: int = 0):
        ms, n = C.c_double(), C.c_uint64()
        self.lib.call("sim_kernel_time", self.h, kind, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def reset_kernel_time(self) -> None:
        self.lib.call("sim_reset_kernel_time", self.h)

    def debug_paths(self) -> int:
        """OR of the kernel-variant bits (PATH_* of kb_common.h) that did work; 0 for the oracle.  Bits 1..512:
        the wide-row variants and wave 0's deferred pass; 1024..8192: the paths chosen by list lengths (row pass
        with HBM lists, KPR proof on a wrapped log ring, > 1024 new joiners in k_resp_node, a Join response
        past the union slots crossing shards as a list)."""
        if "sim_debug_paths" not in self.lib.fn:
            return 0
        v = C.c_uint32()
        self.lib.call("sim_debug_paths", self.h, C.byref(v))
        return v.value

    def kernel_bytes(self, kind: int = 0) -> int:
        """Algorithmic bytes the kernel `kind` (KT_ROWPASS / KT_FOLD / KT_RESP / KT_PROC) moved since
        reset_kernel_time."""
        v = C.c_uint64()
        self.lib.call("sim_kernel_bytes", self.h, kind, C.byref(v))
        return v.value

    def set_profiling(self, level: int) -> None:
        """Per-launch HIP events (kernel_breakdown): 0 none, 1 the byte-counted kernels (default), 2 every launch."""
        self.lib.call("sim_set_profiling", self.h, int(level))

    def kernel_breakdown(self) -> dict:
        """{kernel: {"ms", "launches", "bytes" (None if not counted), "wave_ms": [...]}} since reset_kernel_time."""
        n = C.c_size_t()
        self.lib.call("sim_kernel_breakdown", self.h, None, 0, C.byref(n))
        arr = (KbKernelTime * max(n.value, 1))()
        self.lib.call("sim_kernel_breakdown", self.h, arr, n.value, C.byref(n))
        return {a.name.decode(): {"ms": a.ms, "launches": a.launches, "bytes": a.bytes if a.has_bytes else None,
                                  "wave_ms": list(a.wave_ms)} for a in arr[: n.value]}

    def sparse_footprint(self) -> dict:
        """KB_VARIANT_SPARSE_ROWS: rows that adopted the base, exceptions, explicit stamps, entries of the largest
        row, bytes of the entries, rows (kb_sim_sparse_footprint)."""
        out = (C.c_uint64 * 6)()
        self.lib.call("sim_sparse_footprint", self.h, out, 6)
        keys = ("rows_based", "exceptions", "stamps", "max_row_entries", "bytes", "rows")
        return dict(zip(keys, (int(v) for v in out)))

    def host_syncs(self) -> int:
        """Host waits on the device since creation (stream synchronisations, pinned hand-offs)."""
        v = C.c_uint64()
        self.lib.call("sim_host_syncs", self.h, C.byref(v))
        return v.value
