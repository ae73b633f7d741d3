"""Snapshots of a mesh (include/kaboodle_snapshot.h): what a snapshot's header says, read on the
host.  Taking and restoring one are `Sim.snapshot` / `Sim.restore` and `Mesh.save` / `Mesh.load`."""
from __future__ import annotations

import ctypes as C

from ._ffi import KbSnapshotInfo, SimLib


def info(blob: bytes, lib: SimLib | None = None) -> dict:
    """kb_snapshot_info_of: format_version, abi_version, cfg (the kb_config's fields), round, alive, entries, bytes
    and payload_crc32 of a snapshot, validated as a restore validates it (KbError KB_INVALID_ARGUMENT with the
    library's text otherwise).  Needs the built library, no GPU."""
    if lib is None:
        from . import lib as _lib
        lib = _lib()
    out = KbSnapshotInfo()
    lib.call("snapshot_info_of", blob, len(blob), C.byref(out))
    return out.as_dict()
