"""The snapshot surface without a GPU (include/kaboodle_snapshot.h): the header's declarations against the ctypes
mirror and the library's exports, the committed version-1 snapshot read by kb_snapshot_info_of, and the validation
every restore runs before it touches a device."""
from __future__ import annotations

import ctypes as C
import os
import re
import zlib

import pytest

import parity
from kaboodle_amd._ffi import (KB_ABI_VERSION, KB_INVALID_ARGUMENT, KB_NO_DEVICE, KB_OK, KB_SNAPSHOT_VERSION,
                               KB_VARIANT_SPARSE_ROWS, KbConfig, KbError, KbSnapshotInfo, SimLib)
from kaboodle_amd import snapshot
from parity import GPU_SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kaboodle_snapshot.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "snapshot_v1_fresh_ids.bin")
FUNCS = ("kb_snapshot_info_of", "kb_sim_snapshot", "kb_sim_restore", "kb_sim_snapshot_device_ms")
built = pytest.mark.skipif(not os.path.exists(GPU_SO), reason="HIP library not built (run __graft_entry__.build())")


def golden() -> bytes:
    with open(GOLDEN, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def lib() -> SimLib:
    return parity.gpu_lib()


def test_header_declares_the_surface():
    text = open(HEADER).read()
    for fn in FUNCS:
        assert re.search(rf"\bint {fn}\(", text), fn
    assert re.search(r"#define KB_SNAPSHOT_VERSION\s+1u", text)
    body = re.search(r"typedef struct kb_snapshot_info \{(.*?)\} kb_snapshot_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "kb_config": KbConfig}
    fields = []
    for typ, name, dim in re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", body):
        fields.append((name, ctype[typ] * int(dim) if dim else ctype[typ]))
    assert fields == list(KbSnapshotInfo._fields_)       # the mirror has the header's layout
    assert C.sizeof(KbSnapshotInfo) == 8 + C.sizeof(KbConfig) + 8 + 16 + 4 + 7 * 4


@built
def test_hip_library_exports_the_surface(lib):
    raw = C.CDLL(GPU_SO)
    assert [fn for fn in FUNCS if not hasattr(raw, fn)] == []
    assert all(fn[3:] in lib.fn for fn in FUNCS)


@built
def test_golden_info(lib):
    blob = golden()
    assert len(blob) < 64 * 1024
    info = snapshot.info(blob, lib)
    case = parity.with_cfg({n: c for n, c, _ in parity.standard_cases()}["fresh_ids"], variant=KB_VARIANT_SPARSE_ROWS,
                           track_latency=0)
    want = case["cfg"].to_c()
    assert info["format_version"] == KB_SNAPSHOT_VERSION == 1 and info["abi_version"] == KB_ABI_VERSION
    assert info["cfg"] == {n: int(getattr(want, n)) for n, _ in KbConfig._fields_ if n != "reserved"}
    assert info["round"] == 7                            # taken after round 6
    assert info["bytes"] == len(blob)
    # fresh_ids after round 6 on the sparse oracle: who runs is the mesh's state, whoever simulates it
    from kaboodle_amd._ffi import Sim
    with Sim(parity.oracle_lib(), case["cfg"]) as o:
        parity.setup(o, case)
        for r in range(7):
            parity.apply_events((o,), case, r)
            o.step(1)
        assert info["alive"] == o.stats()["alive"]
    assert blob[:8] == b"KBSNAPLE"                       # little-endian, and the magic says so
    hdr = 24 + C.sizeof(KbConfig) + 32                   # magic, versions and sizes; the config; round .. section count
    assert info["payload_crc32"] == zlib.crc32(blob[hdr:])   # zlib's CRC-32 of everything after the header


def corruptions(blob: bytes) -> dict:
    v2 = bytearray(blob)
    v2[8:12] = (2).to_bytes(4, "little")
    flip = bytearray(blob)
    flip[len(blob) // 2] ^= 0x10
    return {"truncated": blob[: len(blob) - 100], "first byte": bytes([blob[0] ^ 0xFF]) + blob[1:], "version 2": bytes(v2),
            "payload byte": bytes(flip)}


@built
def test_corrupt_snapshots_are_invalid_arguments(lib):
    texts = {}
    for what, bad in corruptions(golden()).items():
        seen = []
        for call in ("info", "restore"):
            with pytest.raises(KbError) as e:
                if call == "info":
                    snapshot.info(bad, lib)
                else:
                    lib.call("sim_restore", bad, len(bad), 0, -1, C.byref(C.c_void_p()))
            assert e.value.code == KB_INVALID_ARGUMENT, (what, call)
            seen.append(str(e.value).split("(", 1)[1])
        assert seen[0] == seen[1], what                  # both say the same thing
        texts[what] = seen[0]
    assert len(set(texts.values())) == len(texts), texts     # and each corruption its own
    assert "truncated" in texts["truncated"] and "magic" in texts["first byte"]
    assert "format_version" in texts["version 2"] and "checksum" in texts["payload byte"]
    with pytest.raises(KbError) as e:
        snapshot.info(golden()[:20], lib)
    assert e.value.code == KB_INVALID_ARGUMENT


@built
def test_intact_snapshot_needs_only_a_device(lib):
    blob = golden()
    h = C.c_void_p()
    rc = lib.fn["sim_restore"](blob, len(blob), 0, -1, C.byref(h))
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if have_gpu:
        assert rc == KB_OK
        lib.call("sim_destroy", h)
    else:
        assert rc == KB_NO_DEVICE and b"device" in lib.fn["last_error"]()
    rc = lib.fn["sim_restore"](blob, len(blob), 9, -1, C.byref(h))   # validated before the device is asked for
    assert rc == KB_INVALID_ARGUMENT and b"shard" in lib.fn["last_error"]()
