"""Kernel resource usage of two builds, side by side, from the compiler's remarks.

    hipcc --offload-arch=gfx950 ... -Rpass-analysis=kernel-resource-usage ... 2> remarks.txt     (once per tree)
    python tools/kernel_resources.py parent_remarks.txt new_remarks.txt k_cs_dense k_delta ... > out.json

Kernels are matched by the short name inside the mangled one; a kernel whose name differs between the trees is given
as parent=new (k_cs_masks=k_id_masks).  Exits 1 when a kernel has scratch, its LDS differs or its occupancy fell."""
from __future__ import annotations

import json
import re
import sys

FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}


def parse(path: str) -> dict[str, dict[str, int]]:
    out: dict[str, dict[str, int]] = {}
    cur = None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def find(table: dict, short: str) -> tuple[str, dict]:
    hits = [(k, v) for k, v in table.items() if re.search(rf"\d{re.escape(short)}E", k)]
    if len(hits) != 1:
        raise SystemExit(f"{short}: {len(hits)} kernels match")
    return hits[0]


def main() -> int:
    parent, new = parse(sys.argv[1]), parse(sys.argv[2])
    rows, bad = [], 0
    for spec in sys.argv[3:]:
        pn, _, nn = spec.partition("=")
        (pk, p), (nk, n) = find(parent, pn), find(new, nn or pn)
        moved = {f: n[f] - p[f] for f in ("vgprs", "sgprs") if n[f] != p[f]}
        ok = n["scratch"] == 0 and p["scratch"] == 0 and n["lds_bytes"] == p["lds_bytes"] and n["waves_per_simd"] >= p["waves_per_simd"]
        bad += not ok
        rows.append({"kernel": nn or pn, "parent_symbol": pk, "symbol": nk, "parent": p, "new": n, "moved": moved, "ok": ok})
    json.dump({"arch": "gfx950", "flags": "-O3 -Rpass-analysis=kernel-resource-usage", "kernels": rows}, sys.stdout, indent=1)
    print()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
