#!/usr/bin/env python
"""Register budget of the gfx950 kernels in one or two builds of librubiks_hip.so, from the code-object metadata (no GPU):
VGPRs, AGPRs, SGPRs and scratch bytes of every kernel whose name matches, and -- with two libraries -- what changed.

    python tools/kernel_regs.py [--match REGEX] BEFORE.so [AFTER.so]

With two libraries the exit status is 1 when a kernel gained scratch where it had none or crossed a step of the
waves-per-SIMD table (MI355X: VGPRs and AGPRs share 512 registers per lane, allocated in granules of 8;
waves per SIMD = min(8, 512 // allocation): <=64 -> 8, 72 -> 7, 80 -> 6, 88-96 -> 5, 104-128 -> 4, 136-168 -> 3,
176-256 -> 2, 264-512 -> 1).  Differences inside a step are listed only.
"""
import argparse
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asm_hazard_check  # noqa: E402

_FIELD = re.compile(r"^  [- ] \.(name|vgpr_count|agpr_count|sgpr_count|private_segment_fixed_size):\s*(\S+)")


def waves_per_simd(vgpr, agpr):
    alloc = max(8, -(-(vgpr + agpr) // 8) * 8)
    return min(8, 512 // alloc)


def kernels(lib, match):
    """{kernel name: (vgpr, agpr, sgpr, scratch bytes)} over every gfx950 code object of the library"""
    out = {}
    pat = re.compile(match)
    for co in asm_hazard_check.code_objects(lib):
        notes = subprocess.run([os.path.join(asm_hazard_check.LLVM, "llvm-readelf"), "--notes", co], capture_output=True,
                               text=True, check=True).stdout
        cur = {}

        def flush():
            if "sgpr_count" in cur and pat.search(cur.get("name", "")):
                out[cur["name"]] = (int(cur["vgpr_count"]), int(cur.get("agpr_count", 0)), int(cur["sgpr_count"]),
                                    int(cur["private_segment_fixed_size"]))

        for line in notes.splitlines():
            if line.startswith("  - ."):                               # a kernel record begins (its argument records sit deeper)
                flush()
                cur = {}
            m = _FIELD.match(line)
            if m:
                cur[m.group(1)] = m.group(2).strip("'\"")
        flush()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--match", default="_backward|finalize")
    ap.add_argument("before")
    ap.add_argument("after", nargs="?")
    a = ap.parse_args()
    before = kernels(a.before, a.match)
    after = kernels(a.after, a.match) if a.after else None
    bad = changed = 0
    print("# kernels matching /%s/: %d%s" % (a.match, len(before), "" if after is None else " before, %d after" % len(after)))
    print("# columns: vgpr agpr sgpr scratch_bytes waves_per_simd" + ("  (before -> after)" if after is not None else ""))
    for name in sorted(set(before) | set(after or {})):
        b, n = before.get(name), (after or {}).get(name)
        if after is None:
            print("%3d %3d %3d %5d  w%d  %s" % (b + (waves_per_simd(b[0], b[1]), name)))
            continue
        if b is None or n is None:
            print("%s  %s" % ("ADDED  " if b is None else "REMOVED", name))
            continue
        wb, wn = waves_per_simd(b[0], b[1]), waves_per_simd(n[0], n[1])
        verdict = "same"
        if (b[3] == 0 and n[3] != 0) or wn < wb:
            verdict, bad = "FAIL", bad + 1
        elif wn > wb:                                            # fewer registers: a step up is a crossing all the same
            verdict, bad = "CROSSED-UP", bad + 1
        elif b != n:
            verdict, changed = "differs-within-step", changed + 1
        print("%3d %3d %3d %5d w%d -> %3d %3d %3d %5d w%d  %-19s %s" % (b + (wb,) + n + (wn, verdict, name)))
    if after is not None:
        print("# %d kernel(s) differ inside an occupancy step, %d crossed a step or gained scratch" % (changed, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
