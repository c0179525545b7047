#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly listings of one translation unit (before / after a refactor).

  hipcc <the library's flags> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage x.hip -o a.s 2> a.res     (both trees)
  python tools/diag/asm_diff.py a.s b.s [a.res b.res]

A kernel's body is the text between its label and its .Lfunc_end, with comments, debug directives, the compilation-unit id and the
function number inside basic-block labels stripped.  Prints one JSON object: per kernel "identical" or "differs", and for the differing
ones the instruction counts and (given the remark files) VGPRs, AGPRs, SGPRs, scratch, LDS and occupancy of both sides.
"""
import json
import re
import subprocess
import sys


def bodies(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name], cur = cur, None
            continue
        s = line.split(";", 1)[0].rstrip()
        if not s.strip() or re.match(r"^\s*\.(loc|file|cfi_|p2align)", s):
            continue
        s = re.sub(r"__hip_cuid_\w+", "__hip_cuid", s)
        s = re.sub(r"\.L(BB|tmp|func_begin)\d+", r".L\1", s)
        cur.append(s.strip())
    return out


def remarks(path):
    rows, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: .*?:\d+:\d+: +(.*?) \[-Rpass", line) or re.search(r"remark: +(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:") or t.startswith("Name:"):
            cur = rows.setdefault(t.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    keys = {"VGPRs": "vgpr", "AGPRs": "agpr", "TotalSGPRs": "sgpr", "ScratchSize [bytes/lane]": "scratch_bytes",
            "LDS Size [bytes/block]": "lds_bytes", "Occupancy [waves/SIMD]": "waves_per_simd"}
    return {n: {v: int(r[k]) for k, v in keys.items() if k in r} for n, r in rows.items()}


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    ra, rb = (remarks(sys.argv[3]), remarks(sys.argv[4])) if len(sys.argv) > 4 else ({}, {})
    names = sorted(set(a) | set(b))
    # (c++filt does not know DF16b = bf16: demangle it as `half` and rename)
    filt = subprocess.run(["c++filt"] + [n.replace("DF16b", "Dh") for n in names], capture_output=True, text=True).stdout.splitlines()
    pretty = {n: f.replace("half", "bf16") for n, f in zip(names, filt)}
    per = {}
    for n in names:
        key = re.sub(r"\(.*", "", pretty.get(n, n)).replace("void ", "")
        if n not in a or n not in b:
            per[key] = {"assembly": "only in " + ("parent" if n in a else "new")}
        elif a[n] == b[n]:
            per[key] = {"assembly": "identical"}
        else:
            per[key] = {"assembly": "differs", "instructions_parent_new": [len(a[n]), len(b[n])]}
            if n in ra and n in rb:
                per[key].update(parent=ra[n], new=rb[n])
    print(json.dumps({"kernels": len(names), "identical": sum(v["assembly"] == "identical" for v in per.values()), "per_kernel": per}, indent=1))


if __name__ == "__main__":
    main()
