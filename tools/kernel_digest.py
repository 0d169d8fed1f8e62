#!/usr/bin/env python3
"""Resource line and instruction-text digest of every kernel in the matrix-pipe CNN sources.

    python tools/kernel_digest.py --out before.json            # compile the tree as it stands
    python tools/kernel_digest.py --compare before.json after.json

A refactor that leaves a kernel's digest equal left its machine code equal.  The script compiles
(device side only, the library's flags) and hashes; it looks at nothing inside the instruction text.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "suo_slam_amd", "csrc")
FILES = ["conv.hip", "conv_wino.hip", "conv_wino_x3.hip", "conv_wino_x3_dma.hip", "conv_wino_x3_skip_dma.hip", "conv_wino_x3_one_pass.hip", "gemm_bf16x3.hip", "gemm_persist.hip",
         "res_small.hip", "res_small_x3.hip", "stem_x3.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage", "-o", "-"]
FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("VGPRs Spill", "vspill"), ("SGPRs Spill", "sspill"),
          ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ")]


def one_file(name, extra):
    p = subprocess.run([HIPCC] + FLAGS + extra + [os.path.join(CSRC, name)], capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"hipcc failed on {name}:\n{p.stderr[-4000:]}")
    res, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: (?:\S+: )?Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None:
            for label, key in FIELDS:
                if m.group(1).strip() == label:
                    cur[key] = int(m.group(2))
    out, body, kern = {}, None, None
    for line in p.stdout.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and m.group(1) in res and body is None:
            kern, body = m.group(1), []
            continue
        if body is not None:
            if line.startswith(".Lfunc_end"):
                out[f"{name}:{kern}"] = dict(res[kern], digest=hashlib.sha256("\n".join(body).encode()).hexdigest()[:16])
                body = None
                continue
            s = line.split(";")[0].rstrip()      # comment lines and trailing comments dropped
            if s and "__hip_cuid" not in s:
                body.append(s)
    return out


def compile_all(extra):
    table = {}
    with ThreadPoolExecutor(max_workers=min(len(FILES), os.cpu_count() or 1, 16)) as ex:
        for part in ex.map(lambda f: one_file(f, extra), [f for f in FILES if os.path.exists(os.path.join(CSRC, f))]):
            table.update(part)
    return table


def compare(a, b):
    keys = [k for _, k in FIELDS]
    same_res = same_dig = 0
    print(f"# {'kernel':<110} {' '.join(keys):<44} | after | digest before / after")
    for k in sorted(set(a) | set(b)):
        ra, rb = a.get(k), b.get(k)
        fa = " ".join(str(ra.get(x, "-")) for x in keys) if ra else "absent"
        fb = " ".join(str(rb.get(x, "-")) for x in keys) if rb else "absent"
        da, db = (ra or {}).get("digest", "-"), (rb or {}).get("digest", "-")
        same_res += fa == fb
        same_dig += da == db
        print(f"{k:<112} {fa:<44} | {'same' if fa == fb else fb} | {da} {'same' if da == db else db}")
    n = len(set(a) | set(b))
    print(f"# {n} kernels: resources equal for {same_res}, digest equal for {same_dig}")
    return same_res == n


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--files", nargs="+", help="only these sources (default: all nine)")
    ap.add_argument("--csrc", help="compile the sources of another tree's csrc directory (e.g. a checkout of the parent commit)")
    ap.add_argument("flags", nargs="*", help="extra compiler flags after --, e.g. -- -DSUO_X3_BK=32")
    args = ap.parse_args()
    if args.compare:
        sys.exit(0 if compare(*(json.load(open(f)) for f in args.compare)) else 1)
    if args.files:
        FILES[:] = args.files
    if args.csrc:
        CSRC = os.path.abspath(args.csrc)
    t = compile_all(args.flags)
    if args.out:
        json.dump(t, open(args.out, "w"), indent=0, sort_keys=True)
    print(f"{len(t)} kernels")
