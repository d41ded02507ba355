"""Digest of the device code of every kernel file, to show that a change of the sources left the kernels as they were.

Each file of build.SOURCES is compiled with build.FLAGS plus `--offload-device-only -S`; of the assembly text, blank lines, lines whose
first non-blank character is `;` or `.` (comments, directives, labels' metadata) and lines that hold the per-build unit id `__hip_cuid_`
are dropped.  What is left is the instruction stream with its labels.  Printed per file: the number of lines and their sha256.

    python tools/device_code_digest.py [FILE.hip ...]                 (default: every file of build.SOURCES)
    python tools/device_code_digest.py --against OTHER/csrc [-D...]   (another tree's csrc: which files differ, and the first differing lines)

Needs the compiler only, no GPU.  Exit status 1 when a file differs.
"""
import difflib
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sup-nerf_amd"))
from build import CSRC, FLAGS, HIPCC, SOURCES  # noqa: E402


def device_lines(path, defines=()):
    cmd = [HIPCC] + FLAGS + list(defines) + ["--offload-device-only", "-S", path, "-o", "-"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + p.stderr)
    keep = []
    for line in p.stdout.splitlines():
        s = line.lstrip()
        if not s or s[0] in ";." or "__hip_cuid_" in line:
            continue
        keep.append(line)
    return keep


def main(argv):
    against = argv[argv.index("--against") + 1] if "--against" in argv else None
    defines = [a for a in argv if a.startswith("-D")]
    names = [a for a in argv if a.endswith(".hip")] or SOURCES
    jobs = [(n, os.path.join(CSRC, n)) for n in names]
    if against:
        jobs += [(n, os.path.join(against, n)) for n in names]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        out = list(pool.map(lambda j: device_lines(j[1], defines) if os.path.exists(j[1]) else None, jobs))
    differ = 0
    for i, n in enumerate(names):
        here = out[i]
        sha = hashlib.sha256("\n".join(here).encode()).hexdigest()
        if not against:
            print(f"{n:20s} {len(here):7d} lines  sha256 {sha}")
            continue
        if not os.path.exists(os.path.join(against, n)):
            print(f"{n:20s} {len(here):7d} lines  sha256 {sha}  (not in {against})")
            continue
        there = out[len(names) + i]
        if here == there:
            print(f"{n:20s} {len(here):7d} lines  sha256 {sha}  identical")
            continue
        differ += 1
        delta = [d for d in difflib.unified_diff(there, here, "against/" + n, n, n=0, lineterm="")]
        changed = sum(1 for d in delta[2:] if d[0] in "+-")
        print(f"{n:20s} {len(here):7d} lines (against: {len(there)})  DIFFERS: {changed} lines added or removed; the first:")
        print("\n".join("    " + d for d in delta[:14]))
    if against:
        print("no differing file" if not differ else f"{differ} file(s) differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
