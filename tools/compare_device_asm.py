#!/usr/bin/env python3
"""Is the gfx950 device code of every product source the same at two revisions?  Needs hipcc only: no GPU, no network.
    python tools/compare_device_asm.py <rev_a> [<rev_b>]        (rev_b omitted: the working tree)
Each revision's absolutetrack_amd/csrc and include/ are exported with `git archive` into a temporary directory; every entry of
build.py's SOURCES is compiled there with the product flags plus `--offload-device-only -S`, and the two texts are compared
with the lines naming `__hip_cuid_` (a hash of the source file) left out.  Kernel names, register counts, LDS sizes and scratch
use are part of that text.  Prints one verdict per file; the exit status is the number of files that differ."""
import concurrent.futures
import io
import os
import shutil
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from absolutetrack_amd.build import FLAGS, SOURCES  # noqa: E402

PATHS = ["absolutetrack_amd/csrc", "include"]


def export(rev, dst):
    if rev is None:
        for p in PATHS:
            shutil.copytree(os.path.join(ROOT, p), os.path.join(dst, p))
    else:
        tar = subprocess.check_output(["git", "-C", ROOT, "archive", rev, "--"] + PATHS)
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(dst)
    return os.path.join(dst, "absolutetrack_amd", "csrc")


def device_asm(csrc, name):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = os.path.join(csrc, name + ".s")
    if not os.path.exists(os.path.join(csrc, name)):      # a source that one of the two revisions does not have
        return None
    subprocess.check_call([hipcc] + FLAGS + ["-Wno-unused-command-line-argument", "--offload-device-only", "-S", name, "-o", out], cwd=csrc)
    return [line for line in open(out) if "__hip_cuid_" not in line]


def main():
    rev_a, rev_b = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None
    with tempfile.TemporaryDirectory() as tmp:
        dirs = [export(rev, os.path.join(tmp, side)) for side, rev in (("a", rev_a), ("b", rev_b))]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            asm = list(pool.map(lambda job: device_asm(*job), [(d, f) for d in dirs for f in SOURCES]))
    differ = 0
    for i, f in enumerate(SOURCES):
        a, b = asm[i], asm[len(SOURCES) + i]
        if a is None or b is None:
            print(f"{f:20s} only in {rev_a if b is None else rev_b or 'the working tree'}")
            continue
        same = a == b
        differ += not same
        print(f"{f:20s} {'identical' if same else 'DIFFERENT'}   ({len(a)} lines)")
    print(f"{len(SOURCES) - differ} of {len(SOURCES)} identical or new: {rev_a} vs {rev_b or 'working tree'}")
    return differ


if __name__ == "__main__":
    sys.exit(main())
