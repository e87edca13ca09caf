"""In-tree build of libvapor_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "libvapor_hip.so")
CSRC = os.path.join(HERE, "csrc")
SOURCES = [os.path.join(CSRC, "vapor_hip.hip"), os.path.join(CSRC, "vapor_bam.cpp")]
# The csrc headers, once, in the order both lists below keep.  The ones that hold device code are part of kernel_source_id();
# vapor_records.h holds the records the kernels read, vapor_names.h the name key and drop rule bam_dedup_kernel shares with the host reader.  vapor_inflate.h, vapor_bgzf.h (the BGZF block parser and scans of the host and
# device readers), vapor_planner.h (share groups, plan layout, clean order) and vapor_readplan.h (the plan of a device reader call, over the
# records of vapor_readrec.h that the readers' kernels read) are host-only; vapor_realign_plan.h is host arithmetic too, but realign_kernel reads its
# constants and functions, so it counts as device code.  A new route's header goes here.
_HEADERS = [("vapor_kernels.h", True), ("vapor_wide.h", True), ("vapor_anyk.h", True), ("vapor_inflate.h", False),
            ("vapor_bamdev.h", True), ("vapor_fasta.h", True), ("vapor_refine.h", True), ("vapor_bgzf.h", False),
            ("vapor_records.h", True), ("vapor_planner.h", False), ("vapor_names.h", True),
            ("vapor_readrec.h", True), ("vapor_readplan.h", False), ("vapor_sa.h", False),
            ("vapor_realign.h", True), ("vapor_realign_plan.h", True),
            # (the band row the realign, trace and junction kernels walk)
            ("vapor_band_row.h", True),
            # (`--realign-out`, DESIGN.md 4.24: the trace kernels, and their host arithmetic, which they read as well)
            ("vapor_realign_trace.h", True), ("vapor_trace_plan.h", True),
            # (`--realign-polish`, DESIGN.md 4.25: the pileup and consensus kernels and the plan they read)
            ("vapor_polish.h", True), ("vapor_polish_plan.h", True),
            # (`--realign-junction`, DESIGN.md 4.26: the row-table and pick kernels and the plan they read)
            ("vapor_junction.h", True), ("vapor_junction_plan.h", True),
            # (`--realign-revote`, DESIGN.md 4.27: the spelling and re-vote kernels and the plan they read)
            ("vapor_revote.h", True), ("vapor_revote_plan.h", True),
            # (the host plan of one polish / re-vote call, put together from the two plans above: host-only, no kernel reads it)
            ("vapor_polish_call.h", False),
            # (the host plan of one vapor_seqset_create* call, and the refusal and image tables the host plans share: host-only)
            ("vapor_seqset_plan.h", False), ("vapor_image.h", False),
            # (the host side of a clean launch; the clean kernels take their constants and their LDS layout from it: device code)
            ("vapor_clean_plan.h", True),
            # (the host side of the explicit-dot routes; vapor_wide.h takes WideAcc and vapor_anyk.h its constants from it: device code)
            ("vapor_dots_plan.h", True),
            # (the host side of the finishing and grid calls; oracle/cpu_twin.cpp reads it too: host-only)
            ("vapor_finish_plan.h", False),
            # (the block pool's policy, DESIGN.md 4.12: host-only)
            ("vapor_pool.h", False)]
DEPS = SOURCES + [os.path.join(CSRC, h) for h, _dev in _HEADERS] + [os.path.join(ROOT, "include", "vapor_hip.h")]
KERNEL_FILES = [os.path.join(CSRC, h) for h, dev in _HEADERS if dev] + [SOURCES[0], os.path.abspath(__file__)]

# The kernels issue their wave-level atomics from one lane already (`if (lane == 0) atomicAdd(...)`); LLVM's atomic
# optimizer wraps each of them in another mbcnt / compare / exec-mask sequence.  Off: clean_kernel 0.0837 -> 0.0826 ms.
# The kernels are vector-issue-bound with their occupancy set by LDS, not by registers: the scheduler strategy that orders for
# instruction-level parallelism instead of for the fewest registers takes a cfg2 pass from 0.1258 to 0.1246 ms (two plans in
# flight; cfg3 the same within 0.2 %, checksums equal; profiles/r05_sched_strategy.txt).
EXTRA_FLAGS = ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


_ID_RE = re.compile(rb"VAPOR_SOURCE_ID=([0-9a-f]{16}:[0-9a-f]{16})")


def _sha16(paths) -> str:
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def kernel_source_id() -> str:
    """sha256 (16 hex digits) over the device code, the host code that launches it and this file (the compiler flags): what a
    committed counter summary must have been measured on.  The host-only helpers (BAM reader, inflate) and the header's
    prose are not part of it: they cannot move a kernel's counters."""
    return _sha16(KERNEL_FILES)


def source_id() -> str:
    """`<kernel_source_id>:<sha over every file the library is built from>` - compiled into the library (vapor_source_id())."""
    return kernel_source_id() + ":" + _sha16(sorted(set(DEPS + [os.path.abspath(__file__)])))


def embedded_source_id(so: str = SO):
    """The id a built library carries, read from the file itself (no dlopen); None for a library built without one."""
    try:
        with open(so, "rb") as f:
            m = _ID_RE.search(f.read())
    except OSError:
        return None
    return m.group(1).decode() if m else None


def build(force: bool = False, verbose: bool = False) -> str:
    # (the binary is tied to its sources by content, not by mtime: a library travels to the GPU box in the working tree, and
    # one that is newer than sources it was not built from would be quoted against fresh counters silently)
    sid = source_id()
    if not force and os.path.exists(SO) and embedded_source_id() == sid:
        return SO
    cmd = [hipcc(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared", '-DVAPOR_SOURCE_ID="%s"' % sid] + EXTRA_FLAGS + [
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"),
           "-Wall", "-Wno-unused-function", "-o", SO] + SOURCES + ["-lz"]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
