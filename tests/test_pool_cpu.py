"""The block pool's policy (vapor_amd/csrc/vapor_pool.h: the rounding of a request, the window of capacities a free block may have
to serve it, smallest first, the capacity the pool knows every block by, the caching limits, foreign pointers, and the test fill
of parameter pool_fill) on the host, under the address and undefined-behaviour sanitizers (tools/pool_check.cpp).  The program
holds the header to direct statements over fake allocators that log every call, and to a model of the rules written out longhand
over a seeded sequence of requests.  That the fill reaches every hand-out over the block's whole capacity before the pointer is
returned is what makes tests/test_gpu_pool_fill.py a test of every block: this file is that half of the argument.  The CPU twin
takes the parameter with the same range check and does nothing."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pool") / "pool_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "vapor_amd", "csrc"), os.path.join(ROOT, "tools", "pool_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "round: 56 edges and every size to 300 KiB",
    "window: 141 requests, served exactly inside [cap, 2 cap + 1 MiB], smallest block first",
    "limits: 13 give-backs, kept up to 16 GiB / 2 GiB and no further, foreign pointers released",
    "fill: 21 hand-outs, one fill each over the block's capacity before the answer, none when off",
    "sequence: 200 rounds of requests, the blocks and fresh allocations of the rules written out longhand",
    "pool_check: all equal",
])
def test_pool_against_direct_statements_under_sanitizers(output, line):
    assert line in output


def test_the_header_is_part_of_the_library_and_holds_no_hip():
    from vapor_amd import build
    path = os.path.join(build.CSRC, "vapor_pool.h")
    assert path in build.DEPS and path not in build.KERNEL_FILES
    with open(path) as f:
        text = f.read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())        # (the comments name the calls the library hands in)
    assert "hip" not in code and "#include <map>" in code


def test_the_twin_takes_the_parameter_with_the_same_range():
    from oracle import oracle as orc
    lib = ctypes.CDLL(orc.build_twin())
    lib.vapor_init.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.vapor_set_param.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]
    lib.vapor_destroy.argtypes = [ctypes.c_void_p]
    ctx = ctypes.c_void_p()
    assert lib.vapor_init(0, ctypes.byref(ctx)) == 0
    try:
        for v in (-1, 0, 0x5A, 0xFF):
            assert lib.vapor_set_param(ctx, b"pool_fill", v) == 0, v
        for v in (-2, 256, 1 << 40):
            assert lib.vapor_set_param(ctx, b"pool_fill", v) != 0, v
    finally:
        lib.vapor_destroy(ctx)
