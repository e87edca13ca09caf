"""tools/readplan_check.cpp as a program of its own, built and run once per pytest process: test_readplan_cpu.py, test_signature_cpu.py,
test_links_cpu.py and test_support_cpu.py each quote lines of the one output.  Built under the address and undefined-behaviour
sanitizers with the strictest of the settings those files had - no recovery from undefined behaviour, leak detection left on - and
held to exit 0 with no sanitizer report."""
import functools
import os
import subprocess
import tempfile

from conftest import ROOT

FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DVBD_EMU",
         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc")]


@functools.lru_cache(maxsize=None)
def output() -> str:
    """The program's stdout."""
    with tempfile.TemporaryDirectory(prefix="readplan_check_") as d:
        exe = os.path.join(d, "readplan_check")
        r = subprocess.run(["g++"] + FLAGS + [os.path.join(ROOT, "tools", "readplan_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    return p.stdout
