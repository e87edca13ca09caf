"""The host plan of a vapor_seqset_create* call (vapor_amd/csrc/vapor_seqset_plan.h: the refusals of the four entries in their
order, where every literal, derived and hidden sequence lies in the planes, the staging buffer's tables and what is written into
them, the threaded staging, what follows the counts the kernels send back) on the host, under the address and undefined-behaviour
sanitizers (tools/seqset_check.cpp).  The program draws its sets from fixed seeds and holds the plan to direct statements, not to
recorded output: every refusal's code and text, and among two faults the one a plain transcription of the entries' checks meets
first; the size limits on both sides with made-up lengths and no bytes; chunk ranges, pads and tail of the planes; the staging
image table by table, the derived tables spelt through the parents' first chunks, its size by the formula written out, a
device-held literal pointing into a page that cannot be read; the slices of the threaded staging against the image one thread
makes, a second time under the thread sanitizer with the threads running.  What the kernels make of these tables is what
tests/test_gpu_planes.py and tests/test_gpu_seqset_plan.py check."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build(tmp, name, sanitize):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + sanitize +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"), "-I" + os.path.join(ROOT, "tools"),
                           os.path.join(ROOT, "tools", "seqset_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("seqset"), "seqset_check", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "refusals: 220 calls with one fault say what the fault is, 2898 with two what the entries' own order meets first",
    "limits: 16 calls of made-up lengths on both sides of every limit",
    "layout: 3000 sets",
    "image: 3000 sets",
    "after the counts: 3000 sets",
    "slices: 200 sets staged by 1, 2, 3, 5, 12, 13 and 64 threads equal the single thread's image",
    "seqset_check: all equal",
])
def test_the_plan_against_direct_statements_under_sanitizers(output, line):
    assert line in output


def test_threaded_staging_under_the_thread_sanitizer(tmp_path):
    exe = _build(tmp_path, "seqset_check_tsan", ["-fsanitize=thread"])
    r = subprocess.run([exe, "slices"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "slices: 60 sets staged by 1, 2, 3, 5, 12, 13 and 64 threads equal the single thread's image" in r.stdout
    assert "seqset_check: all equal" in r.stdout
