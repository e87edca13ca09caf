"""The host side of a clean launch (vapor_amd/csrc/vapor_clean_plan.h: the carving of the clean kernels' dynamic LDS that clean_pair
and the host's byte counts both read, the residency search and its choice of layout, the compiled width of a value range, who cuts
the served pairs' records, the record slots of a plan, what a blocking run decides from its statistics, the packing of
caller-supplied dot lists) on the host, under the address and undefined-behaviour sanitizers (tools/clean_plan_check.cpp).  The
program holds the header to direct statements - regions ordered, disjoint and inside the allocation, geometry against literals,
decisions against rules written out longhand - and to tests/golden/clean_geom.json.gz: what the geometry's formulas answered at
3 209 points (a seeded sample, and every value range at which the width or the workgroups per CU change) before they moved into
the header.  What the kernels make of these launches is what tests/test_gpu_dot_designs.py and tests/test_gpu_clean_plan.py check."""
import gzip
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("clean_plan")
    exe, geom = str(tmp / "clean_plan_check"), str(tmp / "clean_geom.json")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "clean_geom.json.gz"), "rb") as f, open(geom, "wb") as g:
        g.write(f.read())
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"),
                           os.path.join(ROOT, "tools", "clean_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe, geom], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "layout: 85719 staged and 4096 streamed layouts, regions ordered, disjoint and inside the allocation",
    "geometry: 5 shapes, the measured edge and the smallest allocation equal their literals",
    "fixture: 3209 points equal what the formulas answered before",
    "width: 4096 value ranges",
    "rounds: 360 cases",
    "slots: 2000 cases",
    "post-run: 2000 cases",
    "refusals: 24 calls",
    "lists: 600 cases",
    "clean_plan_check: all equal",
])
def test_clean_plan_against_direct_statements_under_sanitizers(output, line):
    assert line in output
