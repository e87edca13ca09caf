"""The host side of the explicit-dot routes (vapor_amd/csrc/vapor_dots_plan.h: what a call and a pair of vapor_wide_batch,
vapor_anyk_batch and vapor_clean_hits_wide are refused for and in which order, a pair's shape, the wide join's hash table, the any-k
pass with its sort schedule, symbol layout, blocks and edit cut, the passes and the scratch of the cleaning, the three writers of a
statistics record, the capacity protocol and the bound on a pair's dots) on the host, under the address and undefined-behaviour
sanitizers (tools/dots_plan_check.cpp).  The program holds the header to direct statements - refusals against the order written out,
sizes against literals and inequalities, the sort schedule against the bitonic network stage by stage - and to
tests/golden/dots_plan.json.gz: what the formulas answered at 3 800 seeded points while vapor_hip.hip still computed them between
its launches (tools/dots_plan_fixture.cpp).  What the kernels make of these launches is what tests/test_gpu_wide.py,
tests/test_gpu_anyk*.py and tests/test_gpu_dots_plan.py check."""
import gzip
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dots_plan")
    exe, points = str(tmp / "dots_plan_check"), str(tmp / "dots_plan.json")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "dots_plan.json.gz"), "rb") as f, open(points, "wb") as g:
        g.write(f.read())
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"),
                           os.path.join(ROOT, "tools", "dots_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe, points], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "refusals: 101 pairs in order, 19 calls",
    "hash table: 10001 sizes",
    "sort schedule: 13 sizes are the bitonic network, 10 kb in 28 launches",
    "symbol layout: 1448402 layouts, strings disjoint, on 16 bytes, 16 bytes behind each",
    "edit cut: 1100 cuts tile their allele, 200 000 symbols in 3 launches",
    "cleaning: 8 flag values, the scratch at 4 extents",
    "records: refused, overflowed and folded equal their literals",
    "capacity protocol: 3 capacities",
    "dot bound: 5 values",
    "fixture: 3800 points equal what the formulas answered before",
    "dots_plan_check: all equal",
])
def test_dots_plan_against_direct_statements_under_sanitizers(output, line):
    assert line in output
