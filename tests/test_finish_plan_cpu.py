"""The host side of the finishing and grid calls (vapor_amd/csrc/vapor_finish_plan.h: what vapor_plan_set_reads, vapor_plan_set_grid
and vapor_grid_pick refuse and in which order, the two upload images with their tables, the sizes of the blocks behind them, which
path a vapor_plan_run_loci takes, when the host's statuses go up again and when a run is repeated, what an asynchronous step is
refused for) on the host, under the address and undefined-behaviour sanitizers (tools/finish_plan_check.cpp).  The program holds
the header to direct statements - refusals alone and in combination against the order written out, the edges of a group's size and
of the winners' slots, the images against disjointness, bounds and alignment, locus_first against a count, the run's decisions
against a literal table - and to tests/golden/finish_plan.json.gz: what the checks and sizes answered at 3 800 seeded points while
vapor_hip.hip still computed them between its launches (tools/finish_plan_fixture.cpp).  What the kernels make of these launches
is what tests/test_gpu_finish.py, tests/test_gpu_refine.py and tests/test_gpu_finish_plan.py check."""
import gzip
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("finish_plan")
    exe, points = str(tmp / "finish_plan_check"), str(tmp / "finish_plan.json")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "finish_plan.json.gz"), "rb") as f, open(points, "wb") as g:
        g.write(f.read())
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"),
                           os.path.join(ROOT, "tools", "finish_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe, points], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


LINES = [
    "read refusals: 345 tables, the first rule in order and the first read win",
    "grid refusals: 38 grids, the first rule in order and the first group win",
    "edges: 1 and 128 candidates, 0 and 129, counts off by one, INT32_MAX slots and one more, nothing at all",
    "images: 13266 shapes tile on 8 bytes, 300 filled, locus_first counts the reads in front",
    "run decisions: 16 states equal their table, 7 refused asynchronous steps in order",
    "fixture: 3800 points equal what the calls answered before, 1908 of them refusals",
    "finish_plan_check: all equal",
]


@pytest.mark.parametrize("line", LINES)
def test_finish_plan_against_direct_statements_under_sanitizers(output, line):
    assert line in output.splitlines()


def test_every_line_of_the_output_is_asserted(output):
    assert output.splitlines() == LINES
