"""The host planner (vapor_amd/csrc/vapor_planner.h: the share groups of a sequence set, the plan of a list of pairs - statuses,
shared joins and their remap tables, launches and cost-balanced join tasks - and the clean order) on the host, under the address
and undefined-behaviour sanitizers (tools/planner_check.cpp).  The program draws its sequence sets and pairs from fixed seeds and
holds the planner to direct statements of its rules, not to recorded plans: the statuses, every pair joined once or served, the
tasks of every launch, the dearest task against every contiguous partition of a small launch, the remap tables against the texts
the segment lists spell (inversions, tandem duplications, insertions, upper-cased twins), the structures that are not shared, the
clean order.  What the kernels make of these plans is what tests/test_gpu_derived.py and tests/test_gpu_parity.py check."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("planner") / "planner_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"),
                           os.path.join(ROOT, "tools", "planner_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "statuses: 3000 cases equal the rule",
    "scored once: 3000 cases",
    "tasks: 3000 cases",
    "partition: 3129 launches as cheap as the best of their partitions",
    "tables: 3000 cases",
    "declined: 227 fourth members, 1042 third copies, 1035 of more than 48 intervals, 1507 long hidden sequences are not shared",
    "clean order: 3000 cases",
    "planner_check: all equal",
])
def test_plans_against_direct_statements_of_the_rules_under_sanitizers(output, line):
    assert line in output
