"""The window-aligned join task table of the host planner (vapor_amd/csrc/vapor_planner.h: plan_launch_aligned, made beside the
cost-balanced one when PlanParams::align_tasks is set; the library's parameter "join_align") on the host, under the address and
undefined-behaviour sanitizers (tools/planner_align_check.cpp).  The program draws its worlds from fixed seeds and holds the
table to direct statements of its rule, not to recorded plans: every joined pair in exactly one task, one allele a task, at most
reads_per_task reads, the launches of the balanced table over the same pair list; by enumeration on small launches: every group
cut as cheaply as its number of ranges allows, no smaller bound within join_tasks, no range the bound does not need; `tasks` and
`launches` byte for byte those of default PlanParams; and by design worlds of more windows than join_tasks, groups above
reads_per_task, groups of one read, join_tasks = 1.  What the kernels make of the table is tests/test_gpu_join_align.py's."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("planner_align") / "planner_align_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"),
                           os.path.join(ROOT, "tools", "planner_align_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "balanced table: 2200 cases byte for byte those of default PlanParams",
    "aligned tasks: 6549 launches",
    "enumerated: 5588 launches, every group cut as cheaply as its ranges allow",
    "by design: 1872 launches of more groups than join_tasks, 3142 groups above reads_per_task, 9744 groups of one read, 1151 launches with join_tasks 1",
    "planner_align_check: all hold",
])
def test_aligned_tasks_against_direct_statements_of_the_rule_under_sanitizers(output, line):
    assert line in output
