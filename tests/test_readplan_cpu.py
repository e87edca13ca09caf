"""The plan of a device reader call (vapor_amd/csrc/vapor_readplan.h: the argument and region rules, the staging block, the arena, the
metadata block and the read-back of vapor_bam_chop_device*; the stretches, the arena, the windows' slots and the gathered texts of
vapor_fasta_windows_device) on the host, under the address and undefined-behaviour sanitizers (tools/readplan_check.cpp).  The
program needs neither zlib nor files: spans and stretches are block tables it fills in itself, calls are drawn from fixed seeds,
and the header is held to direct statements of its rules, not to recorded plans - every refusal reason alone and mixed among good
regions, staging and arena ranges aligned, disjoint and in order, the 1.5 GB and 2 GB refusals at their limits, the metadata block
of the four modes with and without de-duplication (and, without, as it was before the option), the read-back against
minimize_pacbio_read_list by brute force, the windows' bytes against an arena laid out from the program's own blocks, the two size
caps, a text buffer one byte short.  Every buffer is a heap allocation of exactly the bytes the header asks for.  The kernels
behind these plans are what tests/test_gpu_bamdev.py, test_gpu_phase.py, test_gpu_haplotag.py, test_gpu_both_ends.py,
test_gpu_dedup.py and test_gpu_bgzf_fasta.py check, and tests/test_gpu_reader_plan.py the refusals on the real entries."""
import pytest

import readplan_program


@pytest.fixture(scope="module")
def output():
    return readplan_program.output()


@pytest.mark.parametrize("line", [
    "statuses: 13 reasons, each alone among good regions in 800 calls and mixed in 3000 calls with 3940 refused regions, equal the rule",
    "staging and arena: 4000 calls, 17564 spans, 44013 blocks lie where the rule says",
    "metadata: 4 modes with and without de-duplication, 500 to 500 calls each: aligned, disjoint, inputs one prefix, the read-back range what collect reads",
    "limits: 1.5 GB of blocks and 2 GB of block data pass, 64 bytes and one byte more are refused",
    "collect: 1500 calls, 5840 regions (977 full slots, 991 device statuses, 250 bad unions), 470379 entries equal minimize_pacbio_read_list by brute force",
    "fasta stretches: 1500 calls, 4033 stretches: every window in one, ascending, disjoint, together by the chain of shared blocks",
    "fasta windows: 15622 windows spell their 6804839 bytes from their blocks, 3350 refused (529 stretches cut), 1428 buffers one byte short",
    "fasta answers: 1500 calls gathered back to back",
    "fasta caps: a stretch past STAGE_CAP or ARENA_CAP has no room, for all its windows and only those",
    "readplan_check: all equal",
])
def test_reader_plans_against_direct_statements_of_the_rules_under_sanitizers(output, line):
    assert line in output
