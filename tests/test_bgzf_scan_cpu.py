"""The one statement of what a BGZF block is (vapor_amd/csrc/vapor_bgzf.h: the header parser, the block walk, the span scan of
vapor_bam_chop_device* and the stretch scan of vapor_fasta_windows_device) on the host, under the address and undefined-behaviour
sanitizers (tools/bgzf_scan_check.cpp).  The program writes its files with zlib and keeps every block's offsets, sizes and CRC, so
the oracle is zlib plus its own table: well-formed files with foreign subfields before and behind BC and empty blocks, a file cut
at every length, each refusal, random chunks against a direct statement of the span rule, and a span of 65 537 blocks of 64 KB -
more than 4 GB of data, which a 32-bit total wrapped - against one of 32 767.  Every buffer is a heap allocation of exactly the
bytes available.  The kernels behind the scans are what tests/test_gpu_bamdev.py and tests/test_gpu_bgzf_fasta.py check."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bgzf") / "bgzf_scan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DVBD_EMU",
                           "-I" + os.path.join(ROOT, "vapor_amd", "csrc"), os.path.join(ROOT, "tools", "bgzf_scan_check.cpp"), "-lz", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "well-formed: 600 blocks equal the writer's table",
    "truncation: a three-block file cut at every length gives its whole blocks, then more bytes",
    "refusals: 12 kinds refused by the parser, the walk, the span scan and the stretch scan",
    "spans: 3000 chunks equal the rule",
    "wrap: 65537 blocks of 64 KB total 4295032832 bytes and are refused, 32767 are not",
    "stretches: 288 stretches equal the writer's table",
    "bgzf_scan_check: all equal",
])
def test_parser_walk_and_scans_against_the_writers_table_under_sanitizers(output, line):
    assert line in output
