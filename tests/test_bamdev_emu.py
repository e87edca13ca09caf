"""The DEFLATE decoder of bgzf_inflate_kernel (vapor_amd/csrc/vapor_bamdev.h) compiled for the host - one "lane" doing the
wavefront's loops in order - against zlib (tools/bamdev_emu.cpp: streams of every level and strategy, stored / fixed / dynamic
blocks, several blocks in a stream, sizes 0 .. 65 536, the CRC-32 by slices, damaged and truncated streams), under the address
and undefined-behaviour sanitizers.  What this cannot see - the wavefront's memory ordering, the kernels around the decoder - is
what tests/test_gpu_bamdev.py checks on the GPU.  Then the same decoder, and the host's (vapor_inflate::inflate_raw), on legal
DEFLATE that zlib's encoder never writes: the families of tests/deflate_forms.py, every stream confirmed by zlib's inflate."""
import collections
import os
import re
import subprocess

import pytest

from conftest import ROOT


def _build(llb, tmp_path):
    exe = str(tmp_path / "bamdev_emu")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DVBD_EMU", "-DVBD_LLB=" + llb,
                           "-I" + os.path.join(ROOT, "vapor_amd", "csrc"), os.path.join(ROOT, "tools", "bamdev_emu.cpp"), "-lz", "-o", exe])
    return exe


@pytest.mark.parametrize("llb", ["9", "10"])
def test_decoder_core_against_zlib_under_sanitizers(llb, tmp_path):
    exe = _build(llb, tmp_path)
    r = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert "streams equal zlib's bytes and CRC-32 (0 refused for table size)" in r.stdout


@pytest.fixture(scope="module")
def form_records(tmp_path_factory):
    import deflate_forms
    items = deflate_forms.all_forms(1)
    path = str(tmp_path_factory.mktemp("forms") / "forms.rec")
    deflate_forms.write_records(path, items)
    return path, [fam for fam, _stream, _data in items]


@pytest.mark.parametrize("llb", ["9", "10"])
def test_decoder_core_on_legal_deflate_that_zlib_never_writes(llb, tmp_path, form_records):
    """About 3 000 streams of tests/deflate_forms.py - 15-bit codes with the widest extra fields at every alignment of the bit
    buffer, the widest header at every offset of the LDS copy of the stream, 63 / 64 / 65 matches in front of a header, stored
    blocks of every placing, blocks that end at byte 65 536, mixes of all of it - through the decoder core and the host's decoder:
    every one BLK_OK with zlib's bytes, none refused for table size (a complete code cannot exceed the bound the tables are cut
    for), wrong-CRC variants BLK_CRC, ISIZE +- 1 variants refused.  (With `n < 48` as the fast loop's refill rule, 289 of
    these streams - all of the long_codes family - ended as BLK_BAD_STREAM at 9 first-level bits, and 295 at 10: 294 long_codes,
    one mixed.)"""
    path, families = form_records
    assert len(families) >= 3000 and set(families) == {"long_codes", "headers", "match_queue", "stored", "size_edge", "mixed"}
    exe = _build(llb, tmp_path)
    r = subprocess.run([exe, "--forms", path], capture_output=True, text=True, timeout=600)
    failed = collections.Counter(families[int(k)] for k in re.findall(r"FAIL record (\d+)", r.stderr))
    m = re.search(r"bamdev_emu forms: (\d+) streams, (\d+) equal, (\d+) refused \((\d+) refused for table size\), (\d+) wrong bytes, "
                  r"(\d+) host decoder failures, (\d+) variant failures", r.stdout)
    assert m, (r.stdout[-1000:], r.stderr[-2000:])
    n, equal, refused, tables, wrong, host, variants = map(int, m.groups())
    print("llb %s: %d streams, %d equal, %d refused (%d for table size), %d wrong, %d host failures, %d variant failures; failures by family %s"
          % (llb, n, equal, refused, tables, wrong, host, variants, dict(failed)))
    assert n == len(families)
    assert tables == 0, "valid streams refused for table size"
    assert host == 0, r.stderr[-2000:]
    assert (equal, refused, wrong, variants) == (n, 0, 0, 0), (dict(failed), r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
