"""Haplotags from a phased VCF (`--phase-vcf`, vapor_amd/phase.py) without a GPU: the vote rule in the three
host readers against one hand-written table, the VCF reader, and `vapor bed | vcf --phase-vcf` on an untagged world against
`--phased` on the same world with its true tags - on the tests' stand-in engine and on the CPU twin of the C ABI, which has no
haplotagging device reader, so that the array route takes the host readers there."""
import ctypes
import gzip
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from fake_engine import FakeEngine

from vapor_amd import bamio, cli, phase, pipeline, seqio, synth
from vapor_amd import _lib as L


@pytest.fixture()
def twin_eng(oracle):
    """The real Engine on the CPU twin of the C ABI (test infrastructure), as pipeline's engine."""
    from vapor_amd.engine import Engine
    saved = L._lib
    L._lib = L.bind(ctypes.CDLL(oracle.build_twin()))
    e = Engine(0)
    pipeline.set_engine(e)
    yield e
    pipeline.set_engine(None)
    seqio.set_backend(None)
    e.close()
    L._lib = saved


# ------------------------------------------------------------------------------------------
# the vote of a record: three readers, one table written by hand
# ------------------------------------------------------------------------------------------
REACH = 100000
# (name, POS, CIGAR, SEQ, sites (pos, a1, a2, ps), expected (hap, ps), region start or None for POS)
ROWS = [
    ("first_base_even", 100, "8M", "ACGTACGT", [(100, "A", "C", 5)], (1, 5), None),
    ("last_base_odd", 100, "8M", "ACGTACGT", [(107, "G", "T", 5)], (2, 5), None),
    ("behind_the_end", 100, "8M", "ACGTACGT", [(108, "A", "C", 5)], (0, None), None),
    ("before_the_start", 100, "8M", "ACGTACGT", [(99, "A", "C", 5)], (0, None), None),
    ("m_last_and_next_m_first_beside_i", 100, "4M2I4M", "ACGTGGTTCA", [(103, "T", "A", 7), (104, "T", "A", 7)], (1, 7), None),
    ("inside_d", 100, "4M3D4M", "ACGTACGT", [(105, "A", "C", 7)], (0, None), None),
    ("inside_d_and_behind_it", 100, "4M3D4M", "ACGTACGT", [(105, "A", "C", 7), (107, "C", "A", 7)], (2, 7), None),
    ("inside_n_and_behind_it", 100, "4M10N4M", "ACGTACGT", [(108, "A", "C", 3), (114, "A", "G", 3)], (1, 3), None),
    ("leading_s", 100, "3S5M", "TTTACGTA", [(100, "A", "T", 2)], (1, 2), None),
    ("leading_h", 100, "5H6M", "ACGTAC", [(100, "C", "A", 2)], (2, 2), None),
    ("eq_and_x", 100, "3=2X3=", "ACGTACGT", [(103, "T", "C", 9), (106, "G", "C", 9)], (1, 9), None),
    ("read_base_n", 100, "8M", "ACGNACGT", [(103, "A", "C", 1)], (0, None), None),
    ("read_base_eq", 100, "8M", "AC=TACGT", [(102, "A", "C", 1)], (0, None), None),
    ("third_letter", 100, "8M", "ACGTACGT", [(103, "A", "C", 1)], (0, None), None),
    ("gt_0|1_reads_ref", 100, "8M", "ACGTACGT", [(101, "C", "G", 4)], (1, 4), None),
    ("gt_1|2_reads_second_alt", 100, "8M", "ATGTACGT", [(101, "G", "T", 4)], (2, 4), None),
    ("lowercase_read", 100, "8M", "acgtacgt", [(101, "C", "G", 4)], (1, 4), None),
    ("vote_tie", 100, "8M", "ACGTACGT", [(100, "A", "C", 5), (101, "G", "C", 5)], (0, None), None),
    ("two_ps_more_votes_win", 100, "8M", "ACGTACGT", [(100, "A", "C", 3), (101, "A", "C", 9), (102, "A", "G", 9)], (2, 9), None),
    ("two_ps_equal_votes_smaller_ps", 100, "8M", "ACGTACGT", [(100, "A", "C", 9), (101, "A", "C", 3)], (2, 3), None),
    ("winner_ties_inside", 100, "8M", "ACGTACGT", [(100, "A", "C", 3), (101, "A", "C", 3), (102, "G", "A", 9)], (0, None), None),
    ("ps_0", 100, "8M", "ACGTACGT", [(100, "A", "C", 0)], (1, 0), None),
    ("ps_2^32-1", 100, "8M", "ACGTACGT", [(100, "A", "C", 4294967295)], (1, 4294967295), None),
    # region start 101005: the site at start - PHASE_REACH = 1005 is counted (C: haplotype 2), the one at 1004 (A: haplotype 1,
    # which would make a tie) is not
    ("reach", 1000, "10M100000D30M", "ACGTACGTAC" + "G" * 30, [(1004, "A", "T", 6), (1005, "T", "C", 6)], (2, 6), 101005),
    ("no_sites", 100, "8M", "ACGTACGT", [], (0, None), None),
]
CONTIG_LEN = 200000


def table_world():
    """The table as BAM records (one contig a row), its sites, and the chop region of every row - the record of a row is the one
    read its region keeps."""
    refs, recs, site_rows, regions = [], [], [], []
    for t, (name, pos, cigar, seq, sites, _exp, start) in enumerate(ROWS):
        chrom = "t%d" % t
        refs.append((chrom, CONTIG_LEN))
        recs.append((name, t, pos - 1, cigar, seq))
        site_rows += [(chrom, p, a1, a2, ps) for p, a1, a2, ps in sites]
        start = pos if start is None else start
        regions.append((chrom, start, start + 10 if name == "reach" else start + 4, 20))
    return refs, recs, phase.Sites.from_rows(site_rows), regions


def test_the_statement_on_the_hand_written_table():
    assert phase.PHASE_REACH == REACH
    _refs, _recs, sites, regions = table_world()
    for (name, pos, cigar, seq, rows, exp, _start), (chrom, start, end, _fl) in zip(ROWS, regions):
        locus = sites.rows(chrom, start, end)
        if name == "reach":
            assert locus == [(1005, "T", "C", 6)]                      # (the slice is the rule's: one base further out is not in it)
            assert sites.rows(chrom, start - 1, end) == rows
        else:
            assert locus == rows, name
        assert phase.haplotag(pos, cigar, seq, locus) == exp, name
        # the packed form of the operations (what bamio hands over) walks the same
        packed = np.asarray([(n << 4) | "MIDNSHP=X".index(op) for n, op in phase.cigar_ops(cigar)], dtype=np.uint32)
        assert phase.haplotag(pos, packed, seq, locus) == exp, name
    # a site beyond the far end of the reach
    s2 = phase.Sites.from_rows([("c", 1000 + REACH, "A", "C", 1), ("c", 1001 + REACH, "A", "C", 1)])
    assert [r[0] for r in s2.rows("c", 900, 1000)] == [1000 + REACH] and s2.rows("x", 900, 1000) == []


def test_the_file_readers_agree_with_the_table(tmp_path, twin_eng, monkeypatch):
    """bamio's Python reader and vapor_bam_chop_haplotag (through the twin, which compiles vapor_bam.cpp in) on a BAM written
    from the rows; the records carry contradicting HP / PS tags, which are not read."""
    refs, recs, sites, regions = table_world()
    recs = [r + ({"HP": 1 if ROWS[t][5][0] == 2 else 2, "PS": 77},) for t, r in enumerate(recs)]
    bam = str(tmp_path / "table.bam")
    bamio.write_bam(bam, refs, recs, block_size=4096)
    assert hasattr(L.load(), "vapor_bam_chop_haplotag")
    be = seqio.InProcessBam()
    for (name, _pos, _cigar, seq, _rows, exp, _s), (chrom, start, end, fl) in zip(ROWS, regions):
        py = be.chop_python(bam, chrom, start, end, fl, tagged=True, sites=sites)
        monkeypatch.delenv("VAPOR_BAM_NATIVE", raising=False)
        nat = be.chop(bam, chrom, start, end, fl, tagged=True, sites=sites)
        assert len(py) == 1 and py == nat, name
        assert (py[0][2], tuple(py[0][3:])) == (name, exp), name
        # without sites the same call reads the tags; with the sites on the backend it does not
        assert tuple(be.chop(bam, chrom, start, end, fl, tagged=True)[0][3:]) == (1 if exp[0] == 2 else 2, 77)
        be.phase_sites = sites
        assert be.chop(bam, chrom, start, end, fl, tagged=True) == nat
        monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
        assert be.chop(bam, chrom, start, end, fl, tagged=True) == nat
        monkeypatch.delenv("VAPOR_BAM_NATIVE")
        be.phase_sites = None
        assert be.chop(bam, chrom, start, end, fl) == [r[:3] for r in nat]          # (untagged: the entries of before)
    # SAM text (MemorySamtools, and a backend that answers in text alone)
    w = synth.SynthWorld()
    for (name, pos, cigar, seq, _rows, _exp, _s), (chrom, _a, _b, _f) in zip(ROWS, regions):
        w.contigs[chrom] = "A" * 16
        w.reads[chrom] = [synth.SamRecord(name, chrom, pos, cigar, seq, 200000, {"HP": 1, "PS": 77})]
    mem = seqio.MemorySamtools(w)

    class TextOnly:
        view_lines = mem.view_lines
    for (name, _pos, _cigar, _seq, _rows, exp, _s), (chrom, start, end, fl) in zip(ROWS, regions):
        got = mem.chop("x.bam", chrom, start, end, fl, tagged=True, sites=sites)
        assert len(got) == 1 and tuple(got[0][3:]) == exp, name
        monkeypatch.setenv("VAPOR_MEMORY_CHOP", "records")
        assert mem.chop("x.bam", chrom, start, end, fl, tagged=True, sites=sites) == got
        monkeypatch.delenv("VAPOR_MEMORY_CHOP")
        seqio.set_backend(TextOnly())
        assert seqio.chop_pacbio_read_by_pos("x.bam", chrom, start, end, fl, True, sites=sites) == got
        seqio.set_backend(None)
    # the array form of both backends: chop_many(groups=True) with the sites
    chroms = [r[0] for r in regions]
    args = (chroms, [r[1] for r in regions], [r[2] for r in regions], [r[3] for r in regions])
    for backend, src in ((be, bam), (mem, "x.bam")):
        kf, _addr, _q0, _miss, status, _keep, member, pset, tagged = backend.chop_many(src, *args, groups=True, sites=sites)
        assert np.diff(kf).tolist() == [1] * len(ROWS) and not status.any()
        for t, row in enumerate(ROWS):
            hap, ps = row[5]
            assert (int(tagged[t]), int(pset[t])) == ((1, ps) if hap else (0, phase.PS_NONE)), row[0]
            assert int(member[t]) & 7 == (1 | (2 << (hap - 1)) if hap else 1), row[0]
    # the native reader refuses sites that are out of order
    lib = L.load()
    tl = be._open(bam)._take_handle(lib)
    pos = np.asarray([5, 5], dtype=np.int64)
    a = np.asarray([1, 1], dtype=np.uint8)
    n = ctypes.c_int32(0)
    bf = tl["buf"]
    rc = lib.vapor_bam_chop_haplotag(tl["native"], 0, 100, 104, 20, 0, None, bf["seq"].ctypes.data, bf["seq"].size,
                                     ctypes.cast(bf["names"], ctypes.c_void_p), len(bf["names"]), bf["meta"].ctypes.data, 8, ctypes.byref(n),
                                     bf["need"].ctypes.data, 2, pos.ctypes.data, a.ctypes.data, a.ctypes.data, pos.ctypes.data)
    assert rc == L.E_ARG and b"position order" in lib.vapor_bam_last_error()


# ------------------------------------------------------------------------------------------
# the VCF reader
# ------------------------------------------------------------------------------------------
VCF = "\n".join([
    "##fileformat=VCFv4.2",
    "##FORMAT=<ID=PS,Number=1,Type=Integer,Description=\"Phase set\">",
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2",
    "c1\t100\t.\tA\tC\t.\tPASS\t.\tGT:PS\t0|1:7\t1|0:8",                  # a site in both samples
    "c1\t90\t.\tG\tT\t.\tLowQual\t.\tGT:PS\t1|0:7\t0/1:8",                # out of order; FILTER ignored; S2 not phased
    "c1\t110\t.\tAT\tA\t.\tPASS\t.\tGT:PS\t0|1:7\t0|1:8",                 # a deletion
    "c1\t120\t.\tA\tAT\t.\tPASS\t.\tGT:PS\t0|1:7\t0|1:8",                 # an insertion
    "c1\t130\t.\tAC\tGT\t.\tPASS\t.\tGT:PS\t0|1:7\t0|1:8",                # an MNV
    "c1\t140\t.\tA\t<DEL>\t.\tPASS\t.\tGT:PS\t0|1:7\t0|1:8",              # a symbolic allele
    "c1\t150\t.\tA\tC\t.\tPASS\t.\tGT:PS\t0/1:7\t1|1:8",                  # unphased; homozygous
    "c1\t160\t.\tA\tC\t.\tPASS\t.\tGT:PS\t.|.:7\t.:8",                    # missing
    "c1\t170\t.\tA\tC,G\t.\tPASS\t.\tGT:PS\t1|2:7\t2|0:8",                # two ALT alleles
    "c1\t170\t.\tA\tT\t.\tPASS\t.\tGT:PS\t0|1:7\t0|1:8",                  # a second record at the position: dropped
    "c1\t180\t.\ta\tc\t.\tPASS\t.\tGT\t1|0\t0|1",                         # lowercase; no PS key
    "c1\t190\t.\tA\tC\t.\tPASS\t.\tGT:PS\t0|1:.\t0|1:9",                  # PS '.'
    "c1\t200\t.\tA\tC,AT\t.\tPASS\t.\tGT:PS\t1|2:7\t0|1:8",               # S1 carries the insertion: no site there; S2 is one
    "zz\t50\t.\tA\tC\t.\tPASS\t.\tGT:PS\t0|1:3\t0|1:3",                   # a contig the BAM does not have
    "c2\t10\t.\tT\tG\t.\tPASS\t.\tPS:GT\t4294967295:1|0\t5:0|1",          # the keys in another order
]) + "\n"


def test_read_sites(tmp_path):
    plain = tmp_path / "p.vcf"
    plain.write_text(VCF)
    gz = tmp_path / "p.vcf.gz"
    gz.write_bytes(gzip.compress(VCF.encode()))
    bgz = tmp_path / "b.vcf.gz"
    raw = VCF.encode()
    bgz.write_bytes(bamio._bgzf_block(raw[:300]) + bamio._bgzf_block(raw[300:]) + bamio._BGZF_EOF)
    want1 = {"c1": [(90, "T", "G", 7), (100, "A", "C", 7), (170, "C", "G", 7), (180, "C", "A", 0), (190, "A", "C", 0)],
             "c2": [(10, "G", "T", 4294967295)], "zz": [(50, "A", "C", 3)]}
    want2 = {"c1": [(100, "C", "A", 8), (170, "G", "A", 8), (180, "A", "C", 0), (190, "A", "C", 9), (200, "A", "C", 8)],
             "c2": [(10, "T", "G", 5)], "zz": [(50, "A", "C", 3)]}
    for path in (plain, gz, bgz):
        for sample, want in ((None, want1), ("S1", want1), ("S2", want2)):
            s = phase.read_sites(str(path), sample)
            assert {c: s.rows(c, 1, 1000) for c in s.by_contig} == want, (path, sample)
        s = phase.read_sites(str(path), contigs={"c1", "c2"})
        assert set(s.by_contig) == {"c1", "c2"} and len(s) == 6
    with pytest.raises(ValueError, match="no sample 'S3'"):
        phase.read_sites(str(plain), "S3")
    bare = tmp_path / "bare.vcf"
    bare.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nc1\t100\t.\tA\tC\t.\tPASS\t.\n")
    with pytest.raises(ValueError, match="no sample column"):
        phase.read_sites(str(bare))
    # the device form of a region's slice: 8-byte entries, the phase sets as indices into the region's ascending table
    sf, ent, pf, psv = phase.device_site_tables(phase.read_sites(str(plain)), ["c1", "nope", "c2"], [100, 5, 5], [120, 9, 9])
    assert ent.dtype.itemsize == 8 and sf.tolist() == [0, 5, 5, 6] and pf.tolist() == [0, 2, 2, 3] and psv.tolist() == [0, 7, 4294967295]
    assert ent["pos"].tolist() == [90, 100, 170, 180, 190, 10] and ent["idx"].tolist() == [1, 1, 1, 0, 0, 0]
    assert ent["a1"].tolist() == [8, 1, 2, 2, 1, 4] and ent["a2"].tolist() == [4, 2, 4, 1, 2, 8]
    many = phase.Sites.from_rows([("c", 10 + i, "A", "C", i) for i in range(64)] + [("d", 10 + i, "A", "C", i) for i in range(65)])
    sf, ent, pf, psv = phase.device_site_tables(many, ["c", "d"], [5, 5], [73, 74])
    assert sf.tolist() == [0, 64, 64] and pf.tolist() == [0, 64, 129]        # (65 phase sets: no entries, a table one too long)


def test_option_errors(capsys, tmp_path):
    base = ["--sv-input", "a.bed", "--reference", "r.fa", "--pacbio-input", "x.bam", "--output-path", str(tmp_path / "o"),
            "--output-file", str(tmp_path / "o.vapor")]
    vcf = tmp_path / "p.vcf"
    vcf.write_text(VCF)
    pv = ["--phase-vcf", str(vcf)]
    bare = tmp_path / "bare.vcf"
    bare.write_text("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    cases = [("bed", pv + ["--refine", "20"], "--phased and --refine"), ("vcf", pv + ["--both-ends"], "--both-ends and --phased"),
             ("svelter", pv, "--phased applies to"), ("ins", pv, "--phased applies to"),
             ("bed", ["--phase-sample", "S1"], "--phase-sample names a sample of --phase-vcf"),
             ("bed", ["--phased", "--phase-sample", "S1"], "--phase-sample names a sample of --phase-vcf"),
             ("bed", pv + ["--phase-sample", "S3"], "no sample 'S3'"), ("bed", ["--phase-vcf", str(bare)], "no sample column"),
             ("vcf", ["--phase-vcf", str(tmp_path / "missing.vcf")], "--phase-vcf")]
    for mode, more, text in cases:
        with pytest.raises(SystemExit) as e:
            cli.main([mode] + base + more)
        assert e.value.code == 2, (mode, more)
        assert text in capsys.readouterr().err, (mode, more)
    a = cli.build_parser().parse_args(base + pv + ["--phase-sample", "S2"])
    assert a.phase_vcf == str(vcf) and a.phase_sample == "S2" and not a.phased
    assert cli.build_parser().parse_args(base).phase_vcf is None


def test_entry_points_are_declared(twin_eng):
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    for name in ("vapor_bam_chop_haplotag", "vapor_bam_chop_device_haplotag"):
        assert re.search(r"\bint %s\(" % name, h) and name in L.EXPORTS
        assert "SF:339-354" in h[h.index("int " + name) - 2400:h.index("int " + name)]
    assert "vapor_bam_chop_device_haplotag" in L.OPTIONAL_EXPORTS and "vapor_bam_chop_haplotag" not in L.OPTIONAL_EXPORTS
    assert L.ABI_VERSION == 3 and "#define VAPOR_PHASE_REACH %d" % phase.PHASE_REACH in h
    assert "#define VAPOR_PHASE_SETS_DEVICE %d" % phase.PHASE_SETS_DEVICE in h
    args = [None] * 23
    args[2] = args[9] = 0
    assert L.load().vapor_bam_chop_device_haplotag(*args) == L.E_ARG                 # (the twin's stub refuses every call)
    with pytest.raises(NotImplementedError):
        twin_eng.bam_chop_device(None, [], [], [], [], [0], [], tagged=True, sites=phase.device_site_tables(None, [], [], []))


# ------------------------------------------------------------------------------------------
# the test world and the truth oracle
# ------------------------------------------------------------------------------------------
SEED = 3


def truth_world(seed=SEED):
    """The 12-locus world of 30 reads a locus with phased SNVs planted, untagged; its sites."""
    w = synth.make_world(seed, 12, ("DEL", "INV", "INS", "TANDUP"), n_reads=30, read_len=3000, span_range=(200, 1200))
    return w, synth.snv_world(w, seed + 100)


def test_snv_world_draws_as_documented_and_every_read_gets_its_haplotype():
    w0 = synth.make_world(SEED, 12, ("DEL", "INV", "INS", "TANDUP"), n_reads=30, read_len=3000, span_range=(200, 1200))
    before = {c: [(r.qname, r.pos, r.cigar, r.seq) for r in rs] for c, rs in w0.reads.items()}
    w, sites = truth_world()
    assert list(sites) == [l.chrom for l in w.loci] and w.contigs == w0.contigs
    changed, gts = 0, set()
    for l in w.loci:
        rows = sites[l.chrom]
        pos = [r[0] for r in rows]
        assert pos == sorted(set(pos)) and pos[0] >= 2 and pos[-1] <= l.start
        assert all(25 <= b - a <= 55 for a, b in zip(pos, pos[1:]))
        ref = w.contigs[l.chrom]
        assert all(ref[p - 1] == r and alt != r and alt in "ACGT" and gt in ("1|0", "0|1") for p, r, alt, gt in rows)
        gts |= {gt for _p, _r, _a, gt in rows}
        locus = [(p, alt if gt == "1|0" else r, r if gt == "1|0" else alt, 1) for p, r, alt, gt in rows]
        for rec, (qname, rpos, cigar, seq) in zip(w.reads[l.chrom], before[l.chrom]):
            # names, positions, CIGARs and lengths are make_world's; only bases at sites changed, each from REF to the ALT
            assert (rec.qname, rec.pos, rec.cigar, len(rec.seq)) == (qname, rpos, cigar, len(seq))
            diff = [i for i in range(len(seq)) if seq[i] != rec.seq[i]]
            assert len(diff) <= len(rows)
            changed += len(diff)
            # THE PRECONDITION of the truth tests below: the majority vote gives every read its true haplotype
            assert phase.haplotag(rec.pos, rec.cigar, rec.seq, locus) == (1 if qname.endswith("a") else 2, 1), qname
    assert changed > 360 and gts == {"1|0", "0|1"}
    text = synth.snv_vcf_text(sites, sample="NA1", phase_set=12)
    assert text.splitlines()[4].split("\t")[9] == "NA1" and all(ln.endswith(":12") for ln in text.splitlines()[5:])


def _bed_run(tmp, name, bed_text, extra=(), ref="ref.fa", bam="x.bam"):
    bed = tmp / (name + ".bed")
    bed.write_text(bed_text)
    out = tmp / (name + ".vapor")
    args = ["bed", "--sv-input", str(bed), "--reference", ref, "--pacbio-input", bam, "--output-path", str(tmp / "figs"),
            "--output-file", str(out), "--no-figures"] + list(extra)
    assert cli.main(args) == 0
    return out.read_text()


def _tagged_copy(w, flip=False):
    """The world with its true tags (synth.phase_world, no read left out; flip: every HP the wrong way round, in phase set 99)."""
    import copy
    t = copy.copy(w)
    t.reads = {c: [synth.SamRecord(r.qname, r.rname, r.pos, r.cigar, r.seq, r.ref_span) for r in rs] for c, rs in w.reads.items()}
    synth.phase_world(t, seed=1, untagged=0.0, phase_set=1)
    if flip:
        for rs in t.reads.values():
            for r in rs:
                r.tags = {"HP": 3 - r.tags["HP"], "PS": 99}
    return t


def _check_tables(text, truth, unphased):
    assert text == truth                                                     # text for text
    rows = [ln.split("\t") for ln in text.splitlines()]
    assert [r[:10] for r in rows] == [ln.split("\t") for ln in unphased.splitlines()]
    assert tuple(rows[0][10:]) == phase.COLUMNS and len(rows) == 13
    assert all(r[10] == "1" for r in rows[1:])                                # every locus is phased, in the VCF's phase set


def test_truth_oracle_memory_world(twin_eng, tmp_path, monkeypatch):
    """`vapor bed --phase-vcf` on the untagged world equals `vapor bed --phased` on the same world with its true tags: on the
    array route and with the drivers' route forced."""
    w, sites = truth_world()
    vcf = tmp_path / "snv.vcf"
    vcf.write_text(synth.snv_vcf_text(sites))
    bed = synth.bed_text(w)
    seqio.set_backend(seqio.MemorySamtools(_tagged_copy(w)))
    truth = _bed_run(tmp_path, "truth", bed, ["--phased"])
    be = seqio.MemorySamtools(w)
    seqio.set_backend(be)
    unphased = _bed_run(tmp_path, "un", bed)
    got = _bed_run(tmp_path, "hv", bed, ["--phase-vcf", str(vcf)])
    assert be.phase_sites is None                                             # (the run's sites leave the backend with it)
    _check_tables(got, truth, unphased)
    assert _bed_run(tmp_path, "hv_s", bed, ["--phase-vcf", str(vcf), "--phase-sample", "S1"]) == truth
    monkeypatch.setenv("VAPOR_FAST_PATH", "0")
    assert _bed_run(tmp_path, "hv_drv", bed, ["--phase-vcf", str(vcf)]) == truth
    monkeypatch.delenv("VAPOR_FAST_PATH")
    # the reads carry no tag: --phased alone finds nothing to phase
    rows0 = [ln.split("\t") for ln in _bed_run(tmp_path, "ph0", bed, ["--phased"]).splitlines()]
    assert all(r[10:] == ["."] * 9 for r in rows0[1:])
    # a VCF in another phase set, gzipped: the same table but for the VaPoR_PS column
    gz = tmp_path / "snv7.vcf.gz"
    gz.write_bytes(gzip.compress(synth.snv_vcf_text(sites, phase_set=7).encode()))
    got7 = [ln.split("\t") for ln in _bed_run(tmp_path, "hv7", bed, ["--phase-vcf", str(gz)]).splitlines()]
    want = [ln.split("\t") for ln in truth.splitlines()]
    assert [r[:10] + r[11:] for r in got7] == [r[:10] + r[11:] for r in want] and {r[10] for r in got7[1:]} == {"7"}


def test_truth_oracle_from_files_with_the_host_readers(twin_eng, tmp_path, monkeypatch):
    """The same from FASTA / BAM files: vapor_bam_chop_haplotag behind the array route (the twin has no device reader), the
    drivers' route, and bamio's Python reader; and a BAM whose tags contradict the VCF gives the VCF's answer."""
    w, sites = truth_world()
    vcf = tmp_path / "snv.vcf"
    vcf.write_text(synth.snv_vcf_text(sites))
    bed = synth.bed_text(w)
    dirs = {}
    for name, world in (("plain", w), ("truth", _tagged_copy(w)), ("flipped", _tagged_copy(w, flip=True))):
        d = tmp_path / name
        d.mkdir()
        dirs[name] = synth.write_world_files(world, str(d))
    seqio.set_backend(seqio.InProcessBam())
    fa, bam = dirs["plain"]
    truth = _bed_run(tmp_path, "truth", bed, ["--phased"], ref=dirs["truth"][0], bam=dirs["truth"][1])
    unphased = _bed_run(tmp_path, "un", bed, ref=fa, bam=bam)
    from vapor_amd import fastpath
    calls = []
    real = fastpath.run
    monkeypatch.setattr(fastpath, "run", lambda *a, **k: calls.append(k) or real(*a, **k))
    got = _bed_run(tmp_path, "hv", bed, ["--phase-vcf", str(vcf)], ref=fa, bam=bam)
    assert calls == [{"phased": True}]
    _check_tables(got, truth, unphased)
    # contradicting tags are not read
    flipped = _bed_run(tmp_path, "flip_ph", bed, ["--phased"], ref=dirs["flipped"][0], bam=dirs["flipped"][1])
    assert flipped != truth and flipped.splitlines()[1].split("\t")[10] == "99"
    assert _bed_run(tmp_path, "flip_hv", bed, ["--phase-vcf", str(vcf)], ref=dirs["flipped"][0], bam=dirs["flipped"][1]) == truth
    monkeypatch.setenv("VAPOR_FAST_PATH", "0")
    assert _bed_run(tmp_path, "hv_drv", bed, ["--phase-vcf", str(vcf)], ref=fa, bam=bam) == truth and len(calls) == 3
    monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
    assert _bed_run(tmp_path, "hv_py", bed, ["--phase-vcf", str(vcf)], ref=dirs["flipped"][0], bam=dirs["flipped"][1]) == truth


def test_vcf_mode_and_its_info_keys(twin_eng, tmp_path):
    w, sites = truth_world()
    snv = tmp_path / "snv.vcf"
    snv.write_text(synth.snv_vcf_text(sites))
    outs = {}
    for name, world, more in (("truth", _tagged_copy(w), ["--phased"]), ("hv", w, ["--phase-vcf", str(snv)]), ("un", w, [])):
        seqio.set_backend(seqio.MemorySamtools(world))
        d = tmp_path / name
        d.mkdir()
        calls = d / "calls.vcf"
        calls.write_text(synth.vcf_text(w))
        assert cli.main(["vcf", "--sv-input", str(calls), "--reference", "ref.fa", "--pacbio-input", "x.bam", "--output-path", str(d / "figs"),
                         "--output-file", str(d / "unused"), "--no-figures"] + more) == 0
        outs[name] = (d / "calls.vcf.vapor").read_text()
    assert outs["hv"] == outs["truth"] != outs["un"]
    recs = [ln.split("\t") for ln in outs["hv"].splitlines() if not ln.startswith("#")]
    plain = [ln.split("\t") for ln in outs["un"].splitlines() if not ln.startswith("#")]
    assert len(recs) == len(plain) >= 9              # (DEL, INV and INS records; the writer leaves the duplications out)
    for r, p in zip(recs, plain):
        assert r[:7] == p[:7] and r[7].startswith(p[7])
        keys = [x.split("=")[0] for x in r[7][len(p[7]):].split(";") if x]
        assert keys and set(keys) <= set(phase.COLUMNS) and keys[0] == "VaPoR_PS" and "VaPoR_PS=1" in r[7]


# ------------------------------------------------------------------------------------------
# two ranks
# ------------------------------------------------------------------------------------------
_WORKER = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from fake_engine import FakeEngine
from oracle import oracle as orc
from vapor_amd import cli, dist, pipeline, seqio, synth
bed, out, figs, vcf = sys.argv[1:5]
w = synth.make_world(17, 9, ("DEL", "INV", "INS"), span_range=(200, 900), read_len=3000, n_reads=24)
synth.snv_world(w, 117)
pipeline.set_engine(FakeEngine(orc))
seqio.set_backend(seqio.MemorySamtools(w))
if os.environ.get("WORLD_SIZE", "1") != "1":
    dist.init_from_env("gloo")
sys.exit(cli.main(["bed", "--sv-input", bed, "--reference", "ref.fa", "--pacbio-input", "x.bam", "--output-path", figs,
                   "--output-file", out, "--no-figures", "--chunk", "3", "--phase-vcf", vcf]))
"""


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_gloo_ranks_write_the_table_of_one(tmp_path, oracle):
    w = synth.make_world(17, 9, ("DEL", "INV", "INS"), span_range=(200, 900), read_len=3000, n_reads=24)
    sites = synth.snv_world(w, 117)
    bed = tmp_path / "in.bed"
    bed.write_text(synth.bed_text(w))
    vcf = tmp_path / "snv.vcf"
    vcf.write_text(synth.snv_vcf_text(sites, phase_set=6))
    script = _WORKER % (os.path.join(ROOT, "tests"), ROOT)
    tables = []
    for world in (1, 2):
        out = tmp_path / ("out%d.vapor" % world)
        port = _free_port()
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                       OMP_NUM_THREADS="1")
            procs.append(subprocess.Popen([sys.executable, "-c", script, str(bed), str(out), str(tmp_path / "figs"), str(vcf)], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        for p in procs:
            try:
                o, _ = p.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            assert p.returncode == 0, o
        tables.append(out.read_text())
    assert tables[0] == tables[1]
    rows = [ln.split("\t") for ln in tables[0].splitlines()]
    assert len(rows) == 10 and all(r[10] == "6" for r in rows[1:])
