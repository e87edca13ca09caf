"""Haplotype-resolved validation (`--phased`, vapor_amd/phase.py) without a GPU: the tag rule in the three
readers, the phase set and the group lists, the phased genotype, and `vapor bed | vcf --phased` on the tests' stand-in engine
and on the CPU twin of the C ABI - which has no tagged device reader, so that the array route takes the host readers' tagged
chop_many there."""
import copy
import ctypes
import os
import re
import socket
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from fake_engine import FakeEngine

from vapor_amd import bamio, cli, phase, pipeline, seqio, synth
from vapor_amd import _lib as L


@pytest.fixture()
def fake(oracle):
    e = FakeEngine(oracle)
    pipeline.set_engine(e)
    yield e
    pipeline.set_engine(None)
    seqio.set_backend(None)


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
# the tags of a record: three readers, one table written by hand
# ------------------------------------------------------------------------------------------

def _i(tag, typ, v):
    return tag.encode() + typ.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ], v)


def _z(tag, n):
    return tag.encode() + b"Z" + b"m" * n + b"\x00"


B_ARRAY = b"XBBS" + struct.pack("<i", 3) + struct.pack("<3H", 7, 8, 9)

# (name, aux bytes, the same as SAM text fields or None where SAM text cannot say it, expected (hap, ps))
TAG_CASES = [
    ("int_c", _i("HP", "c", 1) + _i("PS", "c", 5), ["HP:i:1", "PS:i:5"], (1, 5)),
    ("int_C", _i("HP", "C", 2) + _i("PS", "C", 200), ["HP:i:2", "PS:i:200"], (2, 200)),
    ("int_s", _i("HP", "s", 1) + _i("PS", "s", -3), ["HP:i:1", "PS:i:-3"], (1, -3)),
    ("int_S", _i("HP", "S", 2) + _i("PS", "S", 60000), ["HP:i:2", "PS:i:60000"], (2, 60000)),
    ("int_i", _i("HP", "i", 1) + _i("PS", "i", 123456789), ["HP:i:1", "PS:i:123456789"], (1, 123456789)),
    ("int_I", _i("HP", "I", 2) + _i("PS", "I", 4000000000), ["HP:i:2", "PS:i:4000000000"], (2, 4000000000)),
    ("before_B", _i("HP", "C", 1) + B_ARRAY + _i("PS", "i", 9), ["HP:i:1", "XB:B:S,7,8,9", "PS:i:9"], (1, 9)),
    ("after_B", B_ARRAY + _i("HP", "C", 2) + _i("PS", "i", 9), ["XB:B:S,7,8,9", "HP:i:2", "PS:i:9"], (2, 9)),
    ("after_Z1", _z("MM", 1) + _i("HP", "C", 1) + _i("PS", "C", 4), ["MM:Z:m", "HP:i:1", "PS:i:4"], (1, 4)),
    ("after_Z63", _z("MM", 63) + _i("HP", "C", 2) + _i("PS", "C", 4), ["MM:Z:" + "m" * 63, "HP:i:2", "PS:i:4"], (2, 4)),
    ("after_Z64", _z("MM", 64) + _i("HP", "C", 1) + _i("PS", "C", 4), ["MM:Z:" + "m" * 64, "HP:i:1", "PS:i:4"], (1, 4)),
    ("after_Z65", _z("MM", 65) + _i("HP", "C", 2) + _i("PS", "C", 4), ["MM:Z:" + "m" * 65, "HP:i:2", "PS:i:4"], (2, 4)),
    ("after_Z5000", _z("MM", 5000) + _i("HP", "C", 1) + _i("PS", "C", 4), ["MM:Z:" + "m" * 5000, "HP:i:1", "PS:i:4"], (1, 4)),
    ("hp_Z", b"HPZ1\x00" + _i("PS", "i", 6), ["HP:Z:1", "PS:i:6"], (0, 6)),
    ("hp_0", _i("HP", "i", 0) + _i("PS", "i", 6), ["HP:i:0", "PS:i:6"], (0, 6)),
    ("hp_3", _i("HP", "i", 3) + _i("PS", "i", 6), ["HP:i:3", "PS:i:6"], (0, 6)),
    ("no_hp", _i("PS", "i", 6), ["PS:i:6"], (0, 6)),
    ("no_ps", _i("HP", "i", 1), ["HP:i:1"], (1, None)),
    ("nothing", b"", [], (0, None)),
    ("two_hp", _i("HP", "C", 2) + _i("HP", "C", 1) + _i("PS", "i", 8) + _i("PS", "i", 9), ["HP:i:2", "HP:i:1", "PS:i:8", "PS:i:9"], (2, 8)),
    ("hp_A_f", b"HPA1" + b"PSf" + struct.pack("<f", 2.0) + _i("HP", "C", 2), ["HP:A:1", "PS:f:2.0", "HP:i:2"], (2, None)),
    # a string without its NUL: what stands before it stands, nothing behind it is read
    ("truncated_Z", _i("HP", "C", 1) + b"MMZ" + b"abc", None, (1, None)),
    # an integer cut short
    ("truncated_i", _i("PS", "C", 7) + b"HPi\x01\x00", None, (0, 7)),
    # an unknown type letter
    ("unknown_type", b"XX?\x01" + _i("HP", "C", 1), None, (0, None)),
]
LONG_OPS = 70001                           # the CG:B,I record: "1M1I" * 35000 + "5000M"


def _tag_bam(path, block_size=4096):
    recs = []
    for t, (name, aux, _sam, _exp) in enumerate(TAG_CASES):
        recs.append((name, 0, 100 + 10 * t, "4000M", "ACGT" * 1000, aux))
    recs.append(("long_cg", 0, 500, "1M1I" * 35000 + "5000M", "AC" * 35000 + "G" * 5000, {"HP": 2, "PS": ("I", 4000000000)}))
    bamio.write_bam(str(path), [("c", 200000)], recs, block_size=block_size)
    return [r[0] for r in sorted(recs, key=lambda r: r[2])]


def test_tag_parsers_agree_with_a_hand_written_table(tmp_path, oracle, monkeypatch):
    bam = tmp_path / "tags.bam"
    order = _tag_bam(bam)
    expect = {name: exp for name, _aux, _sam, exp in TAG_CASES}
    expect["long_cg"] = (2, 4000000000)
    be = seqio.InProcessBam()
    # the Python reader's records
    raw = be._open(str(bam)).fetch_raw("c", 1000, 3000)
    assert [r[0] for r in raw] == order and {r[0]: r[6] for r in raw} == expect
    long_rec = [r for r in raw if r[0] == "long_cg"][0]
    assert len(long_rec[2]) == LONG_OPS                                              # (its CIGAR came from the CG array)
    # the two statements of chop_pacbio_read_by_pos: Python and vapor_bam_chop_tagged
    py = be.chop_python(str(bam), "c", 1000, 3000, 500, tagged=True)
    monkeypatch.delenv("VAPOR_BAM_NATIVE", raising=False)
    nat = be.chop(str(bam), "c", 1000, 3000, 500, tagged=True)
    assert py == nat and [r[2] for r in nat] == order
    assert {r[2]: (r[3], r[4]) for r in nat} == expect
    # untagged: the entries are what they were
    assert be.chop(str(bam), "c", 1000, 3000, 500) == [r[:3] for r in nat] == be.chop_python(str(bam), "c", 1000, 3000, 500)
    # SAM text
    for name, _aux, sam, exp in TAG_CASES:
        if sam is not None:
            assert phase.tags_from_sam(sam) == exp, name
    line = synth.SamRecord("q", "c", 5, "10M", "A" * 10, 10, {"MM": "C+m,5", "HP": 2, "XB": ("B", "S", [1, 2]), "PS": 4000000000}).line()
    assert line.split("\t")[11:] == ["MM:Z:C+m,5", "HP:i:2", "XB:B:S,1,2", "PS:i:4000000000"]
    assert phase.tags_from_sam(line.split("\t")[11:]) == (2, 4000000000)
    assert synth.SamRecord("q", "c", 5, "10M", "A" * 10, 10).line().count("\t") == 10          # (untagged: the line of before)
    # the writer's dict form is the raw form
    assert phase.encode_aux({"HP": ("C", 1), "XB": ("B", "S", [7, 8, 9]), "PS": 9}) == _i("HP", "C", 1) + B_ARRAY + _i("PS", "i", 9)
    assert phase.encode_aux({"PS": 4000000000, "MM": "mm"}) == _i("PS", "I", 4000000000) + b"MMZmm\x00"


def test_tagged_chop_through_the_backends(tmp_path, oracle):
    """MemorySamtools (native and per-record statements) and the SAM-text route read the tags of synth.SamRecord.tags."""
    w = synth.make_world(seed=5, n_loci=2, svtypes=("DEL",), spans=[300, 400], read_len=2500, n_reads=8)
    synth.phase_world(w, seed=9, untagged=0.3, phase_set=77)
    l = w.loci[0]
    be = seqio.MemorySamtools(w)
    got = be.chop("x.bam", l.chrom, l.start - 300, l.start + 300, 300, tagged=True)
    assert len(got) == 8 and be.chop("x.bam", l.chrom, l.start - 300, l.start + 300, 300) == [r[:3] for r in got]
    by_name = {r.qname: r for r in w.reads[l.chrom]}
    for read, _miss, qname, hap, ps in got:
        t = by_name[qname].tags
        assert (hap, ps) == ((t["HP"], 77) if t else (0, None))
        assert t is None or t["HP"] == (1 if qname.endswith("a") else 2)
    assert 0 < sum(1 for r in got if r[3]) < 8
    os.environ["VAPOR_MEMORY_CHOP"] = "records"
    try:
        assert be.chop("x.bam", l.chrom, l.start - 300, l.start + 300, 300, tagged=True) == got
    finally:
        del os.environ["VAPOR_MEMORY_CHOP"]

    class TextOnly:                                         # a backend that answers in SAM text alone (SamtoolsCLI's shape)
        view_lines = be.view_lines
    seqio.set_backend(TextOnly())
    try:
        assert seqio.chop_pacbio_read_by_pos("x.bam", l.chrom, l.start - 300, l.start + 300, 300, True) == got
        assert seqio.chop_pacbio_read_by_pos("x.bam", l.chrom, l.start - 300, l.start + 300, 300) == [r[:3] for r in got]
    finally:
        seqio.set_backend(None)


def test_phase_world_draws_in_the_documented_order():
    w = synth.make_world(seed=5, n_loci=3, svtypes=("DEL", "INS"), spans=[300, 400, 350], read_len=2500, n_reads=6)
    before = [(r.qname, r.pos, r.cigar, r.seq) for c in w.reads for r in w.reads[c]]
    synth.phase_world(w, seed=4, untagged=0.5, phase_set=3)
    assert before == [(r.qname, r.pos, r.cigar, r.seq) for c in w.reads for r in w.reads[c]]
    rng = np.random.default_rng(4)
    for l in w.loci:
        for r in w.reads[l.chrom]:
            want = None if rng.random() < 0.5 else {"HP": 1 if r.qname.endswith("a") else 2, "PS": 3}
            assert r.tags == want


# ------------------------------------------------------------------------------------------
# the phase set and the group lists
# ------------------------------------------------------------------------------------------

def _x(rows):
    """Kept records [read, miss_bp, qname, hap, ps] from (miss, hap, ps) rows."""
    return [["r%d" % t, m, "q%d" % t, h, p] for t, (m, h, p) in enumerate(rows)]


def _names(lst):
    return [r[2] for r in lst]


def test_phase_set_rule_on_hand_made_lists():
    # majority
    assert phase.phase_set(_x([(0, 1, 5), (0, 2, 5), (0, 1, 9), (0, 0, 9), (0, 0, 9)])) == (True, 5)
    # untagged records do not vote, whatever their PS
    assert phase.phase_set(_x([(0, 0, 9), (0, 0, 9), (0, 0, 9), (0, 1, 5)])) == (True, 5)
    # a tie goes to the smaller value
    assert phase.phase_set(_x([(0, 1, 9), (0, 2, 5), (0, 1, 5), (0, 2, 9)])) == (True, 5)
    assert phase.phase_set(_x([(0, 1, -2), (0, 2, 4000000000), (0, 1, 7)])) == (True, -2)
    # "none" against a number: below every number in a tie, outvoted otherwise
    assert phase.phase_set(_x([(0, 1, None), (0, 2, 0)])) == (True, None)
    assert phase.phase_set(_x([(0, 1, None), (0, 2, -5), (0, 2, -5)])) == (True, -5)
    assert phase.phase_set(_x([(0, 1, None), (0, 1, None), (0, 2, 3)])) == (True, None)
    # no tagged record
    assert phase.phase_set(_x([(0, 0, 3), (0, 0, None)])) == (False, None) and phase.phase_set([]) == (False, None)


def test_group_lists_on_hand_made_lists():
    # two phase sets: the minority's tagged reads are in no haplotype group
    x = _x([(0, 1, 5), (3, 2, 5), (1, 1, 9), (0, 0, None), (2, 2, 5), (0, 1, 5)])
    s = phase.select(x)
    assert (s.tagged, s.ps) == (True, 5)
    assert list(s) == x == s.groups[0] and _names(s.groups[1]) == ["q0", "q5"] and _names(s.groups[2]) == ["q1", "q4"]
    assert s.union == x and s.mask == [3, 5, 1, 1, 5, 3] and s.pos == ([0, 1, 2, 3, 4, 5], [0, 5], [1, 4])
    # "none" as the phase set
    s = phase.select(_x([(0, 1, None), (0, 2, None), (0, 2, 4)]))
    assert s.ps is None and s.tagged and _names(s.groups[1]) == ["q0"] and _names(s.groups[2]) == ["q1"]
    # no tagged record: empty haplotype groups
    s = phase.select(_x([(0, 0, 1), (0, 0, 1)]))
    assert not s.tagged and s.groups[1] == [] and s.groups[2] == [] and s.mask == [1, 1]
    # a group of 25: the cap and the miss order; a group of 20: file order, whatever its miss values
    rng = np.random.default_rng(3)
    rows = [(int(rng.integers(0, 4)), 1, 7) for _ in range(25)] + [(int(rng.integers(0, 4)), 2, 7) for _ in range(20)]
    order = rng.permutation(45)
    x = _x([rows[i] for i in order])
    s = phase.select(x)
    g1 = [r for r in x if r[3] == 1]
    g2 = [r for r in x if r[3] == 2]
    assert len(g1) == 25 and len(g2) == 20
    assert s.groups[1] == sorted(g1, key=lambda r: r[1])[:20]                      # (a stable sort: input order inside one value)
    assert s.groups[2] == g2
    assert s.groups[0] == sorted(x, key=lambda r: r[1])[:20] == seqio.minimize_pacbio_read_list(x)
    assert [x.index(r) for r in s.union] == sorted({x.index(r) for g in s.groups for r in g}) and len(s.union) <= 60
    for g in range(3):
        assert [s.union[u] for u in s.pos[g]] == s.groups[g]
        assert all((s.mask[u] >> g) & 1 for u in s.pos[g])
    # the number form (what the array route and the device hand over) is the same selection
    miss = np.asarray([r[1] for r in x]); hap = np.asarray([r[3] for r in x]); ps = np.asarray([r[4] for r in x])
    tagged, p, idx, words = phase.select_numbers(miss, hap, ps, 20)
    assert (tagged, p) == (True, 7) and [x[i] for i in idx] == s.union and [w & 7 for w in words] == s.mask
    scores = [float(i) for i in idx]
    a, h1, h2 = phase.split_scores(words, scores, 3)
    assert a == [float(x.index(r)) for r in s.groups[0]] and h1 == [float(x.index(r)) for r in s.groups[1]]
    assert h2 == [float(x.index(r)) for r in s.groups[2]]
    assert phase.split_scores(words, scores, 20)[1:] == [None, None] and phase.split_scores(words, scores, 19)[1] is not None


def test_phased_genotype_on_hand_made_counts():
    q = np.log(0.95 / 0.05) / np.log(10)
    assert phase.allele(5, 1) == "1" and phase.allele(5, 4) == "0" and phase.allele(4, 2) == "." and phase.allele(0, 0) == "."
    assert phase.allele(1, 0) == "1" and phase.allele(1, 1) == "0"
    assert phase.quality(5, 1) == 3 * q and phase.quality(5, 4) == 3 * q and phase.quality(4, 2) == 0
    assert phase.genotype((5, 0), (6, 6)) == ("1|0", str(5 * q))
    assert phase.genotype((9, 1), (4, 0)) == ("1|1", str(4 * q))
    assert phase.genotype((5, 0), (4, 2)) == ("1|.", ".")                       # a tie
    assert phase.genotype(None, (4, 4)) == (".|0", ".")                         # an unreported group
    assert phase.genotype((0, 0), (4, 4)) == (".|0", ".")                       # a reported group without a scored read
    assert phase.genotype(None, None) == (".", ".") and phase.genotype((2, 1), None) == (".", ".")
    # the counts: non-positive after rounding to two decimals (finish.rounded_nonpositive)
    assert phase.counts([0.5, 0.004, 0.005, -1.0, 0.0]) == (5, 3)
    # the columns of a row
    from vapor_amd import finish
    h1, h2 = [0.5, 0.25, 0.004, 0.7, 0.9], [-1.0, -0.5, 0.3, -0.2]
    t1, t2 = finish.row_tail(h1), finish.row_tail(h2)
    assert phase.columns((True, 12, h1, h2)) == ["12", "1|0", str(2 * q), str(t1[0]), str(t1[1]), t1[4], str(t2[0]), str(t2[1]), t2[4]]
    assert phase.columns((True, None, h1, None)) == [".", "1|.", ".", str(t1[0]), str(t1[1]), t1[4], ".", ".", "."]
    assert phase.columns((False, None, None, None)) == ["."] * 9 == phase.columns(None)
    assert phase.columns((True, 3, [], h2))[1:6] == [".|0", ".", "NA", "NA", "NA"]
    for ph in ((True, 4000000000, h1, h2), (True, None, None, h2), (False, None, None, None), (True, -7, [], [])):
        assert phase.unpack(phase.pack(ph)) == ph
    assert phase.pack(None) == [] and phase.unpack([]) is None
    table = [(True, 12, h1, h2), None, (True, None, h1, None), (True, 3, [], h2), (False, None, None, None)]
    assert phase.columns_many(table) == [phase.columns(ph) for ph in table] and phase.columns_many([]) == []


# ------------------------------------------------------------------------------------------
# `vapor bed --phased`: the subset oracle
# ------------------------------------------------------------------------------------------

def _bed_run(tmp, name, bed_text, extra=(), ref="ref.fa", bam="x.bam"):
    bed = tmp / (name + ".bed")
    bed.write_text(bed_text)
    out = tmp / (name + ".vapor")
    args = ["bed", "--sv-input", str(bed), "--reference", ref, "--pacbio-input", bam, "--output-path", str(tmp / "figs"),
            "--output-file", str(out)] + list(extra)
    if "--figures" in args:
        args.remove("--figures")
    else:
        args.append("--no-figures")
    assert cli.main(args) == 0
    return [ln.split("\t") for ln in out.read_text().splitlines()]


def _only_hap(world, h):
    w = copy.copy(world)
    w.reads = {c: [r for r in rs if r.tags and r.tags.get("HP") == h] for c, rs in world.reads.items()}
    return w


def _oracle_world():
    w = synth.make_world(seed=71, n_loci=36, svtypes=("DEL", "INV", "INS"), span_range=(100, 3000), read_len=7000, n_reads=30)
    return synth.phase_world(w, seed=1071)


def _check_subset_oracle(rows, sub1, sub2, unphased):
    assert rows[0][:10] == unphased[0] and tuple(rows[0][10:]) == phase.COLUMNS
    assert [r[:10] for r in rows] == unphased                            # the first columns: the unphased table
    assert len(rows) == 37
    for t in range(1, len(rows)):
        r = rows[t]
        assert len(r) == 19 and "." not in r[10:], (t, r[10:])             # no locus is left out, no field is empty
        assert r[10] == "1"
        for h, sub in ((1, sub1), (2, sub2)):
            got = r[13 + 3 * (h - 1):16 + 3 * (h - 1)]
            assert got == [sub[t][5], sub[t][6], sub[t][9]], (t, h)        # QS, GS, Rec: text for text
        # the genotype is the statement's, from the Rec strings
        kl = []
        for h in (1, 2):
            sc = [float(v) for v in r[15 + 3 * (h - 1)].split(",")]
            kl.append((len(sc), sum(1 for v in sc if not v > 0)))
        assert (r[11], r[12]) == phase.genotype(*kl)


def test_subset_oracle_memory_world(twin_eng, tmp_path, monkeypatch):
    """For h = 1, 2 the H_h QS / GS / Rec of a phased run equal VaPoR_QS / VaPoR_GS / VaPoR_Rec of an unphased run on the world
    that keeps only the HP = h records: on the array route and with the drivers' route forced."""
    w = _oracle_world()
    # all 30 reads of every locus are kept (so the cap of 20 is exercised), and the smallest group is above the gate of 3
    seqio.set_backend(seqio.MemorySamtools(w))
    sizes = []
    for l in w.loci:
        recs = w.reads[l.chrom]
        assert len(recs) == 30
        sizes += [sum(1 for r in recs if r.tags and r.tags["HP"] == h) for h in (1, 2)]
    assert min(sizes) == 6 and max(len(w.reads[l.chrom]) for l in w.loci) > 20
    bed = synth.bed_text(w)
    unphased = _bed_run(tmp_path, "un", bed)
    rows = _bed_run(tmp_path, "ph", bed, ["--phased"])
    monkeypatch.setenv("VAPOR_FAST_PATH", "0")
    rows_drv = _bed_run(tmp_path, "ph_drv", bed, ["--phased"])
    monkeypatch.delenv("VAPOR_FAST_PATH")
    assert rows == rows_drv
    subs = []
    for h in (1, 2):
        seqio.set_backend(seqio.MemorySamtools(_only_hap(w, h)))
        subs.append(_bed_run(tmp_path, "sub%d" % h, bed))
    _check_subset_oracle(rows, subs[0], subs[1], unphased)


def test_subset_oracle_from_files_with_the_host_reader(twin_eng, tmp_path):
    """The same from FASTA / BAM files: vapor_bam_chop_tagged behind the array route (the twin has no tagged device reader)."""
    w = _oracle_world()
    args = [None] * 19
    args[2] = args[9] = 0
    assert L.load().vapor_bam_chop_device_tagged(*args) == L.E_ARG                   # (the twin's stub refuses every call)
    with pytest.raises(NotImplementedError):
        twin_eng.bam_chop_device(None, [], [], [], [], [0], [], tagged=True)
    dirs = {}
    for name, world in (("all", w), ("h1", _only_hap(w, 1)), ("h2", _only_hap(w, 2))):
        d = tmp_path / name
        d.mkdir()
        dirs[name] = synth.write_world_files(world, str(d))
    seqio.set_backend(seqio.InProcessBam())
    bed = synth.bed_text(w)
    fa, bam = dirs["all"]
    unphased = _bed_run(tmp_path, "un", bed, ref=fa, bam=bam)
    rows = _bed_run(tmp_path, "ph", bed, ["--phased"], ref=fa, bam=bam)
    subs = [_bed_run(tmp_path, "sub" + h, bed, ref=dirs[h][0], bam=dirs[h][1]) for h in ("h1", "h2")]
    _check_subset_oracle(rows, subs[0], subs[1], unphased)
    # an unphased run from the tagged file is the unphased run from the same file written without tags
    plain = copy.copy(w)
    plain.reads = {c: [synth.SamRecord(r.qname, r.rname, r.pos, r.cigar, r.seq, r.ref_span) for r in rs] for c, rs in w.reads.items()}
    d = tmp_path / "plain"
    d.mkdir()
    fa0, bam0 = synth.write_world_files(plain, str(d))
    assert os.path.getsize(bam0) < os.path.getsize(bam)
    assert _bed_run(tmp_path, "un0", bed, ref=fa0, bam=bam0) == unphased
    # and a phased run on the untagged file: the unphased table with nine '.'
    rows0 = _bed_run(tmp_path, "ph0", bed, ["--phased"], ref=fa0, bam=bam0)
    assert [r[:10] for r in rows0] == unphased and all(r[10:] == ["."] * 9 for r in rows0[1:])


def test_the_gate(twin_eng, tmp_path):
    """A group whose list has no more than num_reads_cff (3) reads is not reported: its fields and its allele are '.', the other
    haplotype's and the main columns are not affected."""
    w = synth.make_world(seed=73, n_loci=36, svtypes=("DEL", "INV", "INS"), span_range=(100, 3000), read_len=7000, n_reads=16)
    synth.phase_world(w, seed=1073)
    seqio.set_backend(seqio.MemorySamtools(w))
    small = {(t, h) for t, l in enumerate(w.loci) for h in (1, 2)
             if sum(1 for r in w.reads[l.chrom] if r.tags and r.tags["HP"] == h) <= 3}
    assert len(small) == 3
    bed = synth.bed_text(w)
    unphased = _bed_run(tmp_path, "un", bed)
    rows = _bed_run(tmp_path, "ph", bed, ["--phased"])
    assert [r[:10] for r in rows] == unphased
    for t in range(36):
        r = rows[t + 1]
        assert r[5] != "NA"
        for h in (1, 2):
            f = r[13 + 3 * (h - 1):16 + 3 * (h - 1)]
            if (t, h) in small:
                assert f == [".", ".", "."] and r[11].split("|")[h - 1] == "." and r[12] == "."
            else:
                assert "." not in f and "NA" not in f


# ------------------------------------------------------------------------------------------
# routes
# ------------------------------------------------------------------------------------------

def _two_set_world():
    """DEL, INV, TANDUP and INS loci; on half of them a third of the tagged reads sits in a second phase set, and one locus has
    a tie between the two sets."""
    w = synth.make_world(seed=29, n_loci=12, svtypes=("DEL", "INV", "TANDUP", "INS"), span_range=(150, 1200), read_len=4200, n_reads=26)
    synth.phase_world(w, seed=31, untagged=0.15, phase_set=40)
    for t, l in enumerate(w.loci):
        if t % 2 == 0:
            tagged = [r for r in w.reads[l.chrom] if r.tags]
            for r in tagged[::3]:
                r.tags = {"HP": r.tags["HP"], "PS": 20}
            if t == 4:
                for q, r in enumerate(tagged):
                    r.tags = {"HP": r.tags["HP"], "PS": 20 if q % 2 else 40}
                if len(tagged) % 2:
                    tagged[-1].tags = None
        if t == 5:
            for r in w.reads[l.chrom]:
                if r.tags:
                    r.tags = {"HP": r.tags["HP"]}                  # a locus whose phase set is "none"
    return w


def test_routes_give_the_same_table(twin_eng, tmp_path, monkeypatch):
    """The array route, the drivers' route and a figure-drawing run (which goes entirely through the drivers) give the same
    table, TANDUP loci and loci with reads from two phase sets included."""
    w = _two_set_world()
    seqio.set_backend(seqio.MemorySamtools(w))
    bed = synth.bed_text(w)
    calls = []
    from vapor_amd import fastpath
    real = fastpath.run
    monkeypatch.setattr(fastpath, "run", lambda *a, **k: calls.append(k) or real(*a, **k))
    rows = _bed_run(tmp_path, "array", bed, ["--phased"])
    assert calls == [{"phased": True}]
    monkeypatch.setenv("VAPOR_FAST_PATH", "0")
    assert _bed_run(tmp_path, "drivers", bed, ["--phased"]) == rows and len(calls) == 1
    monkeypatch.delenv("VAPOR_FAST_PATH")
    assert _bed_run(tmp_path, "figures", bed, ["--phased", "--figures"]) == rows and len(calls) == 1
    assert len([f for f in os.listdir(tmp_path / "figs") if f.endswith(".png")]) >= 12
    unphased = _bed_run(tmp_path, "un", bed)
    assert [r[:10] for r in rows] == unphased and calls[-1] == {}
    ps = [r[10] for r in rows[1:]]
    assert ps[4] == "20" and ps[5] == "." and set(ps) == {"20", "40", "."} and ps[0] == "40"
    assert rows[6][11] != "." and "." not in rows[6][13:]                   # phase set "none": the groups are still reported
    kinds = {r[3] for r in rows[1:] if "." not in r[11:]}
    assert kinds == {"DEL", "INV", "TANDUP", "INS"}
    # from files (sorted by position: another record order, so another table), through vapor_bam_chop_tagged: the array
    # route, the drivers' route and the Python reader agree there as well
    d = tmp_path / "files"
    d.mkdir()
    fa, bam = synth.write_world_files(w, str(d))
    seqio.set_backend(seqio.InProcessBam())
    rows_f = _bed_run(tmp_path, "files_array", bed, ["--phased"], ref=fa, bam=bam)
    assert len(calls) == 3 and calls[-1] == {"phased": True}
    assert [r[:10] for r in rows_f] == _bed_run(tmp_path, "files_un", bed, ref=fa, bam=bam)
    assert [r[10] for r in rows_f] == [r[10] for r in rows] and {r[3] for r in rows_f[1:] if "." not in r[11:]} == kinds
    monkeypatch.setenv("VAPOR_FAST_PATH", "0")
    assert _bed_run(tmp_path, "files_drivers", bed, ["--phased"], ref=fa, bam=bam) == rows_f
    monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
    assert _bed_run(tmp_path, "files_python", bed, ["--phased"], ref=fa, bam=bam) == rows_f


# ------------------------------------------------------------------------------------------
# `vapor vcf --phased`
# ------------------------------------------------------------------------------------------

def test_vcf_columns_info_keys_and_unphased_rows(twin_eng, tmp_path):
    w = synth.make_world(seed=41, n_loci=7, svtypes=("DEL", "INV", "INS", "DEL_INV", "DUP_INV", "DEL", "DEL"),
                         spans=[400, 500, 300, 600, 500, 30, 450], read_len=3600, n_reads=24)
    synth.phase_world(w, seed=43, untagged=0.1, phase_set=8)
    for r in w.reads[w.loci[6].chrom]:
        r.tags = None                                                          # a scored locus without a tagged read
    seqio.set_backend(seqio.MemorySamtools(w))
    text = synth.vcf_text(w) + "\t".join([w.loci[0].chrom, "900", "bnd1", "N", "N[%s:700[" % w.loci[1].chrom, ".", "PASS", "SVTYPE=BND", "GT", "0/1"]) + "\n"
    vcf = tmp_path / "calls.vcf"
    vcf.write_text(text)
    args = ["vcf", "--sv-input", str(vcf), "--reference", "ref.fa", "--pacbio-input", "x.bam", "--output-path", str(tmp_path / "figs"),
            "--output-file", str(tmp_path / "unused"), "--no-figures", "--bnd"]
    assert cli.main(args) == 0
    plain = (tmp_path / "calls.vcf.vapor").read_text().splitlines()
    # the table before vcf_vapor_modify rewrites it: captured through the writer's own hook
    from vapor_amd import simple_function as SF
    tables = []
    real = SF.vcf_vapor_modify
    SF.vcf_vapor_modify = lambda v, *a, **k: (tables.append(open(v + ".vapor").read().splitlines()), real(v, *a, **k))[1]
    try:
        assert cli.main(args) == 0
        assert cli.main(args + ["--phased"]) == 0
    finally:
        SF.vcf_vapor_modify = real
    un, ph = [[ln.split("\t") for ln in t] for t in tables]
    assert tuple(ph[0][10:]) == phase.COLUMNS and [r[:len(un[k])] for k, r in enumerate(ph)] == un
    by_type = {}
    for r in ph[1:]:
        assert len(r) == 15
        by_type.setdefault(r[0].split(":")[-1], []).append(r)
    assert set(by_type) == {"DEL", "INV", "INS", "DEL_INV", "DUP_INV", "BND"}
    for t in ("DEL_INV", "DUP_INV", "BND"):
        assert all(r[6:] == ["."] * 9 for r in by_type[t]) and all(r[1] != "NA" for r in by_type[t])
    na = [r for r in by_type["DEL"] if r[1] == "NA"]
    assert len(na) == 1 and na[0][6:] == ["."] * 9                              # the deletion below 50 bp
    untagged = [r for r in by_type["DEL"] if r[0].startswith(w.loci[6].chrom + ":")][0]
    assert untagged[1] != "NA" and untagged[6:] == ["."] * 9
    scored = [by_type["DEL"][0], by_type["INV"][0], by_type["INS"][0]]
    assert all(r[6] == "8" and "." not in r[7:] for r in scored)
    # the annotated VCF
    out = (tmp_path / "calls.vcf.vapor").read_text().splitlines()
    new_meta = [ln for ln in out if ln.startswith("##") and ln not in plain]
    assert [re.match(r"##INFO=<ID=(\w+),", ln).group(1) for ln in new_meta] == list(phase.COLUMNS)
    assert [ln for ln in plain if ln.startswith("#")] == [ln for ln in out if ln.startswith("#") and ln not in new_meta]
    recs_p = [ln.split("\t") for ln in plain if not ln.startswith("#")]
    recs = [ln.split("\t") for ln in out if not ln.startswith("#")]
    assert len(recs) == len(recs_p) == 8
    row_of = {r[0]: r for r in ph[1:]}
    for p, r in zip(recs_p, recs):
        assert p[:7] == r[:7] and p[8:] == r[8:] and r[7].startswith(p[7])
        extra = [x.split("=") for x in r[7][len(p[7]):].split(";") if x]
        svtype = dict(x.split("=") for x in p[7].split(";") if "=" in x)["SVTYPE"]
        if svtype in ("DEL_INV", "DUP_INV", "BND") or r[0] == w.loci[6].chrom or r[0] == w.loci[5].chrom:
            assert extra == []                                                 # keys whose value is '.' are omitted
        else:
            assert [k for k, _v in extra] == list(phase.COLUMNS)
            row = [x for key, x in row_of.items() if key.startswith(r[0] + ":")][0]
            assert [v for _k, v in extra] == row[6:]


def test_option_errors(capsys):
    base = ["--sv-input", "a.bed", "--reference", "r.fa", "--pacbio-input", "x.bam", "--output-path", "o", "--output-file", "o.vapor"]
    for mode, more in (("bed", ["--phased", "--refine", "20"]), ("vcf", ["--refine", "20", "--phased"]), ("svelter", ["--phased"]),
                       ("ins", ["--phased"])):
        with pytest.raises(SystemExit) as e:
            cli.main([mode] + base + more)
        assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--phased and --refine" in err and "--phased applies to" in err
    assert cli.build_parser().parse_args(base + ["--phased"]).phased and not cli.build_parser().parse_args(base).phased


def test_entry_points_are_declared(twin_eng, oracle):
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    for name in ("vapor_bam_chop_tagged", "vapor_bam_chop_device_tagged"):
        assert re.search(r"\bint %s\(" % name, h) and name in L.EXPORTS
    assert "vapor_bam_chop_device_tagged" in L.OPTIONAL_EXPORTS and "vapor_bam_chop_tagged" not in L.OPTIONAL_EXPORTS
    assert L.ABI_VERSION == 3 and hasattr(L.load(), "vapor_bam_chop_tagged")     # (the twin compiles the host reader in)
    assert "SF:339-354" in h[h.index("vapor_bam_chop_device_tagged") - 2200:h.index("vapor_bam_chop_device_tagged")]
    assert "SF:1091-1102" in h[h.index("vapor_bam_chop_device_tagged") - 2200:h.index("vapor_bam_chop_device_tagged")]


# ------------------------------------------------------------------------------------------
# two ranks
# ------------------------------------------------------------------------------------------

_WORKER = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from fake_engine import FakeEngine
from oracle import oracle as orc
from vapor_amd import cli, dist, pipeline, seqio, synth
bed, out, figs = sys.argv[1:4]
w = synth.make_world(seed=53, n_loci=9, svtypes=("DEL", "INV", "INS"), span_range=(150, 900), read_len=3000, n_reads=24)
synth.phase_world(w, seed=57, phase_set=6)
pipeline.set_engine(FakeEngine(orc))
seqio.set_backend(seqio.MemorySamtools(w))
if os.environ.get("WORLD_SIZE", "1") != "1":
    dist.init_from_env("gloo")
sys.exit(cli.main(["bed", "--sv-input", bed, "--reference", "ref.fa", "--pacbio-input", "x.bam", "--output-path", figs,
                   "--output-file", out, "--no-figures", "--chunk", "3", "--phased"]))
"""


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_gloo_ranks_write_the_table_of_one(tmp_path, oracle):
    w = synth.make_world(seed=53, n_loci=9, svtypes=("DEL", "INV", "INS"), span_range=(150, 900), read_len=3000, n_reads=24)
    bed = tmp_path / "in.bed"
    bed.write_text(synth.bed_text(w))
    script = _WORKER % (os.path.join(ROOT, "tests"), ROOT)
    tables = []
    for world in (1, 2):
        out = tmp_path / ("out%d.vapor" % world)
        port = _free_port()
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                       OMP_NUM_THREADS="1")
            procs.append(subprocess.Popen([sys.executable, "-c", script, str(bed), str(out), str(tmp_path / "figs")], env=env,
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
    assert len(rows) == 10 and tuple(rows[0][10:]) == phase.COLUMNS and all(r[10] == "6" and "." not in r[11:] for r in rows[1:])
