"""The evidence modes' chunk hook (`--depth`, `--signatures`, `--links`, `--support`) over a per-chromosome
pattern of two BAM files, and the two behaviours of the native host readers.  The hook: a chunk of every measured type and one
without a payload, the payloads against those built here by hand - the module's rule over each file's records, the module's merge
across the files -, the number of the backend's calls and the order of their regions, on the native host readers and on the Python
statement.  No device is asked (VAPOR_BAM_DEVICE=0)."""
import os

import pytest

from vapor_amd import _lib as L
from vapor_amd import bamio, cli, depth, links, modes, seqio, signature, support  # noqa: F401  (cli sets the modes' hooks)

MODULES = {"depth": depth, "signatures": signature, "links": links, "support": support}
MANY = {"depth": "depth_many", "signatures": "signature_many", "links": "links_many", "support": "support_many"}
ZERO = {"depth": [0] * 3, "signatures": [0] * 10, "links": [0] * 5, "support": [0] * 7}
REFS = [("c", 60000), ("d", 3000)]


def _sa(*entries):
    return b"SAZ" + b"".join(e.encode() + b";" for e in entries) + b"\0"


def _rec(name, tid, pos0, cigar, aux=b"", flag=0, mapq=60):
    import re
    qlen = sum(int(n) for n, c in re.findall(r"(\d+)([MIS=X])", cigar))
    return (name, tid, pos0, cigar, "ACGT" * (qlen // 4) + "A" * (qlen % 4), aux, mapq, flag)


# per locus of JOBS below: records that clip at, span, or carry the event at its breakpoints; which file holds which: 1, 2 or both
RECORDS = [
    (1, _rec("del_clip", 0, 4900, "100M40S", _sa("c,5301,+,100S40M,60,0"))),
    (2, _rec("del_gap", 0, 4900, "100M300D100M")),
    (3, _rec("del_ref", 0, 4900, "200M")),
    (3, _rec("del_dup", 0, 4900, "200M", flag=0x400)),                       # never counted
    (2, _rec("del_sup", 0, 5300, "60S100M", _sa("c,4901,+,100M60S,60,0"), flag=0x800)),
    (1, _rec("big_l", 0, 7850, "150M40S", _sa("c,29001,+,150S40M,60,0"))),
    (2, _rec("big_r", 0, 29000, "40S150M", _sa("c,7851,+,150M40S,60,2"))),
    (3, _rec("big_ref", 0, 28900, "300M")),
    (1, _rec("dup_l", 0, 30000, "40S200M", _sa("c,30601,+,200M40S,60,0"))),
    (2, _rec("dup_r", 0, 30600, "200M40S", _sa("c,30001,+,200S40M,20,0"))),
    (1, _rec("dup_ins", 0, 30350, "100M800I100M")),
    (3, _rec("inv_l", 0, 34880, "120M45S", _sa("c,35881,-,45S120M,60,0"))),
    (2, _rec("inv_r", 0, 36000, "45S120M", _sa("c,35001,-,120M45S,60,0"))),
    (1, _rec("ins_op", 0, 39900, "100M80I100M")),
    (2, _rec("ins_clip", 0, 39900, "100M35S")),
    (3, _rec("ins_ref", 0, 39800, "400M")),
    (2, _rec("bnd_a", 0, 44900, "100M40S", _sa("x,5,+,10M,60,0", "d,700,+,40S100M,60,1"))),
    (1, _rec("bnd_b", 1, 699, "40S100M", _sa("c,44901,+,100M40S,60,0"))),
    (1, _rec("bnd_c", 0, 46900, "100M40S", _sa("d,1401,-,100M40S,60,0"))),
    (1, _rec("bnd_d", 1, 1400, "100M40S", _sa("c,46901,-,100M40S,60,0"))),
]
INS_SEQ = "ACGT" * 20
# (type, chrom, start, end, ins_seq) of a cli.Job's spec, or a breakend's scored view
JOBS = [("DEL", "c", 5001, 5300, ""), ("DEL", "c", 8001, 29000, ""), ("TANDUP", "c", 30001, 30800, ""), ("INV", "c", 35001, 36000, ""),
        ("INS", "c", 40000, 40000, INS_SEQ), ("DISDUP", "c", 50001, 50500, "")]
BNDS = [["c", 45000, "d", 700, "3to5", ""], ["c", 47000, "d", 1500, "3to3", "ACGT"]]


class _Job:
    """What the hook reads of a cli.Job."""
    def __init__(self, spec=None, ctx=None, bnd=None):
        self.spec, self.ctx, self.bnd = spec, ctx, bnd


@pytest.fixture(scope="module")
def pattern(tmp_path_factory):
    """Two files of one XXX pattern: the first has both contigs, the second lacks `d`."""
    d = tmp_path_factory.mktemp("evidence_hook")
    bamio.write_bam(str(d / "reads.one.bam"), REFS, [r for where, r in RECORDS if where & 1], block_size=4096)
    bamio.write_bam(str(d / "reads.two.bam"), REFS[:1], [r for where, r in RECORDS if where & 2], block_size=4096)
    return str(d / "reads.XXX.bam")


def _regions_of(name, svtype, locus, length_of):
    """[(contig, fields, partner or None)] of a locus, in the order the hook sends them, from the module's own `regions`."""
    mod = MODULES[name]
    if name == "links":
        left, right = links.regions(svtype, locus, length_of)
        return left + right
    return [(locus[0], f, None) for f in mod.regions(svtype, locus, length_of(locus[0]))]


def _answer(name, b, contig, fields, partner):
    """A region's words from one file by the module's rule over bamio's records."""
    lo, hi = (fields[0], fields[3]) if name == "depth" else (fields[0], fields[1])
    if contig not in b.tid or not hi > lo:
        return list(ZERO[name])
    if name == "links":
        return links.words(links.answer(b.fetch_links(contig, lo + 1, hi, exclude_more=links.EXCLUDE), fields, partner, 0))
    recs = [(r[1], r[2]) for r in b.fetch_raw(contig, lo + 1, hi, exclude_more=MODULES[name].EXCLUDE)]
    if name == "depth":
        return depth.cover(recs, fields)
    return signature.words(signature.answer(recs, fields)) if name == "signatures" else support.answer(recs, fields)


def _merge(name, a, b):
    return [int(x) + int(y) for x, y in zip(a, b)] if name == "depth" else MODULES[name].merge_words(a, b)


def _payload(name, svtype, locus, regs, got):
    """A locus's payload from its regions' merged words."""
    if not regs:
        return None
    if name == "depth":
        cov_in = sum(g[1] for g in got)
        cov_fl = sum(g[0] + g[2] for g in got)
        len_in = sum(f[2] - f[1] for _c, f, _p in regs)
        len_fl = sum((f[1] - f[0]) + (f[3] - f[2]) for _c, f, _p in regs)
        return depth.Payload([cov_in, len_in, cov_fl, len_fl], svtype)
    if name == "links":
        half = len(regs) // 2                     # (left and right: as many regions each)
        l = r = [0] * 5
        for a in got[:half]:
            l = links.merge_words(l, a)
        for a in got[half:]:
            r = links.merge_words(r, a)
        start, end = (locus[1], locus[3]) if svtype == "BND" else (locus[1], locus[2])
        return links.Payload([l[2], l[1], r[2], r[1], l[3], l[4], r[3], r[4]], start, end)
    return MODULES[name].payload(svtype, locus, [f for _c, f, _p in regs], got)


def _whole(p):
    return None if p is None else (type(p), list(p), vars(p))


@pytest.mark.parametrize("native", ["1", "0"])
@pytest.mark.parametrize("name", list(MODULES))
def test_the_hook_over_two_files_of_a_pattern(name, native, pattern, monkeypatch):
    mod, mode = MODULES[name], {"depth": modes.DEPTH, "signatures": modes.SIGNATURES, "links": modes.LINKS, "support": modes.SUPPORT}[name]
    monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
    monkeypatch.setenv("VAPOR_BAM_NATIVE", native)
    be = seqio.InProcessBam()
    held = seqio._backend
    seqio.set_backend(be)
    calls = []
    real = getattr(be, MANY[name])
    monkeypatch.setattr(be, MANY[name], lambda engine, f, chroms, regions, *partners: calls.append((f, list(chroms), [tuple(int(v) for v in r) for r in regions],
                                                                                               [list(p) for p in partners]))
                        or real(engine, f, chroms, regions, *partners))
    lengths = []
    real_length = be.contig_length
    monkeypatch.setattr(be, "contig_length", lambda f, ref, chrom: lengths.append(f) or real_length(f, ref, chrom))
    ctx = (3, pattern, "r.fa")
    jobs = [_Job(spec, ctx) for spec in JOBS]
    if name == "links":
        jobs[2:2] = [_Job(bnd=(BNDS[0], ctx))]
        jobs.append(_Job(bnd=(BNDS[1], ctx)))
    jobs.append(_Job())                              # (a row of fixed scores: no spec, no breakend)
    try:
        files = seqio.bam_in_decide(pattern, None)
        assert sorted(os.path.basename(f) for f in files) == ["reads.one.bam", "reads.two.bam"]
        got = mode.chunk_payloads(jobs, list(range(len(jobs))), None)
    finally:
        seqio.set_backend(held)
    # by hand: every locus's regions on the first file's contig lengths, every region's words per file, merged across the files
    opened = [bamio.BamFile(f) for f in files]
    first = opened[0]
    length_of = lambda c: int(first.refs[first.tid[c]][1]) if c in first.tid else 0      # noqa: E731
    want, sent = {}, []
    for t, j in enumerate(jobs):
        if j.bnd is not None:
            svtype, locus = "BND", list(j.bnd[0])
        elif j.spec is not None:
            svtype, chrom, s, e, ins_seq = j.spec
            locus = [chrom, s, len(ins_seq)] if svtype == "INS" else [chrom, s, e]
        else:
            continue
        if svtype not in mod.TYPES:
            continue
        regs = _regions_of(name, svtype, locus, length_of)
        words = []
        for contig, fields, partner in regs:
            w = list(ZERO[name])
            for b in opened:
                w = _merge(name, w, _answer(name, b, contig, fields, partner))
            words.append([int(v) for v in w])
        sent += regs
        want[t] = _payload(name, svtype, locus, regs, words)
    for b in opened:
        b.close()
    assert sorted(got) == sorted(want) and len(want) == {"depth": 3, "signatures": 5, "links": 6, "support": 5}[name]
    for t in want:
        assert _whole(got[t]) == _whole(want[t]), (name, t, got[t], want[t])
    assert any(any(list(p)[:3]) for p in got.values())                    # (the records are seen)
    if name == "links":
        assert sum(p[0] + p[2] for p in got.values()) >= 6, got            # linked reads on DEL, TANDUP, INV and both breakends
    # one call per file, in the files' order, each with every region of the chunk in the jobs' order
    assert [c[0] for c in calls] == files and set(lengths) == {files[0]}
    for _f, chroms, regions, partners in calls:
        assert chroms == [c for c, _f2, _p in sent] and regions == [tuple(f) for _c, f, _p in sent]
        assert partners == ([[p for _c, _f2, p in sent]] if name == "links" else [])
    assert len(sent) == {"depth": 4, "signatures": 6, "links": 14, "support": 6}[name]


# ------------------------------------------------------------------------------------------------------------------------------
# the native host readers: depth answers a region without chunks itself, the others let the library refuse in its own words
# ------------------------------------------------------------------------------------------------------------------------------
def test_depth_native_answers_zeros_without_the_library_when_the_index_lists_no_chunk(pattern, monkeypatch):
    b = bamio.BamFile(pattern.replace("XXX", "one"))
    assert b.index.chunks(0, 52000, 53000) == [] and b.index.chunks(0, 4000, 6300) != []
    want = b.depth_native(0, (4000, 5000, 5300, 6300))
    assert want[0] > 0 and want[1] > 0

    class Without:
        def __getattr__(self, attr):
            if attr == "vapor_bam_depth":
                raise AssertionError("the library is not asked")
            return getattr(real, attr)
    real = L.load()
    monkeypatch.setattr(L, "_lib", Without())
    assert b.depth_native(0, (52000, 52300, 52700, 53000)) == [0, 0, 0]
    assert b.depth_native(0, (4000, 5000, 5300, 6300), []) == [0, 0, 0]
    monkeypatch.setattr(L, "_lib", real)
    b.close()


@pytest.mark.parametrize("name", ["signatures", "links", "support"])
def test_the_other_native_readers_refuse_a_region_in_the_librarys_words_also_without_a_chunk(name, pattern):
    b = bamio.BamFile(pattern.replace("XXX", "one"))
    mod = MODULES[name]
    entry = {"signatures": "vapor_bam_signature", "links": "vapor_bam_links", "support": "vapor_bam_support"}[name]
    native = getattr(b, {"signatures": "signature_native", "links": "links_native", "support": "support_native"}[name])
    more = (b"c",) if name == "links" else ()

    def row(w0, w3, x, tol):
        if name == "links":
            return [w0, w3, x, x + 300, tol, 30, 1, 0, 0, 0, 1]
        return [w0, w3, x, x + 300, tol, 30, 0, 0, 3] + ([51, 30] if name == "support" else [])
    assert mod.TOL_MAX == 255
    for w0, w3, x in ((4900, 5400, 5000), (52000, 52400, 52100)):          # chunks overlap the first, none the second
        assert bool(b.index.chunks(0, w0, w3)) == (w0 == 4900)
        good = native(0, row(w0, w3, x, 50), None, *more)
        assert len(good) == len(ZERO[name]) and (any(good) == (w0 == 4900))
        for chunks in (None, []):
            with pytest.raises(ValueError, match=entry):
                native(0, row(w0, w3, x, mod.TOL_MAX + 1), chunks, *more)
    b.close()
