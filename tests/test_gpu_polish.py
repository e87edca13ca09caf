"""`--realign-polish` on the device (vapor_realign_polish - the two trace kernels, then pileup_kernel,
consensus_kernel, pileup_ins_kernel and insert_kernel) against the plain-integer model of tests/polish_model.py, exact in counts,
calls, sites, ins and stats: the designed loci (alleles of 1, 63, 64, 65 and 300 columns, '=' runs of 64 and 65, bands 31, 100,
256 and 512, more than 256 sites), a seeded fuzz, an allele as bytes and as a derived sequence, reads from device-held BAM bases,
the call's shapes and refusals, counts == NULL, the budget at its floor with one group, several groups and a locus that does not
fit, and the CLI's files on a small world in memory."""
import ctypes

import numpy as np
import pytest

import plane_model as PM
import polish_model as M
import test_gpu_realign as TG
import test_gpu_trace as TT
import test_polish_cpu as TP
import test_signature_cpu as TS
from vapor_amd import _lib as L
from vapor_amd import bamio, pipeline, polish, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def tables(loci):
    """(seqs, rows, first, col_off) of loci [(name, pairs, allele, band)] for one call: per locus its allele, then its reads."""
    seqs, rows, first, col_off = [], [], [0], [0]
    for _name, pairs, allele, _band in loci:
        a = len(seqs)
        seqs.append(allele.decode("latin-1"))
        for read, off2 in pairs:
            rows.append((len(seqs), a, off2, 0, 0))
            seqs.append(read.decode("latin-1"))
        first.append(len(rows))
        col_off.append(col_off[-1] + len(allele))
    return seqs, rows, first, col_off


def per_locus(stats, calls, sites, ins, counts, col_off):
    """The model's shape of what Engine.realign_polish returns; what lies behind the kept sites and their texts must be 0."""
    out = []
    for g in range(len(stats)):
        a, b = col_off[g], col_off[g + 1]
        k = int(stats[g][polish.SITES])
        assert not sites[g][k:].any() and not ins[g][k:].any()
        texts = []
        for s in range(k):
            nb = int(sites[g][s][1])
            assert not ins[g][s][nb:].any()
            texts.append(bytes(ins[g][s][:nb]))
        out.append((counts[a:b].tolist() if counts is not None else None, calls[a:b].tolist(), sites[g][:k].tolist(), texts, stats[g].tolist()))
    return out


def device(eng, loci, want_counts=True):
    out = [None] * len(loci)
    for band in sorted({l[3] for l in loci}):
        idx = [t for t, l in enumerate(loci) if l[3] == band]
        seqs, rows, first, col_off = tables([loci[t] for t in idx])
        ss = eng.seqset(seqs)
        try:
            got = eng.realign_polish(ss, eng.make_pairs(rows), band, first, col_off, want_counts)
        finally:
            ss.close()
        for t, g in zip(idx, per_locus(*got, col_off)):
            out[t] = g
    return out


def wrong(loci, got, expect, counts=True):
    return [(l[0], g[4], e[4]) for l, g, e in zip(loci, got, expect) if (g if counts else g[1:]) != (tuple(e) if counts else tuple(e)[1:])]


def test_designed_loci_equal_the_model(eng):
    loci, expect = M.designed_loci(), M.designed_expected()
    assert {l[3] for l in loci} >= {31, 100, 256, 512} and {len(l[2]) for l in loci} >= {1, 63, 64, 65, 300}
    assert expect[-1][4][5] == M.MAX_SITES and expect[-1][4][7] > 0
    got = device(eng, loci)
    bad = wrong(loci, got, expect)
    assert not bad, (len(bad), bad[:5])
    # counts == NULL: the other outputs are the same
    bad = wrong(loci, device(eng, loci, want_counts=False), expect, counts=False)
    assert not bad, (len(bad), bad[:5])


def test_seeded_fuzz_equals_the_model(eng):
    loci = M.fuzz_loci()
    assert len(loci) == 40 and all(3 <= len(l[1]) <= 8 for l in loci)
    expect = [M.polish(*l[1:]) for l in loci]
    bad = wrong(loci, device(eng, loci), expect)
    assert not bad, (len(bad), bad[:5])


def test_an_allele_as_bytes_and_as_a_derived_sequence(eng):
    """The same locus three times in one call: the allele as bytes, described by segments of a window (one reverse-complemented),
    and as a derived twin of the bytes; against polish.statement (held to the model by tests/test_polish_cpu.py)."""
    rng = np.random.default_rng(3)
    window = "".join("ACGTacgtN"[j] for j in rng.integers(0, 9, 700))
    segs = [(0, 0, 210, False), (0, 333, 97, True), (0, 500, 200, False)]
    text = PM.spell([window.encode()], segs).decode()
    reads = [(text[5:150] + text[160:400] + "ACGTT" + text[400:], 5), (text[:300] + "ACGTT" + text[300:], 0), (text[100:], 97),
             (text[40:150] + text[160:400] + "ACGTT" + text[400:480], 33)]
    seqs = [window, text] + [r for r, _o in reads]
    ss = eng.seqset(seqs, None, [(segs, False), ([(1, 0, len(text), False)], False)])
    n_lit = len(seqs)
    try:
        for band in (31, 256):
            rows = [(2 + k, a, o, 0, 0) for a in (1, n_lit, n_lit + 1) for k, (_r, o) in enumerate(reads)]
            first, col_off = [0, 4, 8, 12], [0, len(text), 2 * len(text), 3 * len(text)]
            got = per_locus(*eng.realign_polish(ss, eng.make_pairs(rows), band, first, col_off, True), col_off)
            want = per_locus(*[np.asarray(v)[None] if k in (0, 2, 3) else v for k, v in enumerate(_stated(reads, text, band))], [0, len(text)])[0]
            assert got == [want] * 3 and want[4][polish.PCOV] > 400, (band, got[0][4], want[4])
    finally:
        ss.close()


def _stated(reads, allele, band):
    """polish.statement's five in Engine.realign_polish's order."""
    counts, calls, sites, ins, stats = polish.statement(reads, allele, band)
    return stats, calls, sites, ins, counts


def test_reads_from_device_held_bam_bases(eng, tmp_path):
    """src_kind 1 of vapor_seqset_create_mixed: the reads never cross the link as text; their pile is that of their texts
    uploaded as bytes, and the statement's.  The record holds all sixteen BAM codes."""
    rng = np.random.default_rng(12)
    nib = np.concatenate([rng.choice([1, 2, 4, 8], 300), rng.permutation(16), rng.choice([1, 2, 4, 8], 285)])
    p = str(tmp_path / "one.bam")
    bamio.write_bam(p, [("c", 9000)], [("r", 0, 100, "601M", "".join(PM.BAM_NIBBLES[j] for j in nib))])
    kf, addr, q0, _miss, status, batches = seqio.InProcessBam().chop_many_device(eng, p, ["c"], [101], [700], [100])
    try:
        assert int(kf[-1]) == 1 and status.tolist() == [0]
        spans = [(0, 601), (20, 500), (100, 501), (7, 300)]                 # (first, length) of the record's bases
        texts = [PM.bam_text(nib, f, n, 1) for f, n in spans]
        allele = PM.bam_text(nib, 0, 601, 1).replace(b"=", b"A")
        allele = allele[:250] + b"GG" + allele[250:400] + allele[410:]       # (the reads lack two bases and carry ten more)
        offs = [0, 15, 90, 0]
        host = [np.frombuffer(t, dtype=np.uint8).copy() for t in texts + [allele]]
        n_dev = len(spans)
        a = np.asarray([int(addr[0])] * n_dev + [h.ctypes.data for h in host], dtype=np.uint64)
        lens = np.asarray([s[1] for s in spans] + [len(h) for h in host], dtype=np.int64)
        kind = np.asarray([1] * n_dev + [0] * len(host), dtype=np.uint8)
        first = np.asarray([s[0] for s in spans] + [0] * len(host), dtype=np.int64)
        ss = eng.seqset_raw(a, lens, None, keepalive=host, src_kind=kind, src_first=first)
        try:
            al = 2 * n_dev
            rows = [(t, al, offs[t], 0, 0) for t in range(n_dev)] + [(n_dev + t, al, offs[t], 0, 0) for t in range(n_dev)]
            col_off = [0, len(allele), 2 * len(allele)]
            got = per_locus(*eng.realign_polish(ss, eng.make_pairs(rows), 100, [0, n_dev, 2 * n_dev], col_off, True), col_off)
        finally:
            ss.close()
    finally:
        for bt in batches:
            bt.close()
    reads = [(t.decode("latin-1"), o) for t, o in zip(texts, offs)]
    want = per_locus(*[np.asarray(v)[None] if k in (0, 2, 3) else v for k, v in enumerate(_stated(reads, allele.decode("latin-1"), 100))],
                     [0, len(allele)])[0]
    assert got == [want, want] and want[4][polish.PDEL] >= 2 and want[4][polish.PINS] >= 8, want[4]


def _refused(status, n_col):
    return ([[0] * 8] * n_col, [M.KEEP] * n_col, [], [], [status, 0, 0, 0, 0, 0, 0, 0])


def test_call_shapes_empty_and_refused_loci_and_refusals(eng):
    base = [l for l in M.designed_loci() if l[3] == 100]
    expect = [M.polish(*l[1:]) for l in base]
    for n in (0, 1, 5, 60):
        loci = [base[t % len(base)] for t in range(n)]
        seqs, rows, first, col_off = tables(loci)
        ss = eng.seqset(seqs or ["A"])
        try:
            got = per_locus(*eng.realign_polish(ss, eng.make_pairs(rows), 100, first, col_off, True), col_off)
        finally:
            ss.close()
        assert len(got) == n and got == [tuple(expect[t % len(base)]) for t in range(n)], n
    # an empty locus between full ones; a locus with a refused pair; one with two different seq2; one whose columns are not its
    # allele's length: each among good ones, which are served
    good = [base[3], base[7], base[12], base[20], base[25]]
    seqs, rows, first, col_off = tables(good)
    n_col = [len(l[2]) for l in good]
    want = [tuple(M.polish(*l[1:])) for l in good]
    ss = eng.seqset(seqs)
    try:
        a = first[1]
        # (locus 1 empty: its pairs go; its columns stay)
        r2 = rows[:a] + rows[first[2]:]
        f2 = first[:2] + [v - (first[2] - a) for v in first[2:]]
        got = per_locus(*eng.realign_polish(ss, eng.make_pairs(r2), 100, f2, col_off, True), col_off)
        assert got == [want[0], ([[0] * 8] * n_col[1], [M.KEEP] * n_col[1], [], [], [0] * 8)] + want[2:]
        for what in ("bad pair", "two seq2", "columns"):
            r3, c3 = list(rows), list(col_off)
            if what == "bad pair":
                r3[first[2] + 1] = (r3[first[2] + 1][0], r3[first[2] + 1][1], n_col[2] + 1, 0, 0)
            elif what == "two seq2":
                r3[first[3] - 1] = (r3[first[3] - 1][0], rows[0][1], 0, 0, 0)
            else:
                c3 = col_off[:3] + [v + 2 for v in col_off[3:]]
            got = per_locus(*eng.realign_polish(ss, eng.make_pairs(r3), 100, first, c3, True), c3)
            assert got == want[:2] + [_refused(L.E_ARG, c3[3] - c3[2])] + want[3:], what
        # the call-level refusals
        pairs = eng.make_pairs(rows)
        for b in (0, -1, L.MAX_BAND + 1):
            with pytest.raises(L.VaporHipError) as e:
                eng.realign_polish(ss, pairs, b, first, col_off)
            assert e.value.code == L.E_ARG and "band outside 1 .. VAPOR_MAX_BAND" in str(e.value)
        for f, c in ((first[:-1] + [first[-1] - 1], col_off), ([1] + first[1:], col_off), (first, [1] + col_off[1:]),
                     (first[:2] + [first[1] - 1] + first[3:], col_off), (first, col_off[:2] + [col_off[1] - 1] + col_off[3:])):
            with pytest.raises(L.VaporHipError) as e:
                eng.realign_polish(ss, pairs, 100, f, c)
            assert e.value.code == L.E_ARG and "ascend from 0" in str(e.value)
        fn = L.load().vapor_realign_polish
        assert fn(eng._ctx, ss._h, 0, None, 100, 0, None, None, None, None, None, None, None) == 0
        assert fn(eng._ctx, None, 0, None, 100, 0, None, None, None, None, None, None, None) == L.E_ARG
        got = per_locus(*eng.realign_polish(ss, pairs, 100, first, col_off, True), col_off)          # (the context is as good as before)
        assert got == want
    finally:
        ss.close()


def check_budget_at_its_floor(make_engine):
    """At the floor of trace_budget: 60 small loci, answered as at the default budget and as the model has them; twelve loci of
    six pairs of 4 000 rows at band 512 (2 MB of rows a pair) fall into several groups and one locus of seventy such pairs
    (140 MB of rows) is refused with E_NOMEM while its neighbours are served - all of it the default budget's answer, where the
    large locus is served."""
    rng = np.random.default_rng(21)
    base = [l for l in M.designed_loci() if l[3] == 100]
    small = [base[t % len(base)] for t in range(60)]
    want_small = [tuple(M.polish(*l[1:])) for l in small]
    allele = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 4040)
    truth = np.concatenate([allele[:1500], allele[1503:2500], np.frombuffer(b"GATTACA", dtype=np.uint8), allele[2500:]]).copy()
    truth[777] = ord("A") if truth[777] != ord("A") else ord("C")
    reads = []
    for k in range(6):
        r = truth[k:4000 + k].copy()
        r[97 + k::501] = ord("N")
        reads.append((r.tobytes(), k))
    long_locus = ("long", reads, allele.tobytes(), 512)
    huge = ("huge", [reads[k % 6] for k in range(70)], allele.tobytes(), 512)
    tiny = [(l[0], l[1], l[2], 512) for l in small[:4]]
    mixed = tiny[:2] + [long_locus] * 6 + [huge] + [long_locus] * 6 + tiny[2:]
    results = {}
    for budget in (None, 1):
        e = make_engine()
        try:
            if budget is not None:
                e.set_param("trace_budget", budget)          # (below the floor: raised to it)
            results[budget] = (device(e, small), device(e, mixed))
        finally:
            e.close()
    assert results[None][0] == results[1][0] == want_small
    d, f = results[None][1], results[1][1]
    assert f[8] == _refused(L.E_NOMEM, 4040) and d[8][4][0] == 0 and d[8][4][1] == 70
    assert f[:8] + f[9:] == d[:8] + d[9:]
    assert all(g == d[2] for g in d[2:8] + d[9:15]) and d[2][4][:2] == [0, 6]
    assert d[2][4][polish.PSUB] >= 1 and d[2][4][polish.PDEL] >= 3 and d[2][4][polish.PINS] >= 7
    assert d[:2] + d[15:] == [tuple(M.polish(*l[1:])) for l in tiny]


def test_the_budget_at_its_floor():
    check_budget_at_its_floor(lambda: Engine(0))


# ------------------------------------------------------------------------------------------------------------------------------
# through the CLI
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmd", ["bed", "vcf"])
def test_cli_on_a_world_in_memory(cmd, tmp_path, monkeypatch):
    """`vapor bed | vcf --realign --realign-polish --realign-out` on the seven loci of tests/test_gpu_realign.py against the same
    run with the engine's three entries replaced by the Python statements: identical table, SAM, FASTA and .pol.fa; SAM and FASTA
    are `--realign-out`'s own."""
    w = synth.make_support_world(seed=4, specs=TG.SPECS, layers=4, read_len=4000)
    text = synth.bed_text(w) if cmd == "bed" else synth.vcf_text(w)
    pipeline.set_engine(None)
    try:
        seqio.set_backend(seqio.MemorySamtools(w))
        plain, _ = TS.run_main(tmp_path, "plain", cmd, text, ["--realign", "--realign-out", str(tmp_path / "plain_pre")])
        seqio.set_backend(seqio.MemorySamtools(w))
        table, annotated = TS.run_main(tmp_path, "dev", cmd, text, ["--realign", "--realign-polish", "--realign-out", str(tmp_path / "dev_pre")])
        TT._statement_engine(monkeypatch)
        monkeypatch.setattr(Engine, "realign_polish", TP.stated_polish)
        seqio.set_backend(seqio.MemorySamtools(w))
        stated, stated_annotated = TS.run_main(tmp_path, "stated", cmd, text,
                                               ["--realign", "--realign-polish", "--realign-out", str(tmp_path / "stated_pre")])
    finally:
        seqio.set_backend(None)
        pipeline.set_engine(None)
    assert table == stated and annotated == stated_annotated
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-13:] == list(polish.COLUMNS)
    assert "\n".join("\t".join(r[:-6]) for r in rows) + "\n" == plain
    for ext in (".sam", ".fa"):
        assert (tmp_path / ("dev_pre" + ext)).read_text() == (tmp_path / ("plain_pre" + ext)).read_text() == (tmp_path / ("stated_pre" + ext)).read_text()
    pol = (tmp_path / "dev_pre.pol.fa").read_text()
    assert pol == (tmp_path / "stated_pre.pol.fa").read_text()
    n_loci = sum(1 for t, _s, _z in TG.SPECS if not (cmd == "vcf" and t == "TANDUP"))
    assert pol.count(">") == n_loci and all(ln.endswith("|POL") for ln in pol.splitlines()[0::2])
    assert any(r[-6] not in (".", "0") and r[-1] != "." for r in rows[1:])
