"""`--realign-revote` on the device (vapor_realign_revote - the polish's six kernels, then spell_kernel,
spell_pack_kernel and realign_onto_kernel) against the plain-integer model of tests/revote_model.py, exact in vout, lout and
spelt, its polish outputs equal to vapor_realign_polish's on the same input: the designed loci (polished lengths at nibble, word
and chunk edges, flagged columns across a round of 256, more than 256 sites, every compiled width), a seeded fuzz, spelt == NULL,
an allele as bytes, as a derived sequence and as an upper-cased twin, reads from device-held BAM bases, the call's shapes and
refusals, a short spelt slot, the budget at its floor, a locus whose polished allele is one symbol too long, and the CLI's table,
VCF and files on a small world in memory."""
import numpy as np
import pytest

import plane_model as PM
import revote_model as M
import test_gpu_junction as TGJ
import test_gpu_polish as TGP
import test_gpu_realign as TG
import test_gpu_trace as TT
import test_polish_cpu as TP
import test_revote_cpu as TRV
import test_signature_cpu as TS
from vapor_amd import _lib as L
from vapor_amd import bamio, pipeline, polish, revote, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def tables(loci):
    """(seqs, rows, first, col_off, votes, vfirst) of loci [(name, pairs, votes, allele, band)] for one call: per locus its allele,
    then its piled reads, then the reads of its vote pairs."""
    seqs, rows, first, col_off, votes, vfirst = [], [], [0], [0], [], [0]
    for _name, pairs, vs, allele, _band in loci:
        a = len(seqs)
        seqs.append(allele.decode("latin-1"))
        for read, off2 in pairs:
            rows.append((len(seqs), a, off2, 0, 0))
            seqs.append(read.decode("latin-1"))
        for read, off2 in vs:
            votes.append((len(seqs), a, off2, 0, 0))
            seqs.append(read.decode("latin-1"))
        first.append(len(rows))
        vfirst.append(len(votes))
        col_off.append(col_off[-1] + len(allele))
    return seqs, rows, first, col_off, votes, vfirst


def per_locus(got, vfirst):
    """[(lout, vout, spelt)] of what Engine.realign_revote returns; spelt None without the output, what lies behind plen must be 0."""
    vout, lout, so, spelt = got[5:]
    out = []
    for g in range(len(lout)):
        text = None
        if spelt is not None:
            plen = int(lout[g][1])
            end = int(so[g + 1]) if g + 1 < len(so) else len(spelt)
            assert not spelt[int(so[g]) + plen:end].any()
            text = spelt[int(so[g]):int(so[g]) + plen].tolist()
        out.append((lout[g].tolist(), vout[vfirst[g]:vfirst[g + 1]].tolist(), text))
    return out


def same_polish(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4])) and (want[4] is None or np.array_equal(got[4], want[4]))


def device(eng, loci, want_spelt=True):
    """Per locus (lout, vout, spelt); the polish outputs of every call are held to Engine.realign_polish's on the same input."""
    out = [None] * len(loci)
    for band in sorted({l[4] for l in loci}):
        idx = [t for t, l in enumerate(loci) if l[4] == band]
        seqs, rows, first, col_off, votes, vfirst = tables([loci[t] for t in idx])
        ss = eng.seqset(seqs)
        try:
            got = eng.realign_revote(ss, eng.make_pairs(rows), band, first, col_off, eng.make_pairs(votes), vfirst, True, want_spelt)
            assert same_polish(got, eng.realign_polish(ss, eng.make_pairs(rows), band, first, col_off, True)), band
        finally:
            ss.close()
        for t, g in zip(idx, per_locus(got, vfirst)):
            out[t] = g
    return out


def wrong(loci, got, expect, spelt=True):
    return [(l[0], g[0], e[0]) for l, g, e in zip(loci, got, expect)
            if (g[0], g[1]) != (e[0], e[1]) or (spelt and g[2] != e[2])]


def test_designed_loci_equal_the_model(eng):
    loci, expect = M.designed_loci(), M.designed_expected()
    assert {l[4] for l in loci} >= {1, 2, 31, 32, 33, 100, 256, 512} and {e[0][1] for e in expect} >= {7, 8, 9, 31, 32, 33, 63, 64, 65, 1456}
    bad = wrong(loci, device(eng, loci), expect)
    assert not bad, (len(bad), bad[:5])
    # spelt == NULL: the other outputs are the same
    bad = wrong(loci, device(eng, loci, want_spelt=False), expect, spelt=False)
    assert not bad, (len(bad), bad[:5])


def test_seeded_fuzz_equals_the_model(eng):
    loci = M.fuzz_loci()
    assert len(loci) == 40
    expect = [M.revote(l[2], l[3], l[4], M.polish_of(l)) for l in loci]
    bad = wrong(loci, device(eng, loci), expect)
    assert not bad, (len(bad), bad[:5])


def _stated(reads, votes, allele, band, upper=False):
    """(lout, vout, spelt) of a locus by polish.statement and revote.statement."""
    _counts, calls, sites, ins, _stats = polish.statement(reads, allele, band)
    lout, vout, spelt, _own = revote.statement(votes, allele, calls, sites, ins, band, upper)
    return lout.tolist(), vout.tolist(), spelt.tolist()


def test_an_allele_as_bytes_as_a_derived_sequence_and_as_an_upper_cased_twin(eng):
    """The same locus four times in one call: the allele as bytes, described by segments of a window (one reverse-complemented),
    as a derived twin of the bytes and as an upper-cased twin, which spells what its plane holds."""
    rng = np.random.default_rng(3)
    window = "".join("ACGTacgtN"[j] for j in rng.integers(0, 9, 700))
    segs = [(0, 0, 210, False), (0, 333, 97, True), (0, 500, 200, False)]
    text = PM.spell([window.encode()], segs).decode()
    reads = [(text[5:150] + text[160:400] + "ACGTT" + text[400:], 5), (text[:150] + text[160:400] + "ACGTT" + text[400:], 0), (text[100:], 97),
             (text[40:150] + text[160:400] + "ACGTT" + text[400:480], 33)]      # (three of four lack ten bases and carry five more)
    votes = reads + [(text[150:260], 150), (text[401:470], 400), ("ACGT", len(text)), (text[:80], 0)]
    seqs = [window, text] + [r for r, _o in votes]
    ss = eng.seqset(seqs, None, [(segs, False), ([(1, 0, len(text), False)], False), ([(1, 0, len(text), False)], True)])
    n_lit = len(seqs)
    try:
        for band in (31, 256):
            alleles = (1, n_lit, n_lit + 1, n_lit + 2)
            rows = [(2 + k, a, o, 0, 0) for a in alleles for k, (_r, o) in enumerate(reads)]
            vrows = [(2 + k, a, o, 0, 0) for a in alleles for k, (_r, o) in enumerate(votes)]
            first, vfirst = [4 * g for g in range(5)], [len(votes) * g for g in range(5)]
            col_off = [len(text) * g for g in range(5)]
            got = eng.realign_revote(ss, eng.make_pairs(rows), band, first, col_off, eng.make_pairs(vrows), vfirst, True, True)
            assert same_polish(got, eng.realign_polish(ss, eng.make_pairs(rows), band, first, col_off, True))
            mine = per_locus(got, vfirst)
            want, upper = _stated(reads, votes, text, band), _stated(reads, votes, text, band, True)
            assert mine[:3] == [want] * 3 and mine[3] == upper, (band, mine[0][0], want[0])
            assert want[2] != upper[2] and want[1] == upper[1] and want[0][1] != len(text) and any(c >= 4 for c in want[2])
    finally:
        ss.close()


def test_reads_from_device_held_bam_bases(eng, tmp_path):
    """src_kind 1 of vapor_seqset_create_mixed: the reads never cross the link as text; their second vote is that of their texts
    uploaded as bytes, and the statement's."""
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
            got = eng.realign_revote(ss, eng.make_pairs(rows), 100, [0, n_dev, 2 * n_dev], col_off, eng.make_pairs(rows), [0, n_dev, 2 * n_dev],
                                     True, True)
            mine = per_locus(got, [0, n_dev, 2 * n_dev])
        finally:
            ss.close()
    finally:
        for bt in batches:
            bt.close()
    reads = [(t.decode("latin-1"), o) for t, o in zip(texts, offs)]
    want = _stated(reads, reads, allele.decode("latin-1"), 100)
    assert mine == [want, want] and want[0][1] == len(allele) - 2 + 10 and all(v[1] == 0 for v in want[1]), want[0]


def test_call_shapes_bad_pairs_short_slots_and_refusals(eng):
    base = [l for l in M.designed_loci() if l[4] == 100 and 0 < len(l[3]) <= 300]
    expect = {l[0]: M.revote(l[2], l[3], l[4], M.polish_of(l)) for l in base}

    def want_of(l):
        e = expect[l[0]]
        return (e[0], e[1], e[2])
    for n in (0, 1, 5, 60):
        loci = [base[(7 * t) % len(base)] for t in range(n)]
        seqs, rows, first, col_off, votes, vfirst = tables(loci)
        ss = eng.seqset(seqs or ["A"])
        try:
            got = per_locus(eng.realign_revote(ss, eng.make_pairs(rows), 100, first, col_off, eng.make_pairs(votes), vfirst, False, True), vfirst)
        finally:
            ss.close()
        assert len(got) == n and got == [want_of(l) for l in loci], n
    good = [base[3], base[7], base[12], base[20], base[25]]
    want = [want_of(l) for l in good]
    seqs, rows, first, col_off, votes, vfirst = tables(good)
    n_col = [len(l[3]) for l in good]
    ss = eng.seqset(seqs)
    try:
        pairs = eng.make_pairs(rows)

        def run(votes=votes, vfirst=vfirst, spelt_off=None, rows=rows, first=first):
            got = eng.realign_revote(ss, eng.make_pairs(rows), 100, first, col_off, eng.make_pairs(votes), vfirst, False, True, spelt_off)
            return per_locus(got, vfirst)
        # a locus without vote pairs is spelt all the same; no vote pair at all
        a, b = vfirst[1], vfirst[2]
        got = run(votes[:a] + votes[b:], vfirst[:2] + [v - (b - a) for v in vfirst[2:]])
        assert got == [want[0], (want[1][0], [], want[1][2])] + want[2:]
        got = run([], [0] * 6)
        assert got == [(w[0], [], w[2]) for w in want]
        # a locus without piled reads takes its allele from its vote pairs: nothing is called, the allele is spelt as it is
        a, b = first[3], first[4]
        got = run(rows=rows[:a] + rows[b:], first=first[:4] + [v - (b - a) for v in first[4:]])
        plain = M.revote(good[3][2], good[3][3], 100, M.pm.polish([], good[3][3], 100))
        assert got == want[:3] + [(plain[0], plain[1], plain[2])] + want[4:] and plain[0][1] == n_col[3]
        # bad vote pairs among good ones: off2 behind the allele, another seq2, a sequence that is none
        v3 = list(votes)
        k = vfirst[2]
        v3[k] = (v3[k][0], v3[k][1], n_col[2] + 1, 0, 0)
        v3[k + 1] = (v3[k + 1][0], votes[0][1], 0, 0, 0)
        v3[vfirst[4]] = (len(seqs), v3[vfirst[4]][1], 0, 0, 0)
        got = run(v3)
        refused = [-1, L.E_ARG, 0, 0]
        assert got[2] == (want[2][0], [refused, refused] + want[2][1][2:], want[2][2])
        assert got[4] == (want[4][0], [refused] + want[4][1][1:], want[4][2]) and got[:2] + got[3:4] == want[:2] + want[3:4]
        # off2 == len is legal
        assert all(any(o == len(l[3]) for _r, o in l[2]) for l in good) and all(v[1] == 0 for w in want for v in w[1])
        # a short spelt slot: that locus has vstatus E_ARG, its polish part is served, the others are written
        cap = [n + polish.RMAX * min(n, polish.MAX_SITES) for n in n_col]
        so = np.concatenate(([0], np.cumsum([cap[0], cap[1], cap[2] - 1, cap[3], cap[4]])))
        full = eng.realign_revote(ss, pairs, 100, first, col_off, eng.make_pairs(votes), vfirst, True, True, so)
        assert same_polish(full, eng.realign_polish(ss, pairs, 100, first, col_off, True))
        got = per_locus(full, vfirst)
        assert got[2] == ([L.E_ARG, want[2][0][1], 0, 0], [[-1, L.E_ARG, 0, 0]] * len(want[2][1]), [0] * want[2][0][1])
        assert got[:2] + got[3:] == want[:2] + want[3:]
        # the call-level refusals: the polish's, and the three of the second vote
        vp = eng.make_pairs(votes)
        for b in (0, -1, L.MAX_BAND + 1):
            with pytest.raises(L.VaporHipError) as e:
                eng.realign_revote(ss, pairs, b, first, col_off, vp, vfirst)
            assert e.value.code == L.E_ARG and "vapor_realign_revote: band outside 1 .. VAPOR_MAX_BAND" in str(e.value)
        with pytest.raises(L.VaporHipError) as e:
            eng.realign_revote(ss, pairs, 100, [1] + first[1:], col_off, vp, vfirst)
        assert e.value.code == L.E_ARG and "ascend from 0" in str(e.value)
        for vf in (vfirst[:-1] + [vfirst[-1] - 1], [1] + vfirst[1:], vfirst[:2] + [vfirst[1] - 1] + vfirst[3:]):
            with pytest.raises(L.VaporHipError) as e:
                eng.realign_revote(ss, pairs, 100, first, col_off, vp, vf)
            assert e.value.code == L.E_ARG and "vfirst must ascend from 0 to n_votes" in str(e.value)
        for bad in ([1] + so.tolist()[1:], so.tolist()[:2] + [int(so[1]) - 1] + so.tolist()[3:]):
            with pytest.raises(L.VaporHipError) as e:
                eng.realign_revote(ss, pairs, 100, first, col_off, vp, vfirst, False, True, bad)
            assert e.value.code == L.E_ARG and "spelt_off must ascend from 0" in str(e.value)
        fn = L.load().vapor_realign_revote
        none = [None] * 7
        assert fn(eng._ctx, ss._h, 0, None, 100, 0, *none, 0, *none[:6]) == 0
        assert fn(eng._ctx, ss._h, 0, None, 100, 0, *none, -1, *none[:6]) == L.E_ARG
        assert fn(eng._ctx, None, 0, None, 100, 0, *none, 0, *none[:6]) == L.E_ARG
        assert run() == want                                                       # (the context is as good as before)
    finally:
        ss.close()


def check_budget_at_its_floor(make_engine):
    """At the floor of trace_budget sixty small loci and, between small ones, twelve loci of six pairs of 4 000 rows at band 512,
    which fall into several groups: the default budget's answers, in the polish part and in the second vote."""
    rng = np.random.default_rng(21)
    base = [l for l in M.designed_loci() if l[4] == 100 and 0 < len(l[3]) <= 300]
    small = [base[(5 * t) % len(base)] for t in range(60)]
    allele = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 4040)
    truth = np.concatenate([allele[:1500], allele[1503:2500], np.frombuffer(b"GATTACA", dtype=np.uint8), allele[2500:]]).copy()
    reads = [(truth[k:4000 + k].tobytes(), k) for k in range(6)]
    votes = reads + [(truth[2000:2600].tobytes(), 2003), (allele[3000:3500].tobytes(), 3000)]
    long_locus = ("long", reads, votes, allele.tobytes(), 512)
    tiny = [(l[0], l[1], l[2], l[3], 512) for l in small[:4]]
    mixed = tiny[:2] + [long_locus] * 12 + tiny[2:]
    results = {}
    for budget in (None, 1):
        e = make_engine()
        try:
            if budget is not None:
                e.set_param("trace_budget", budget)          # (below the floor: raised to it)
            results[budget] = (device(e, small), device(e, mixed))
        finally:
            e.close()
    assert results[None] == results[1]
    assert results[1][0] == [tuple(M.revote(l[2], l[3], l[4], M.polish_of(l))[:3]) for l in small]
    d = results[None][1]
    want = _stated([(r.decode(), o) for r, o in reads], [(r.decode(), o) for r, o in votes], allele.tobytes().decode(), 512)
    assert all(g == want for g in d[2:14]) and want[0] == [0, 4040 - 3 + 7, 0, 0] and want[1][6][2:] == [2000, 4044 - 2000]


def test_the_budget_at_its_floor():
    check_budget_at_its_floor(lambda: Engine(0))


def test_a_polished_allele_one_symbol_too_long(eng):
    """One locus of 65 535 columns whose three reads insert one base: plen 65 536, vstatus E_ARG and every vote pair refused with
    it; the polish part is served, and the codes are spelt."""
    rng = np.random.default_rng(5)
    allele = rng.choice(np.frombuffer(b"ACG", dtype=np.uint8), 65535).tobytes()
    read = allele[:30000] + b"T" + allele[30000:]
    locus = ("too long", [(read[:65535], 0)] * 3, [(read[:65535], 0), (allele[65000:], 65000)], allele, 31)
    (lout, vout, spelt), = device(eng, [locus])
    assert lout == [L.E_ARG, 65536, 0, 0] and vout == [[-1, L.E_ARG, 0, 0]] * 2
    assert spelt == [M.rm.code(v) for v in read]


# ------------------------------------------------------------------------------------------------------------------------------
# through the CLI
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmd", ["bed", "vcf"])
def test_cli_on_a_world_in_memory(cmd, tmp_path, monkeypatch):
    """`vapor bed | vcf --realign --realign-polish --realign-junction --realign-revote --realign-out` on the seven loci of
    tests/test_gpu_realign.py against the same run with the statements in place of the engine's entries: identical table, VCF
    and files; the earlier columns and the files are those of the run without `--realign-revote`."""
    w = synth.make_support_world(seed=4, specs=TG.SPECS, layers=4, read_len=4000)
    text = synth.bed_text(w) if cmd == "bed" else synth.vcf_text(w)
    flags = ["--realign", "--realign-polish", "--realign-junction"]
    pipeline.set_engine(None)
    try:
        seqio.set_backend(seqio.MemorySamtools(w))
        before, _ = TS.run_main(tmp_path, "before", cmd, text, flags + ["--realign-out", str(tmp_path / "before_pre")])
        seqio.set_backend(seqio.MemorySamtools(w))
        table, annotated = TS.run_main(tmp_path, "dev", cmd, text, flags + ["--realign-revote", "--realign-out", str(tmp_path / "dev_pre")])
        TT._statement_engine(monkeypatch)
        monkeypatch.setattr(Engine, "realign_polish", TP.stated_polish)
        monkeypatch.setattr(Engine, "realign_junction", TGJ.TJ.stated_junction)
        monkeypatch.setattr(Engine, "realign_revote", TRV.stated_revote)
        seqio.set_backend(seqio.MemorySamtools(w))
        stated, stated_annotated = TS.run_main(tmp_path, "stated", cmd, text,
                                               flags + ["--realign-revote", "--realign-out", str(tmp_path / "stated_pre")])
    finally:
        seqio.set_backend(None)
        pipeline.set_engine(None)
    assert table == stated and annotated == stated_annotated
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-8:] == list(revote.COLUMNS)
    assert "\n".join("\t".join(r[:-8]) for r in rows) + "\n" == before
    for ext in (".sam", ".fa", ".pol.fa"):
        assert (tmp_path / ("dev_pre" + ext)).read_text() == (tmp_path / ("before_pre" + ext)).read_text() == (tmp_path / ("stated_pre" + ext)).read_text()
    assert sum(1 for r in rows[1:] if r[-1] != ".") >= 3 and any(r[-8:] == ["."] * 8 for r in rows[1:])
