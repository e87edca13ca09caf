"""`--realign` on the device (vapor_realign_batch - realign_kernel, one wavefront a pair) against the plain-integer
model of tests/realign_model.py, exactly: the designed pairs (lane-ownership edges of the band, nibble, word and chunk edges of
off2, events of exactly B and of B + 1, ends on the last row or the last column only, the symbols that match nothing), every
source a sequence set has (bytes, derived sequences, device-held BAM bases), the call's shapes and refusals, one pair of 65 535
symbols, a seeded fuzz, and the CLI's tables on a small world in memory."""
import ctypes

import numpy as np
import pytest

import plane_model as PM
import realign_model as M
import test_signature_cpu as TS
from fake_engine import _materialise
from vapor_amd import _lib as L
from vapor_amd import bamio, pipeline, realign, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def device(eng, cases):
    """d of every case (name, read, allele, off2, band): one set and one call per band."""
    out = [None] * len(cases)
    for band in sorted({c[4] for c in cases}):
        idx = [t for t, c in enumerate(cases) if c[4] == band]
        seqs = [s.decode("latin-1") for t in idx for s in (cases[t][1], cases[t][2])]
        ss = eng.seqset(seqs)
        try:
            d, st = eng.realign(ss, eng.make_pairs([(2 * k, 2 * k + 1, cases[t][3], 0, 0) for k, t in enumerate(idx)]), band)
        finally:
            ss.close()
        assert st.tolist() == [0] * len(idx) and d.dtype == np.int32
        for t, v in zip(idx, d.tolist()):
            out[t] = v
    return out


def test_designed_pairs_equal_the_model(eng):
    cases, expect = M.designed_cases(), M.designed_expected()
    assert {c[4] for c in cases} >= set(M.BANDS) and len(cases) > 450
    got = device(eng, cases)
    wrong = [(c[0], g, e) for c, g, e in zip(cases, got, expect) if g != e]
    assert not wrong, wrong[:10]


def lane_widths(bands):
    """The compiled lane width each band runs at: the smallest of 1, 2, 3, 5, 9, 17 that deals its 2 B + 1 slots to 64 lanes."""
    return [min(w for w in (1, 2, 3, 5, 9, 17) if 64 * w >= 2 * band + 1) for band in bands]


def test_bands_on_both_sides_of_every_lane_width_equal_the_model(eng):
    cases = M.edge_band_cases()
    bands = sorted({c[4] for c in cases})
    assert bands == list(M.EDGE_BANDS) and lane_widths(bands) == list(M.EDGE_WIDTHS) and set(lane_widths(bands)) == {1, 2, 3, 5, 9, 17}
    got = device(eng, cases)
    wrong = [(c[0], g, M.distance(*c[1:])) for c, g in zip(cases, got) if g != M.distance(*c[1:])]
    assert not wrong, wrong[:10]


def test_seeded_fuzz_equals_the_model(eng):
    cases = M.fuzz_cases()
    assert len(cases) == 60 and all(len(c[1]) <= 300 and len(c[2]) <= 300 for c in cases)
    got = device(eng, cases)
    wrong = [(c[0], g, M.distance(*c[1:])) for c, g in zip(cases, got) if g != M.distance(*c[1:])]
    assert not wrong, wrong[:10]


def test_an_allele_as_bytes_and_as_a_derived_sequence(eng):
    """The same allele as bytes and described: segments of a window, one reverse-complemented, and an upper-cased twin."""
    rng = np.random.default_rng(3)
    window = "".join("ACGTacgtN"[j] for j in rng.integers(0, 9, 700))
    segs = [(0, 0, 210, False), (0, 333, 97, True), (0, 500, 200, False)]
    text = PM.spell([window.encode()], segs).decode()
    read = text[5:150] + text[160:400] + "ACGTT" + text[400:]
    seqs = [window, read, text, text.upper()]
    ss = eng.seqset(seqs, None, [(segs, False), (segs, True), ([(2, 0, len(text), False)], True)])
    try:
        for band, off2 in ((33, 5), (256, 0), (512, 7)):
            rows = [(1, a, off2, 0, 0) for a in (2, 4, 3, 5, 6)]        # bytes, derived; upper-cased bytes, derived, twin of the bytes
            d, st = eng.realign(ss, eng.make_pairs(rows), band)
            e = M.distance(read.encode(), text.encode(), off2, band)
            assert st.tolist() == [0] * 5 and d.tolist() == [e] * 5, (band, off2, d.tolist(), e)
    finally:
        ss.close()


def test_a_read_from_device_held_bam_bases(eng, tmp_path):
    """src_kind 1 and 2 of vapor_seqset_create_mixed: the read never crosses the link as text; its distance is the one of its text
    uploaded as bytes, and the model's.  The read holds all sixteen BAM codes ('=' matches nothing, the IUPAC codes neither)."""
    rng = np.random.default_rng(12)
    nib = np.concatenate([rng.choice([1, 2, 4, 8], 1500), rng.permutation(16), rng.integers(0, 16, 24), rng.choice([1, 2, 4, 8], 461)])
    assert set(nib.tolist()) == set(range(16))
    p = str(tmp_path / "one.bam")
    bamio.write_bam(p, [("c", 9000)], [("r", 0, 100, "2001M", "".join(PM.BAM_NIBBLES[j] for j in nib))])
    kf, addr, q0, _miss, status, batches = seqio.InProcessBam().chop_many_device(eng, p, ["c"], [101], [700], [100])
    try:
        assert int(kf[-1]) == 1 and int(q0[0]) == 0 and status.tolist() == [0]
        spans = [(1, 0, 2001), (1, 33, 900), (1, 1000, 1001), (2, 2000, 2001), (2, 1300, 777), (2, 64, 65)]      # (src_kind, first, length)
        texts = [PM.bam_text(nib, f, n, k) for k, f, n in spans]
        allele = PM.bam_text(nib, 0, 2001, 1).replace(b"=", b"A")
        allele = allele[:700] + allele[760:]                             # (the read carries 60 bases the allele lacks)
        rc_allele = bytes(PM._complementary(allele)[::-1])
        host = [np.frombuffer(t, dtype=np.uint8).copy() for t in texts + [allele, rc_allele]]
        n_dev = len(spans)
        a = np.asarray([int(addr[0])] * n_dev + [h.ctypes.data for h in host], dtype=np.uint64)
        lens = np.asarray([s[2] for s in spans] + [len(h) for h in host], dtype=np.int64)
        kind = np.asarray([s[0] for s in spans] + [0] * len(host), dtype=np.uint8)
        first = np.asarray([s[1] for s in spans] + [0] * len(host), dtype=np.int64)
        ss = eng.seqset_raw(a, lens, None, keepalive=host, src_kind=kind, src_first=first)
        try:
            al, rc = 2 * n_dev, 2 * n_dev + 1
            rows, expect = [], []
            for t, (k, f, n) in enumerate(spans):
                target, ttext = (al, allele) if k == 1 else (rc, rc_allele)
                off2 = f if k == 1 else 0
                off2 = min(off2, 690)
                rows += [(t, target, off2, 0, 0), (n_dev + t, target, off2, 0, 0)]
                expect.append(realign.statement(texts[t], ttext, off2, 256))
            d, st = eng.realign(ss, eng.make_pairs(rows), 256)
            assert st.tolist() == [0] * len(rows)
            assert d[0::2].tolist() == d[1::2].tolist() == expect, (d.tolist(), expect)
            assert M.distance(texts[5], rc_allele, 0, 256) == expect[5]      # (the statement, held to the model on the shortest)
        finally:
            ss.close()
    finally:
        for bt in batches:
            bt.close()


def test_call_shapes_bad_pairs_and_refusals(eng):
    rng = np.random.default_rng(8)
    cases = M.fuzz_cases(seed=5, count=40, max_len=120)
    seqs = [s.decode() for c in cases for s in (c[1], c[2])] + ["A" * 10, ""]
    ss = eng.seqset(seqs)
    n_seq = len(seqs)
    try:
        # n_pairs of 0, 1, one more than a workgroup's wavefronts, a few hundred: the same pairs give the same answers
        good = [(2 * (t % 40), 2 * (t % 40) + 1, cases[t % 40][3], 0, 0) for t in range(300)]
        band = 33
        expect = [M.distance(c[1], c[2], c[3], band) for c in cases]
        for n in (0, 1, 4, 5, 300):
            d, st = eng.realign(ss, eng.make_pairs(good[:n]), band)
            assert len(d) == len(st) == n and st.tolist() == [0] * n
            assert d.tolist() == [expect[t % 40] for t in range(n)], n
        # bad pairs among good ones: a bad one gets VAPOR_E_ARG and -1, a good one its d; k and flags are ignored
        bad = [(-1, 1, 0, 0, 0), (0, n_seq, 0, 0, 0), (n_seq, -5, 0, 0, 0), (0, 1, -1, 0, 0), (0, 1, len(seqs[1]) + 1, 0, 0),
               (0, n_seq - 2, 11, 0, 0)]
        edge = [(0, 1, len(seqs[1]), 77, 0xFFFFFFFF), (0, n_seq - 2, 10, -3, 9), (n_seq - 1, n_seq - 1, 0, 0, 0), (n_seq - 1, 0, 0, 0, 0)]
        rows, want = [], []
        for t in range(60):
            pick = int(rng.integers(0, 3))
            if pick == 0:
                rows.append(bad[t % len(bad)]); want.append((-1, L.E_ARG))
            elif pick == 1:
                rows.append(edge[t % len(edge)]); want.append((0, 0))            # (an empty side: nothing to pay)
            else:
                rows.append(good[t]); want.append((expect[t % 40], 0))
        d, st = eng.realign(ss, eng.make_pairs(rows), band)
        assert list(zip(d.tolist(), st.tolist())) == want
        # a sequence longer than VAPOR_MAX_SEQ_LEN on either side
        big = eng.seqset(["ACGT" * 16384, "ACGT" * 16384, "ACGTA" * 13108])
        try:
            assert [len(s) for s in ("ACGT" * 16384, "ACGTA" * 13108)] == [65536, 65540]
            d, st = eng.realign(big, eng.make_pairs([(0, 1, 0, 0, 0), (2, 2, 0, 0, 0)]), 2)
            assert d.tolist() == [-1, -1] and st.tolist() == [L.E_ARG, L.E_ARG]
        finally:
            big.close()
        # the call-level refusals
        for b in (0, -1, L.MAX_BAND + 1, 1 << 20):
            with pytest.raises(L.VaporHipError) as e:
                eng.realign(ss, eng.make_pairs(good[:3]), b)
            assert e.value.code == L.E_ARG and "band outside 1 .. VAPOR_MAX_BAND" in str(e.value)
        out = np.zeros(8, dtype=np.int32)
        pairs = eng.make_pairs(good[:3])
        assert L.load().vapor_realign_batch(eng._ctx, ss._h, -1, pairs.ctypes.data, 33, L.ptr(out, ctypes.c_int32)) == L.E_ARG
        assert L.load().vapor_realign_batch(eng._ctx, ss._h, 0, None, 33, None) == 0
        assert L.load().vapor_realign_batch(eng._ctx, None, 1, pairs.ctypes.data, 33, L.ptr(out, ctypes.c_int32)) == L.E_ARG
        d, st = eng.realign(ss, eng.make_pairs(good[:3]), L.MAX_BAND)             # (the context is as good as before)
        assert st.tolist() == [0, 0, 0] and d.tolist() == [M.distance(c[1], c[2], c[3], 512) for c in cases[:3]]
    finally:
        ss.close()


def test_one_long_pair(eng):
    """n = m = 65 535, B = 512, a planted deletion of 300 bases and a substitution every 1 000.  The model of this one case is the
    numpy statement (realign.statement), itself held to the plain model on the small cases by tests/test_realign_cpu.py: the plain
    model's full matrix of 4.3e9 cells is out of reach."""
    rng = np.random.default_rng(99)
    allele = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 65535 + 300)
    read = np.concatenate([allele[:30000], allele[30300:]]).copy()
    for p in range(500, 65535, 1000):
        read[p] = ord("A") if read[p] != ord("A") else ord("C")
    allele = allele[:65535]
    assert len(read) == len(allele) == L.MAX_SEQ_LEN
    r, a = read.tobytes().decode(), allele.tobytes().decode()
    ss = eng.seqset([r, a])
    try:
        d, st = eng.realign(ss, eng.make_pairs([(0, 1, 0, 0, 0)]), 512)
    finally:
        ss.close()
    e = realign.statement(r, a, 0, 512)
    print("one long pair: d = %d, statement %d" % (int(d[0]), e))
    assert st.tolist() == [0] and int(d[0]) == e and 300 <= e <= 300 + 66


# ------------------------------------------------------------------------------------------------------------------------------
# through the CLI
# ------------------------------------------------------------------------------------------------------------------------------
SPECS = (("DEL", 600, "hom"), ("DEL", 600, "ref"), ("INS", 250, "hom"), ("INV", 700, "hom"), ("INV", 700, "ref"), ("TANDUP", 300, "hom"),
         ("DEL", 12000, "hom"))
WANT_GT = {"hom": "1/1", "ref": "0/0"}
_stated = {}


def _statement_engine(monkeypatch):
    """Engine.realign replaced by the statement over the texts of the set (kept beside the set when it is made)."""
    orig = Engine.seqset

    def seqset(self, seqs, upper=None, derived=None):
        ss = orig(self, seqs, upper, derived)
        ss.texts = list(seqs) + _materialise(list(seqs), derived)
        return ss

    def stated(self, ss, pairs, band):
        d = np.zeros(len(pairs), dtype=np.int32)
        for t, p in enumerate(pairs):
            key = (ss.texts[p["seq1"]], ss.texts[p["seq2"]], int(p["off2"]), band)
            if key not in _stated:
                _stated[key] = realign.statement(*key)
            d[t] = _stated[key]
        return d, np.zeros(len(pairs), dtype=np.int32)
    monkeypatch.setattr(Engine, "seqset", seqset)
    monkeypatch.setattr(Engine, "realign", stated)


@pytest.mark.parametrize("cmd", ["bed", "vcf"])
def test_cli_on_a_world_in_memory(cmd, tmp_path, monkeypatch):
    """`vapor bed | vcf --realign` on a world of seven loci, all four types: the leading columns are the plain run's table byte for
    byte, the VaPoR_RA_* columns those of the same run with Engine.realign replaced by the Python statement (held to the plain
    model on the designed cases by tests/test_realign_cpu.py; the plain model itself needs minutes at these lengths), the hom loci
    1/1 and the ref loci 0/0 (tests/test_realign_cpu.py checks the same genotypes without a device)."""
    w = synth.make_support_world(seed=4, specs=SPECS, layers=4, read_len=4000)
    text = synth.bed_text(w) if cmd == "bed" else synth.vcf_text(w)
    pipeline.set_engine(None)
    calls = []
    orig = Engine.realign
    monkeypatch.setattr(Engine, "realign", lambda self, ss, pairs, band: calls.append(len(pairs)) or orig(self, ss, pairs, band))
    try:
        seqio.set_backend(seqio.MemorySamtools(w))
        plain, _ = TS.run_main(tmp_path, "plain", cmd, text)
        assert not calls and "VaPoR_RA" not in plain
        seqio.set_backend(seqio.MemorySamtools(w))
        table, annotated = TS.run_main(tmp_path, "dev", cmd, text, ["--realign"])
        assert calls and sum(calls) % 2 == 0
        _statement_engine(monkeypatch)
        seqio.set_backend(seqio.MemorySamtools(w))
        stated, _ = TS.run_main(tmp_path, "stated", cmd, text, ["--realign"])
    finally:
        seqio.set_backend(None)
        pipeline.set_engine(None)
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-7:] == list(realign.COLUMNS)
    assert "\n".join("\t".join(r[:-7]) for r in rows) + "\n" == plain
    assert table == stated
    by_contig = {(r[0] if cmd == "bed" else r[0].split(":")[0]): r[-7:] for r in rows[1:]}
    n_loci = 0
    for l, (t, _span, zyg) in zip(w.loci, SPECS):
        if cmd == "vcf" and t == "TANDUP":
            continue
        n_loci += 1
        cols = by_contig[l.chrom]
        diffs = [int(v) for v in cols[6].split(",")]
        assert cols == M.columns(diffs) and len(diffs) > 3 and cols[4] == WANT_GT[zyg], (l, cols)
    assert len(by_contig) == n_loci and sum(calls) == 2 * sum(len(c[6].split(",")) for c in by_contig.values())
    if cmd == "vcf":
        assert sum(ln.startswith("##INFO=<ID=VaPoR_RA_") for ln in annotated.splitlines()) == 7
        rec = {ln.split("\t")[2]: ln.split("\t")[7] for ln in annotated.splitlines() if not ln.startswith("#")}
        for l in w.loci:
            if l.svtype != "TANDUP":
                assert rec[l.svid].endswith("".join(";%s=%s" % kv for kv in zip(realign.COLUMNS, by_contig[l.chrom]) if kv[1] != "."))
