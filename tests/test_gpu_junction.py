"""`--realign-junction` on the device (vapor_realign_junction - junction_rows_kernel, junction_pick_kernel) against
the plain-integer model of tests/junction_model.py, exact in `out` and in `rows`: every designed pair at bands 1, 2, 31, 32, 33,
100, 256 and 512 (2B + 1 = 63, 65, 67 are lane-ownership edges), 60 fuzz pairs, rows == NULL, a sequence as bytes, as a derived
sequence with a reverse-complemented segment and as an upper-cased twin, the call's shapes with refused pairs among good ones,
the call-level refusals, lengths that end a sequence at a nibble, word and chunk edge (the backward pass reads from there), one
pair of 65 535 against 65 535 symbols at band 512, and the CLI's table and files on a small world in memory."""
import ctypes

import numpy as np
import pytest

import junction_model as M
import plane_model as PM
import test_gpu_realign as TG
import test_gpu_trace as TT
import test_junction_cpu as TJ
import test_polish_cpu as TP
import test_signature_cpu as TS
from vapor_amd import _lib as L
from vapor_amd import junction, pipeline, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def device(eng, pairs, band, want_rows=True):
    """[(out[1:7], rows)] of pairs [(name, s, l, ...)] in one call; every status 0 and every last word 0."""
    seqs, rows = [], []
    for _name, s, l, *_rest in pairs:
        rows.append((len(seqs), len(seqs) + 1, 0, 0, 0))
        seqs += [s.decode("latin-1"), l.decode("latin-1")]
    ss = eng.seqset(seqs)
    try:
        out, row_off, tab = eng.realign_junction(ss, eng.make_pairs(rows), band, want_rows)
    finally:
        ss.close()
    assert out[:, 0].tolist() == [0] * len(pairs) and out[:, 7].tolist() == [0] * len(pairs)
    if not want_rows:
        assert row_off is None and tab is None
        return [(tuple(o[1:7].tolist()), None) for o in out]
    assert [int(b - a) for a, b in zip(row_off[:-1], row_off[1:])] == [len(p[1]) + 1 for p in pairs]
    return [(tuple(o[1:7].tolist()), [tuple(r) for r in tab[a:b].tolist()]) for o, a, b in zip(out, row_off[:-1], row_off[1:])]


def wrong(pairs, got, expect):
    return [(p[0], g[0], e[0]) for p, g, e in zip(pairs, got, expect) if g != tuple(e)]


@pytest.mark.parametrize("band", M.BANDS)
def test_designed_pairs_equal_the_model_at_every_band(eng, band):
    pairs = M.designed_pairs()
    assert {len(p[1]) for p in pairs} >= set(M.LENGTHS) and len(pairs) >= 80
    bad = wrong(pairs, device(eng, pairs, band), M.expected_pairs(band))
    assert not bad, (band, len(bad), bad[:5])


def test_bands_on_both_sides_of_every_lane_width_equal_the_model(eng):
    """A jump of B and of B + 1 in the longer sequence at the bands around every step of the compiled lane widths, rows asked for."""
    bands = (31, 32, 63, 64, 95, 96, 159, 160, 287, 288, 512)
    widths = [min(w for w in (1, 2, 3, 5, 9, 17) if 64 * w >= 2 * band + 1) for band in bands]       # 2 B + 1 slots over 64 lanes
    assert widths == [1, 2, 2, 3, 3, 5, 5, 9, 9, 17, 17] and set(widths) == {1, 2, 3, 5, 9, 17}
    rng = np.random.default_rng(26)
    for band in bands:
        left, right = bytes(rng.choice(list(b"ACG"), 8).tolist()), bytes(rng.choice(list(b"ACG"), band + 20).tolist())
        pairs = [("jump of %d B=%d" % (extra, band), left + right, left + b"T" * extra + right, band) for extra in (band, band + 1)]
        bad = wrong(pairs, device(eng, pairs, band), [M.junction(s, l, band) for _n, s, l, _b in pairs])
        assert not bad, (band, len(bad), bad[:5])


def test_designed_pairs_at_their_own_band_and_without_rows(eng):
    pairs, expect = M.designed_pairs(), M.expected_pairs()
    got = {}
    for band in sorted({p[3] for p in pairs}):
        idx = [t for t, p in enumerate(pairs) if p[3] == band]
        full = device(eng, [pairs[t] for t in idx], band)
        bare = device(eng, [pairs[t] for t in idx], band, want_rows=False)            # rows == NULL: `out` is the same
        assert [g[0] for g in full] == [g[0] for g in bare], band
        got.update(zip(idx, full))
    bad = wrong(pairs, [got[t] for t in range(len(pairs))], expect)
    assert not bad, (len(bad), bad[:5])


def test_seeded_fuzz_equals_the_model(eng):
    pairs = M.fuzz_pairs()
    assert len(pairs) == 60
    for band in sorted({p[3] for p in pairs}):
        mine = [p for p in pairs if p[3] == band]
        bad = wrong(mine, device(eng, mine, band), [M.junction(s, l, band) for _n, s, l, _b in mine])
        assert not bad, (band, len(bad), bad[:5])


def test_sequence_ends_at_nibble_word_and_chunk_edges(eng):
    """The backward pass starts at a sequence's last symbol, wherever in a word of the 4-bit plane it stands: every ns and nl
    around 8 (a word) and 32 (a chunk), the longer sequence up to 70 symbols beyond the shorter's end."""
    rng = np.random.default_rng(19)
    base = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), 200, p=[.2, .2, .2, .2, .04, .04, .04, .04, .04]))
    pairs = []
    for ns in (1, 6, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 95, 96, 97):
        for extra in (0, 1, 7, 8, 9, 31, 32, 33, 70):
            cut = ns // 2
            s = base[:ns]
            l = s[:cut] + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), extra)) + s[cut:]
            pairs.append(("ns=%d nl=%d" % (ns, ns + extra), s, l))
    for band in (2, 33):
        bad = wrong(pairs, device(eng, pairs, band), [M.junction(s, l, band) for _n, s, l in pairs])
        assert not bad, (band, len(bad), bad[:5])


def test_a_sequence_as_bytes_as_a_derived_sequence_and_as_an_upper_cased_twin(eng):
    """The same pair five ways in one call: the longer sequence as bytes, described by segments of a window (one
    reverse-complemented), as a derived twin of the bytes and as their upper-cased twin, and the shorter one upper-cased too;
    against junction.junction (held to the model by tests/test_junction_cpu.py).  Case never matters, so all five agree."""
    rng = np.random.default_rng(3)
    window = "".join("ACGTacgtN"[j] for j in rng.integers(0, 9, 700))
    segs = [(0, 0, 210, False), (0, 333, 97, True), (0, 500, 200, False)]
    text = PM.spell([window.encode()], segs).decode()
    short = text[:180] + text[251:300] + "G" + text[300:]
    seqs = [window, text, short]
    n_lit = len(seqs)
    ss = eng.seqset(seqs, None, [(segs, False), ([(1, 0, len(text), False)], False), ([(1, 0, len(text), False)], True),
                                 ([(2, 0, len(short), False)], True)])
    try:
        for band in (31, 256):
            rows = [(2, 1, 0, 0, 0), (2, n_lit, 0, 0, 0), (2, n_lit + 1, 0, 0, 0), (2, n_lit + 2, 0, 0, 0), (n_lit + 3, n_lit, 0, 0, 0)]
            out, row_off, tab = eng.realign_junction(ss, eng.make_pairs(rows), band, True)
            want, want_rows = junction.junction(short, text, band, True)
            # (the planted jump is found; an N matches nothing, so every N of the shorter sequence and the planted G cost 1)
            assert want[1:4] == (180, 180, 251) and want[0] == short.count("N") + 1
            for t in range(len(rows)):
                assert out[t].tolist() == [0] + list(want) + [0], (band, t)
                assert np.array_equal(tab[row_off[t]:row_off[t + 1]], want_rows), (band, t)
    finally:
        ss.close()


def test_call_shapes_refused_pairs_and_refusals(eng):
    good = M.fuzz_pairs(seed=5, count=40, max_len=120)
    seqs = [s.decode("latin-1") for p in good for s in (p[1], p[2])] + ["A" * 10, "", "ACGT"]
    n_seq = len(seqs)
    want = [M.junction(s, l, 33) for _n, s, l, _b in good]
    ss = eng.seqset(seqs)
    try:
        for n in (0, 1, 5, 300):
            rows, expect = [], []
            for t in range(n):
                g = t % len(good)
                kind = t % 7 if n >= 5 else 0
                if kind == 3:
                    rows.append((2 * g, 2 * g + 1, 1, 0, 0))                   # off2 != 0
                elif kind == 4:
                    rows.append((n_seq - 3, n_seq - 1, 0, 0, 0))               # len(seq1) > len(seq2)
                elif kind == 5:
                    rows.append((2 * g, n_seq + (t % 3) - 1 if t % 3 else -1, 0, 0, 0))      # an index outside the set
                else:
                    rows.append((2 * g, 2 * g + 1, 0, 0, 0))
                expect.append(None if kind in (3, 4, 5) else want[g])
            out, row_off, tab = eng.realign_junction(ss, eng.make_pairs(rows), 33, True)
            assert len(out) == n and len(row_off) == n + 1
            for t, e in enumerate(expect):
                if e is None:
                    assert out[t].tolist() == [L.E_ARG, 0, 0, 0, 0, 0, 0, 0], (n, t)
                else:
                    assert out[t].tolist() == [0] + list(e[0]) + [0], (n, t)
                    assert [tuple(r) for r in tab[row_off[t]:row_off[t] + len(e[1])].tolist()] == e[1], (n, t)
        # an empty shorter sequence against an empty longer one; against a longer one
        out, row_off, tab = eng.realign_junction(ss, eng.make_pairs([(n_seq - 2, n_seq - 2, 0, 0, 0), (n_seq - 2, n_seq - 1, 0, 0, 0)]), 2, True)
        assert out.tolist() == [[0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 4, 0, 0, 0]] and tab.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]
        # the call-level refusals
        pairs = eng.make_pairs([(0, 1, 0, 0, 0), (2, 3, 0, 0, 0)])
        for b in (0, -1, L.MAX_BAND + 1):
            with pytest.raises(L.VaporHipError) as e:
                eng.realign_junction(ss, pairs, b)
            assert e.value.code == L.E_ARG and "band outside 1 .. VAPOR_MAX_BAND" in str(e.value)
        fn = L.load().vapor_realign_junction
        i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
        out = np.zeros((2, 8), dtype=np.int32)
        rows = np.zeros((1000, 4), dtype=np.int32)
        po, pr = out.ctypes.data_as(i32p), rows.ctypes.data_as(i32p)
        assert fn(eng._ctx, ss._h, 0, None, 33, None, None, None) == 0
        assert fn(eng._ctx, None, 0, None, 33, None, None, None) == L.E_ARG
        assert fn(eng._ctx, ss._h, -1, pairs.ctypes.data, 33, po, None, None) == L.E_ARG
        assert fn(eng._ctx, ss._h, 2, pairs.ctypes.data, 33, None, None, None) == L.E_ARG
        for off in ([1, 400, 800], [0, 400, 399]):                              # a row table that does not ascend from 0
            ro = np.asarray(off, dtype=np.int64)
            assert fn(eng._ctx, ss._h, 2, pairs.ctypes.data, 33, po, ro.ctypes.data_as(i64p), pr) == L.E_ARG
        assert fn(eng._ctx, ss._h, 2, pairs.ctypes.data, 33, po, None, pr) == L.E_ARG           # rows without a row table
        # a slot of fewer than ns + 1 rows refuses its pair alone
        ro = np.asarray([0, len(good[0][1]), 800], dtype=np.int64)
        assert fn(eng._ctx, ss._h, 2, pairs.ctypes.data, 33, po, ro.ctypes.data_as(i64p), pr) == 0
        assert out[0].tolist() == [L.E_ARG, 0, 0, 0, 0, 0, 0, 0] and out[1].tolist() == [0] + list(want[1][0]) + [0]
        assert not rows[:int(ro[1])].any() and [tuple(r) for r in rows[int(ro[1]):int(ro[1]) + len(want[1][1])].tolist()] == want[1][1]
        got, _o, _r = eng.realign_junction(ss, pairs, 33)                       # (the context is as good as before)
        assert got.tolist() == [[0] + list(want[t][0]) + [0] for t in (0, 1)]
    finally:
        ss.close()


def check_tables_beyond_the_budget_refuse_the_call(make_engine):
    """16 (ns + 1) bytes a pair: 65 pairs of 65 535 rows are 68 MB, above the floor of trace_budget (64 MiB) and below its default."""
    rng = np.random.default_rng(4)
    s = "".join("ACGT"[j] for j in rng.integers(0, 4, 65535))
    e = make_engine()
    try:
        ss = e.seqset([s[:40], s[:60], s])
        try:
            many = e.make_pairs([(2, 2, 0, 0, 0)] * 65)
            e.set_param("trace_budget", 1)                      # (below the floor: raised to it)
            with pytest.raises(L.VaporHipError) as err:
                e.realign_junction(ss, many, 1)
            assert err.value.code == L.E_NOMEM and "trace_budget" in str(err.value)
            out, _o, _r = e.realign_junction(ss, e.make_pairs([(0, 1, 0, 0, 0)]), 1)          # (the context is as good as before)
            assert out[0].tolist() == [0] + list(junction.junction(s[:40], s[:60], 1)) + [0]
        finally:
            ss.close()
    finally:
        e.close()


def test_tables_beyond_the_budget_refuse_the_call():
    check_tables_beyond_the_budget_refuse_the_call(lambda: Engine(0))


def test_one_pair_of_65535_against_65535_symbols(eng):
    """The longest pair the entry takes, at band 512, with a planted jump of 3 000 symbols: against junction.junction (held to
    the model on the small cases by tests/test_junction_cpu.py), in `out` and in all 65 536 rows.  And the event such a jump
    stands for, a window of 65 535 symbols against its allele 3 000 shorter: found exactly."""
    rng = np.random.default_rng(6)
    l = "".join("ACGT"[j] for j in rng.integers(0, 4, 65535))
    tail = "".join("ACGT"[j] for j in rng.integers(0, 4, 3000))
    allele = l[:30011] + l[33011:]
    s = allele + tail
    assert len(s) == len(l) == 65535
    ss = eng.seqset([s, l, allele])
    try:
        out, row_off, tab = eng.realign_junction(ss, eng.make_pairs([(0, 1, 0, 0, 0), (2, 1, 0, 0, 0)]), 512, True)
    finally:
        ss.close()
    want, want_rows = junction.junction(s, l, 512, True)
    assert out[0].tolist() == [0] + list(want) + [0]
    assert np.array_equal(tab[:65536], want_rows)
    cost, i, j1, j2 = out[1, 1:5].tolist()
    assert (cost, j2 - j1) == (0, 3000) and i == j1 <= 30011 and l[j1:30011] == l[j1 + 3000:33011]       # (left-normalised)


# ------------------------------------------------------------------------------------------------------------------------------
# through the CLI
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmd", ["bed", "vcf"])
def test_cli_on_a_world_in_memory(cmd, tmp_path, monkeypatch):
    """`vapor bed | vcf --realign --realign-polish --realign-junction --realign-out` on the seven loci of
    tests/test_gpu_realign.py against the same run with the engine's four entries replaced by the Python statements: identical
    table, annotated VCF, SAM, FASTA and .pol.fa; the three files and the leading columns are `--realign-polish`'s own."""
    w = synth.make_support_world(seed=4, specs=TG.SPECS, layers=4, read_len=4000)
    text = synth.bed_text(w) if cmd == "bed" else synth.vcf_text(w)
    opts = ["--realign", "--realign-polish", "--realign-junction", "--realign-out"]
    pipeline.set_engine(None)
    try:
        seqio.set_backend(seqio.MemorySamtools(w))
        plain, _ = TS.run_main(tmp_path, "plain", cmd, text, ["--realign", "--realign-polish", "--realign-out", str(tmp_path / "plain_pre")])
        seqio.set_backend(seqio.MemorySamtools(w))
        table, annotated = TS.run_main(tmp_path, "dev", cmd, text, opts + [str(tmp_path / "dev_pre")])
        TT._statement_engine(monkeypatch)
        monkeypatch.setattr(Engine, "realign_polish", TP.stated_polish)
        monkeypatch.setattr(Engine, "realign_junction", TJ.stated_junction)
        seqio.set_backend(seqio.MemorySamtools(w))
        stated, stated_annotated = TS.run_main(tmp_path, "stated", cmd, text, opts + [str(tmp_path / "stated_pre")])
    finally:
        seqio.set_backend(None)
        pipeline.set_engine(None)
    assert table == stated and annotated == stated_annotated
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-19:] == list(junction.COLUMNS)
    assert "\n".join("\t".join(r[:-6]) for r in rows) + "\n" == plain
    for ext in (".sam", ".fa", ".pol.fa"):
        assert (tmp_path / ("dev_pre" + ext)).read_text() == (tmp_path / ("plain_pre" + ext)).read_text() == (tmp_path / ("stated_pre" + ext)).read_text()
    lensed = [r[-6:] for r in rows[1:] if r[-6] != "."]
    assert lensed and any(s[0] == "DEL" and s[1] == s[2] and s[3:] == ["0", "0", "0"] for s in lensed), lensed
    if cmd == "vcf":
        assert "##INFO=<ID=VaPoR_RA_JLEN," in annotated and "VaPoR_RA_JT=DEL" in annotated
