"""`--realign-out` on the device (vapor_realign_trace - realign_trace_kernel and traceback_kernel, one wavefront a
pair each) against the plain-integer model of tests/trace_model.py, run for run: the designed pairs at every compiled lane width,
a seeded fuzz, an allele as bytes and as a derived sequence, the call's shapes, bad pairs and refusals, cap_runs at 1, at exactly
n_runs and one below it, the workspace budget at its floor with several groups, d equal to vapor_realign_batch's on all of it,
one pair of 65 535 symbols, and the CLI's files on a small world in memory."""
import ctypes
import re

import numpy as np
import pytest

import plane_model as PM
import realign_model as RM
import test_gpu_realign as TG
import test_signature_cpu as TS
import trace_model as M
from vapor_amd import _lib as L
from vapor_amd import pipeline, realign, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def unpack(head, runs):
    """Per pair (d, status, i_end, j_end, runs) from what Engine.realign_trace returns; the head's last three words are 0."""
    assert head.dtype == np.int32 and runs.dtype == np.uint32 and not head[:, 5:].any()
    return [(int(h[0]), int(h[1]), int(h[2]), int(h[3]), realign.runs_of(h, r) if h[1] == 0 else int(h[4])) for h, r in zip(head, runs)]


def device(eng, cases, cap=None):
    """(d, i_end, j_end, runs) of every case (name, read, allele, off2, band): one set and one call per band; d is held to
    vapor_realign_batch's on the way."""
    out = [None] * len(cases)
    for band in sorted({c[4] for c in cases}):
        idx = [t for t, c in enumerate(cases) if c[4] == band]
        seqs = [s.decode("latin-1") for t in idx for s in (cases[t][1], cases[t][2])]
        ss = eng.seqset(seqs)
        try:
            pairs = eng.make_pairs([(2 * k, 2 * k + 1, cases[t][3], 0, 0) for k, t in enumerate(idx)])
            head, runs = eng.realign_trace(ss, pairs, band, cap or max(len(cases[t][1]) + len(cases[t][2]) + 1 for t in idx))
            d, st = eng.realign(ss, pairs, band)
        finally:
            ss.close()
        assert st.tolist() == [0] * len(idx) and d.tolist() == head[:, 0].tolist()
        for t, g in zip(idx, unpack(head, runs)):
            assert g[1] == 0, (cases[t][0], g)
            out[t] = (g[0], g[2], g[3], g[4])
    return out


def test_designed_pairs_equal_the_model_run_for_run(eng):
    cases, expect = M.designed_cases(), M.designed_expected()
    assert {c[4] for c in cases} >= set(RM.BANDS) and len(cases) > 500
    got = device(eng, cases)
    wrong = [(c[0], g, e[:4]) for c, g, e in zip(cases, got, expect) if g != tuple(e[:4])]
    assert not wrong, (len(wrong), wrong[:5])


def test_bands_on_both_sides_of_every_lane_width_equal_the_model_run_for_run(eng):
    cases = RM.edge_band_cases()
    bands = sorted({c[4] for c in cases})
    widths = [min(w for w in (1, 2, 3, 5, 9, 17) if 64 * w >= 2 * band + 1) for band in bands]       # 2 B + 1 slots over 64 lanes
    assert bands == list(RM.EDGE_BANDS) and widths == list(RM.EDGE_WIDTHS) and set(widths) == {1, 2, 3, 5, 9, 17}
    got = device(eng, cases)
    expect = [tuple(M.trace(*c[1:])[:4]) for c in cases]
    wrong = [(c[0], g, e) for c, g, e in zip(cases, got, expect) if g != e]
    assert not wrong, (len(wrong), wrong[:5])


def test_seeded_fuzz_equals_the_model(eng):
    cases = RM.fuzz_cases()
    assert len(cases) == 60
    got = device(eng, cases)
    wrong = [(c[0], g, M.trace(*c[1:])[:4]) for c, g in zip(cases, got) if g != tuple(M.trace(*c[1:])[:4])]
    assert not wrong, (len(wrong), wrong[:5])


def test_an_allele_as_bytes_and_as_a_derived_sequence(eng):
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
            got = unpack(*eng.realign_trace(ss, eng.make_pairs(rows), band, 2000))
            e = M.trace(read.encode(), text.encode(), off2, band)
            assert got == [(e[0], 0, e[1], e[2], e[3])] * 5, (band, off2, got[0], e)
    finally:
        ss.close()


def test_call_shapes_bad_pairs_and_refusals(eng):
    rng = np.random.default_rng(8)
    cases = RM.fuzz_cases(seed=5, count=40, max_len=120)
    seqs = [s.decode() for c in cases for s in (c[1], c[2])] + ["A" * 10, ""]
    ss = eng.seqset(seqs)
    n_seq = len(seqs)
    band = 33
    try:
        good = [(2 * (t % 40), 2 * (t % 40) + 1, cases[t % 40][3], 0, 0) for t in range(300)]
        expect = [M.trace(c[1], c[2], c[3], band) for c in cases]
        want_good = [(e[0], 0, e[1], e[2], e[3]) for e in expect]
        for n in (0, 1, 5, 300):
            head, runs = eng.realign_trace(ss, eng.make_pairs(good[:n]), band, 250)
            assert len(head) == len(runs) == n and unpack(head, runs) == [want_good[t % 40] for t in range(n)], n
        bad = [(-1, 1, 0, 0, 0), (0, n_seq, 0, 0, 0), (n_seq, -5, 0, 0, 0), (0, 1, -1, 0, 0), (0, 1, len(seqs[1]) + 1, 0, 0),
               (0, n_seq - 2, 11, 0, 0)]
        rows, want = [], []
        for t in range(60):
            if int(rng.integers(0, 2)) == 0:
                rows.append(bad[t % len(bad)]); want.append((-1, L.E_ARG, 0, 0, 0))
            else:
                rows.append(good[t]); want.append(want_good[t % 40])
        head, runs = eng.realign_trace(ss, eng.make_pairs(rows), band, 250)
        assert unpack(head, runs) == want
        d, st = eng.realign(ss, eng.make_pairs(rows), band)
        assert d.tolist() == head[:, 0].tolist() and st.tolist() == head[:, 1].tolist()
        # cap_runs of 1, of exactly n_runs and of one below it
        need = [len(e[3]) for e in expect]
        for t in range(40):
            if need[t] < 2:
                continue
            pairs = eng.make_pairs([good[t]])
            assert unpack(*eng.realign_trace(ss, pairs, band, need[t])) == [want_good[t]]
            for cap in (need[t] - 1, 1):
                assert unpack(*eng.realign_trace(ss, pairs, band, cap)) == [(expect[t][0], L.E_OVERFLOW, expect[t][1], expect[t][2], need[t])]
        one = eng.seqset(["ACGTACGT", "ACGTACGT", "ACGTAGGT"])
        try:
            got = unpack(*eng.realign_trace(one, eng.make_pairs([(0, 1, 0, 0, 0), (0, 2, 0, 0, 0)]), 4, 1))
            assert got == [(0, 0, 8, 8, [(8, "=")]), (1, L.E_OVERFLOW, 8, 8, 3)]
        finally:
            one.close()
        # the call-level refusals
        pairs = eng.make_pairs(good[:3])
        for b in (0, -1, L.MAX_BAND + 1):
            with pytest.raises(L.VaporHipError) as e:
                eng.realign_trace(ss, pairs, b, 100)
            assert e.value.code == L.E_ARG and "band outside 1 .. VAPOR_MAX_BAND" in str(e.value)
        for cap in (0, -1):
            with pytest.raises(L.VaporHipError) as e:
                eng.realign_trace(ss, pairs, band, cap)
            assert e.value.code == L.E_ARG and "cap_runs below 1" in str(e.value)
        head, runs = np.zeros(24, dtype=np.int32), np.zeros(300, dtype=np.uint32)
        fn = L.load().vapor_realign_trace
        assert fn(eng._ctx, ss._h, -1, pairs.ctypes.data, 33, 100, L.ptr(head, ctypes.c_int32), L.ptr(runs, ctypes.c_uint32)) == L.E_ARG
        assert fn(eng._ctx, ss._h, 0, None, 33, 100, None, None) == 0
        assert fn(eng._ctx, None, 1, pairs.ctypes.data, 33, 100, L.ptr(head, ctypes.c_int32), L.ptr(runs, ctypes.c_uint32)) == L.E_ARG
        assert unpack(*eng.realign_trace(ss, pairs, band, 250)) == want_good[:3]          # (the context is as good as before)
    finally:
        ss.close()


def check_budget_at_its_floor_and_several_groups(make_engine):
    """300 small pairs run in one group at the floor; forty pairs of 4 000 rows at band 512 (2 MB of workspace each) among them
    make several.  Both answers equal the default budget's, and the small pairs' the model's."""
    rng = np.random.default_rng(21)
    cases = RM.fuzz_cases(seed=9, count=30, max_len=100)
    long_a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 4200)
    longs = []
    for k in range(4):
        r = np.concatenate([long_a[:1000 + 100 * k], long_a[1000 + 100 * k + 40:4040]]).copy()
        r[::97] = ord("A")
        longs.append(r.tobytes().decode())
    seqs = [s.decode() for c in cases for s in (c[1], c[2])] + longs + [long_a.tobytes().decode()]
    small = [(2 * (t % 30), 2 * (t % 30) + 1, cases[t % 30][3], 0, 0) for t in range(300)]
    big = [(60 + (t % 4), 64, 0, 0, 0) for t in range(40)]
    mixed = small[:150] + big[:20] + [(-1, 0, 0, 0, 0)] + small[150:] + big[20:]
    band = 512
    want_small = [M.trace(c[1], c[2], c[3], band) for c in cases]
    results = {}
    for budget in (None, 1):
        e = make_engine()
        try:
            if budget is not None:
                e.set_param("trace_budget", budget)          # (below the floor: raised to it)
            ss = e.seqset(seqs)
            try:
                results[budget] = [unpack(*e.realign_trace(ss, e.make_pairs(rows), band, 600)) for rows in (small, mixed)]
                d, st = e.realign(ss, e.make_pairs(mixed), band)
            finally:
                ss.close()
        finally:
            e.close()
        assert [(g[0], g[1]) for g in results[budget][1]] == list(zip(d.tolist(), st.tolist()))
    assert results[None] == results[1]
    assert results[1][0] == [(w[0], 0, w[1], w[2], w[3]) for w in (want_small[t % 30] for t in range(300))]
    got_big = [g for g, row in zip(results[1][1], mixed) if row[0] >= 60]
    for g, row in zip(got_big, big):
        assert g[1] == 0 and g[2] == 4000 and sum(k for k, op in g[4] if op == "D") >= 40, g[:4]
        assert sum(k for k, op in g[4] if op in "=XI") == 4000 and sum(k for k, op in g[4] if op in "=XD") == g[3]
        assert g == got_big[row[0] - 60]                     # (the same pair gives the same trace wherever it stands)


def test_the_budget_at_its_floor_and_several_groups():
    check_budget_at_its_floor_and_several_groups(lambda: Engine(0))


def test_one_long_pair(eng):
    """n = m = 65 535, B = 512, a planted deletion of 300 bases and a substitution every 1 000, against realign.trace_statement
    (held to the plain model on the small cases by tests/test_trace_cpu.py)."""
    rng = np.random.default_rng(99)
    allele = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 65535 + 300)
    read = np.concatenate([allele[:30000], allele[30300:]]).copy()
    for p in range(500, 65535, 1000):
        read[p] = ord("A") if read[p] != ord("A") else ord("C")
    allele = allele[:65535]
    r, a = read.tobytes().decode(), allele.tobytes().decode()
    ss = eng.seqset([r, a])
    try:
        got = unpack(*eng.realign_trace(ss, eng.make_pairs([(0, 1, 0, 0, 0)]), 512, 1000))[0]
        d, _st = eng.realign(ss, eng.make_pairs([(0, 1, 0, 0, 0)]), 512)
    finally:
        ss.close()
    e = realign.trace_statement(r, a, 0, 512)
    print("one long pair: d = %d, %d runs, end (%d, %d)" % (got[0], len(got[4]), got[2], got[3]))
    assert got == (e[0], 0, e[1], e[2], e[3]) and int(d[0]) == e[0]
    assert sum(k for k, op in got[4] if op == "D") >= 300 and 300 <= e[0] <= 366


# ------------------------------------------------------------------------------------------------------------------------------
# through the CLI
# ------------------------------------------------------------------------------------------------------------------------------
_traced = {}


def _statement_engine(monkeypatch):
    """Engine.realign and Engine.realign_trace replaced by the statements over the texts of the set."""
    TG._statement_engine(monkeypatch)

    def traced(self, ss, pairs, band, cap_runs):
        head = np.zeros((len(pairs), 8), dtype=np.int32)
        runs = np.zeros((len(pairs), cap_runs), dtype=np.uint32)
        for t, p in enumerate(pairs):
            key = (ss.texts[p["seq1"]], ss.texts[p["seq2"]], int(p["off2"]), band)
            if key not in _traced:
                _traced[key] = realign.trace_statement(*key)
            d, i_end, j_end, rr = _traced[key]
            head[t, :5] = (d, 0 if len(rr) <= cap_runs else L.E_OVERFLOW, i_end, j_end, len(rr))
            if rr and len(rr) <= cap_runs:
                runs[t, cap_runs - len(rr):] = [k << 2 | realign.OPS.index(op) for k, op in rr]
        return head, runs
    monkeypatch.setattr(Engine, "realign_trace", traced)


@pytest.mark.parametrize("cmd", ["bed", "vcf"])
def test_cli_on_a_world_in_memory(cmd, tmp_path, monkeypatch):
    """`vapor bed | vcf --realign --realign-out` on the seven loci of tests/test_gpu_realign.py: the table is the `--realign`
    run's, and table, SAM and FASTA are those of the same run with the engine's two entries replaced by the Python statements."""
    w = synth.make_support_world(seed=4, specs=TG.SPECS, layers=4, read_len=4000)
    text = synth.bed_text(w) if cmd == "bed" else synth.vcf_text(w)
    pipeline.set_engine(None)
    calls = []
    orig = Engine.realign_trace
    monkeypatch.setattr(Engine, "realign_trace", lambda self, ss, pairs, band, cap: calls.append((len(pairs), cap)) or orig(self, ss, pairs, band, cap))
    try:
        seqio.set_backend(seqio.MemorySamtools(w))
        plain, annotated_plain = TS.run_main(tmp_path, "plain", cmd, text, ["--realign"])
        assert not calls
        seqio.set_backend(seqio.MemorySamtools(w))
        table, annotated = TS.run_main(tmp_path, "dev", cmd, text, ["--realign", "--realign-out", str(tmp_path / "dev_pre")])
        assert calls and calls[0][1] == realign.FIRST_CAP_RUNS
        _statement_engine(monkeypatch)
        seqio.set_backend(seqio.MemorySamtools(w))
        stated, _ = TS.run_main(tmp_path, "stated", cmd, text, ["--realign", "--realign-out", str(tmp_path / "stated_pre")])
    finally:
        seqio.set_backend(None)
        pipeline.set_engine(None)
    assert table == plain == stated and annotated == annotated_plain
    sam, fa = (tmp_path / "dev_pre.sam").read_text(), (tmp_path / "dev_pre.fa").read_text()
    assert sam == (tmp_path / "stated_pre.sam").read_text() and fa == (tmp_path / "stated_pre.fa").read_text()
    n_loci = sum(1 for t, _s, _z in TG.SPECS if not (cmd == "vcf" and t == "TANDUP"))
    assert fa.count(">") == 2 * n_loci and sam.count("@SQ\t") == 2 * n_loci
    records = [ln.split("\t") for ln in sam.splitlines() if not ln.startswith("@")]
    n_reads = sum(len(r.split("\t")[-1].split(",")) for r in table.splitlines()[1:])
    # (one pair a read over a round's first calls; a read without an '=' or 'X' is not written)
    assert 0 < len(records) <= n_reads == sum(n for n, cap in calls if cap == realign.FIRST_CAP_RUNS)
    # the hom DEL locus (the first): every ALT-voting read lies on |ALT and carries no D or I run of 50 or more
    first = fa.splitlines()[0][1:-4]
    mine = [f for f in records if f[0].rsplit("/", 1)[0] == first]
    alt = [f for f in mine if f[14] == "vt:Z:ALT"]
    assert len(alt) > 3 and len(alt) == int(table.splitlines()[1].split("\t")[-7])
    for f in alt:
        assert f[2] == first + "|ALT" and not [k for k, op in re.findall(r"(\d+)([ID])", f[5]) if int(k) >= 50], f[:6]
