"""The wide route (vapor_wide_batch / vapor_clean_hits_wide): sequences longer than VAPOR_MAX_SEQ_LEN, checked exactly
against the C oracle (int32 positions, no length limit) and, for pairs both routes accept, against the narrow route."""
import numpy as np
import pytest

import dot_designs

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CAP = 1048575


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes().decode()


def _mutate(rng, s, rate=0.02):
    """A read of allele s: substitutions and a few short indels."""
    a = np.frombuffer(s.encode(), dtype=np.uint8).copy()
    pos = rng.random(len(a)) < rate
    a[pos] = ACGT[rng.integers(0, 4, int(pos.sum()))]
    out = a.tobytes().decode()
    for _ in range(4):
        p = int(rng.integers(0, len(out) - 50))
        out = out[:p] + out[p + int(rng.integers(1, 20)):] if rng.random() < 0.5 else out[:p] + _rand(rng, 7) + out[p:]
    return out


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgtNn", "TGCAtgcaNn"))


def _cases(rng):
    """(name, read, allele, off2): the kinds of pair the issue lists, at lengths across the narrow limit."""
    out = []
    for n in (65535, 65536, 70000, 131071):
        al = _rand(rng, n)
        out.append(("mut%d" % n, _mutate(rng, al), al, 0))
    al = _rand(rng, 70000)
    rd = _mutate(rng, al)
    inv = rd[:30000] + _revcomp(rd[30000:40000]) + rd[40000:]
    out.append(("inversion", inv, al, 0))
    nread = rd[:20000] + "N" * 12 + rd[20012:50000] + "n" + rd[50001:]
    out.append(("n_in_read", nread, al, 0))
    soft = al[:10000] + al[10000:30000].lower() + al[30000:]
    out.append(("softmask", _mutate(rng, al), soft, 0))
    big = _rand(rng, 140000)
    out.append(("off2", _mutate(rng, big[70000:]), big, 70000))
    return out


def _check_stats(st, exp, name):
    assert st[15] == 0, (name, st.tolist())
    assert st[:10].tolist() == exp[:10].tolist(), (name, st[:10].tolist(), exp[:10].tolist())


def test_stats_against_oracle(eng, oracle):
    rng = np.random.default_rng(11)
    cases = _cases(rng)
    seqs, rows = [], []
    for name, rd, al, off2 in cases:
        b = len(seqs)
        seqs += [rd, al]
        for k in (10, 20, 30, 40):
            for fl in (1, 2, 5, 3):
                rows.append((b, b + 1, off2, k, fl))
    ss = eng.seqset(seqs)
    st = eng.score_wide(ss, eng.make_pairs(rows))
    ss.close()
    exp_of, r4_of, n_dir = {}, {}, 0
    for t, (s1, s2, off2, k, fl) in enumerate(rows):
        key = (s1, s2, off2, k)
        if key not in exp_of:
            exp_of[key] = oracle.pair_stats(k, seqs[s1], seqs[s2][off2:], want_hits=True)
        exp = exp_of[key][0].copy()
        if not fl & 1:
            exp[3] = exp[4] = 0
        if not fl & 2:
            exp[5] = exp[6] = exp[9] = 0
        _check_stats(st[t], exp, (t, rows[t]))
        if fl == 5:                                 # the directed statistics, once per pair and window size
            if key not in r4_of:
                _st, h, k1, _k2 = exp_of[key]
                r4_of[key] = dot_designs.r4_words(h[k1 > 0].tolist()) if exp[3] > 0 else [0, 0, 0, 0]
            assert st[t, 10:14].tolist() == r4_of[key], (t, rows[t], st[t, 10:14].tolist(), r4_of[key])
            n_dir += 1
    assert int(st[:, 0].min()) > 0 and n_dir == len(rows) // 4


def test_large_pairs_cap_and_refusal(eng, oracle):
    rng = np.random.default_rng(12)
    al = _rand(rng, 300000)
    rd = _mutate(rng, al, 0.01)
    at_cap = _rand(rng, CAP)
    over = at_cap + "A"
    seqs = [rd, al, at_cap[:200000], at_cap, over]
    rows = [(0, 1, 0, 20, 3), (2, 3, 0, 30, 3), (4, 1, 0, 20, 3), (0, 4, 0, 20, 3), (0, 1, 0, 10, 1)]
    ss = eng.seqset(seqs)
    st = eng.score_wide(ss, eng.make_pairs(rows))
    ss.close()
    _check_stats(st[0], oracle.pair_stats(20, rd, al), "300k")
    _check_stats(st[1], oracle.pair_stats(30, seqs[2], at_cap), "cap")
    assert st[2, 15] == -4 and st[3, 15] == -4          # one base over the cap: VAPOR_E_ARG
    exp = oracle.pair_stats(10, rd, al)
    exp[5] = exp[6] = exp[9] = 0
    _check_stats(st[4], exp, "after refusals")


def test_hits_equal_dotdata(eng, oracle):
    rng = np.random.default_rng(13)
    al = _rand(rng, 70000)
    rd = _mutate(rng, al)
    soft = al[:5000] + al[5000:9000].lower() + al[9000:]
    ss = eng.seqset([rd, al, soft])
    st, hits = eng.score_wide(ss, eng.make_pairs([(0, 1, 0, 10, 3), (0, 2, 100, 20, 0), (2, 2, 0, 10, 0)]), want_hits=True)
    ss.close()
    for t, (a, b) in enumerate(((rd, al), (rd, soft[100:]), (soft, soft))):
        k = (10, 20, 10)[t]
        exp = oracle.dotdata_array(k, a, b)
        assert st[t, 0] == len(exp)
        assert np.array_equal(hits[t], exp), t


def test_clean_hits_wide_against_oracle(eng, oracle):
    rng = np.random.default_rng(14)
    al = _rand(rng, 90000)
    rd = _mutate(rng, al, 0.05)
    h1 = oracle.dotdata_array(10, rd, al)
    h2 = np.concatenate([h1, rng.integers(0, CAP + 1, size=(5000, 2)).astype(np.int32)])
    st, fl = eng.clean_hits_wide([h1, h2, np.zeros((0, 2), np.int32)], flags=[3, 3, 3])
    for t, h in enumerate((h1, h2)):
        k1 = oracle.clean_c1_flags(h)
        k2 = oracle.clean_c2_flags(h)
        assert np.array_equal((fl[t] & 1) != 0, k1 > 0), t
        assert np.array_equal((fl[t] & 2) != 0, k2 == 1), t
        assert np.array_equal((fl[t] & 4) != 0, k2 == 2), t
        assert st[t, 0] == len(h) and st[t, 3] == int((k1 > 0).sum()) and st[t, 5] == int((k2 > 0).sum())
    assert st[2, 0] == 0 and st[2, 1] == -1 and st[2, 15] == 0
    from vapor_amd import _lib as L
    with pytest.raises(L.VaporHipError) as e:
        eng.clean_hits_wide([np.asarray([[CAP + 1, 0]], np.int32)])
    assert e.value.code == L.E_ARG


def test_narrow_pairs_through_the_wide_route(eng):
    """Pairs the narrow route accepts give its statistics exactly, all sixteen words (DIR included)."""
    from vapor_amd import synth
    alleles, reads, pr = synth.make_pairs(seed=5, n_alleles=6, reads_per_allele=6, read_len=8000, allele_len=12000)
    seqs = alleles + reads
    rng = np.random.default_rng(15)
    rows = []
    for r, a in pr:
        k = int(rng.choice([10, 20, 30, 40]))
        fl = int(rng.choice([1, 2, 3, 5, 7]))
        rows.append((len(alleles) + r, a, int(rng.integers(0, 200)), k, fl))
    rows.append((len(alleles), len(alleles), 0, 10, 7))          # a self plot
    ss = eng.seqset(seqs)
    pairs = eng.make_pairs(rows)
    narrow = eng.score(ss, pairs)
    wide = eng.score_wide(ss, pairs)
    _st, hits = eng.dotplots(ss, pairs)
    _st2, whits = eng.score_wide(ss, pairs, want_hits=True)
    ss.close()
    assert np.array_equal(narrow, wide), np.argwhere(narrow != wide)[:5].tolist()
    for a, b in zip(hits, whits):
        assert np.array_equal(a, b)


def test_mixed_batch_overflow_then_rerun(eng, oracle):
    import ctypes
    from vapor_amd import _lib as L
    rng = np.random.default_rng(16)
    al = _rand(rng, 80000)
    rd = _mutate(rng, al)
    sa = _rand(rng, 3000)
    sr = _mutate(rng, sa)
    ss = eng.seqset([rd, al, sr, sa])
    pairs = eng.make_pairs([(2, 3, 0, 10, 7), (0, 1, 0, 10, 3), (2, 3, 5, 20, 3)])
    st = np.zeros((3, 16), np.int64)
    off = np.zeros(4, np.int64)
    hits = np.zeros((16, 2), np.int32)
    lib = L.load()
    rc = lib.vapor_wide_batch(eng._ctx, ss._h, 3, pairs.ctypes.data, L.ptr(st, ctypes.c_int64), L.ptr(hits, ctypes.c_int32), 16,
                              L.ptr(off, ctypes.c_int64))
    assert rc == L.E_OVERFLOW and off[3] > 16
    exp = [oracle.pair_stats(10, sr, sa), oracle.pair_stats(10, rd, al), oracle.pair_stats(20, sr, sa[5:])]
    for t in range(3):
        _check_stats(st[t], exp[t], t)
    hits = np.zeros((int(off[3]), 2), np.int32)
    st2 = np.zeros((3, 16), np.int64)
    rc = lib.vapor_wide_batch(eng._ctx, ss._h, 3, pairs.ctypes.data, L.ptr(st2, ctypes.c_int64), L.ptr(hits, ctypes.c_int32),
                              int(off[3]), L.ptr(off, ctypes.c_int64))
    ss.close()
    assert rc == 0 and np.array_equal(st, st2)
    for t, (a, b) in enumerate(((sr, sa), (rd, al), (sr, sa[5:]))):
        h = hits[off[t]:off[t + 1]]
        assert np.array_equal(h[np.lexsort((h[:, 1], h[:, 0]))], oracle.dotdata_array((10, 10, 20)[t], a, b)), t


def test_reference_named_functions_on_a_70kb_pair(oracle):
    from vapor_amd import simple_function as SF
    rng = np.random.default_rng(17)
    ref = _rand(rng, 70000)
    alt = ref[:30000] + _rand(rng, 3000) + ref[30000:]
    rd = _mutate(rng, alt, 0.01)[:69000]
    assert SF.dotdata(20, rd, ref[:66000]) == oracle.dotdata(20, rd, ref[:66000])
    dots = SF.dotdata(10, rd, alt)
    assert SF.clean_dotdata_diagnal_and_anti_diagnal(dots) == oracle.clean_dotdata_diagnal_and_anti_diagnal(dots)
    x = [rd, 0]
    for k in (10, 20):
        assert SF.calcu_vapor_single_read_score_abs_dis_m1b(ref, alt, x, k) == oracle.score_abs_dis_m1b(ref, alt, x, k)
        assert SF.calcu_vapor_single_read_score_within_10Perc_m1b(ref, alt, x, k) == oracle.score_within_10Perc_m1b(ref, alt, x, k)
        assert (SF.calcu_vapor_single_read_score_directed_dis_m1b_redefine_diagnal(ref, alt, x, k)
                == oracle.score_directed_dis_m1b_redefine_diagnal(ref, alt, x, k))
    # window_size_refine (SF:2030-2046) on the 70 kb allele: its self plot's counts decide at the first size
    n, nd, nl = oracle.qual_check_counts(oracle.dotdata_array(10, alt, alt))
    assert len(alt) > 65535 and not 0.1 < float(nl) / float(n) < 0.5 and float(nd) / float(n) > 0.4
    assert SF.window_size_refine(alt) == [10, [float(nd) / float(n), [0]]]


def test_score_requests_long_loci(oracle):
    """A long locus among short ones: scored on the wide route, in place; the short ones as before."""
    from vapor_amd import pipeline
    rng = np.random.default_rng(18)
    ref = _rand(rng, 9000)
    alt = ref[:4000] + _rand(rng, 70000) + ref[4000:]
    reads = [(_mutate(rng, alt, 0.01)[int(m):], int(m)) for m in (0, 3, 7)]
    sref = _rand(rng, 4000)
    salt = sref[:2000] + sref[2500:]
    sreads = [(_mutate(rng, salt, 0.01), 0)]
    reqs = [pipeline.Score(kind="s1", ref_seq=sref, alt_seq=salt, reads=sreads, k=10),
            pipeline.Score(kind="s1", ref_seq=ref, alt_seq=alt, reads=reads, k=10),
            pipeline.Score(kind="s2", ref_seq=ref, alt_seq=alt, reads=reads, k=20),
            pipeline.Score(kind="s3", ref_seq=ref, alt_seq=alt, reads=reads, k=10)]
    eng = pipeline.get_engine()
    got = pipeline.score_requests(eng, reqs)
    alone = pipeline.score_requests(eng, reqs[:1])
    assert got[0] == alone[0]
    fn = {"s1": oracle.score_abs_dis_m1b, "s2": oracle.score_within_10Perc_m1b, "s3": oracle.score_directed_dis_m1b_redefine_diagnal}
    for r, g in zip(reqs[1:], got[1:]):
        assert not isinstance(g, BaseException), g
        exp = []
        for x in r.reads:
            a, b = fn[r.kind](r.ref_seq, r.alt_seq, [x[0], x[1]], r.k)
            exp.append(None if (a == 0 or b == 0) else 1.0 - float(b) / float(a))
        assert g == exp, (r.kind, g, exp)


@pytest.mark.parametrize("name,n_loci", [("cfg2", None), ("cfg3", 60)])
def test_workload_pairs_through_the_wide_route(eng, name, n_loci):
    """Every pair of bench.py's cfg2 batch and of a prefix of cfg3's (DEL / TANDUP with DIR / INV / INS, derived alleles, the
    seeds bench.py uses): the wide route gives the plan route's sixteen statistics words exactly."""
    from vapor_amd import workload as wl
    spec = dict(wl.WORKLOADS[name])
    if n_loci is not None:
        spec["n_loci"] = n_loci
    w = wl.make_workload(name, seed={"cfg2": 1000, "cfg3": 3000}[name], **spec)
    ss = w.upload(eng)
    try:
        narrow = eng.score(ss, w.pairs)
        wide = eng.score_wide(ss, w.pairs)
    finally:
        ss.close()
    assert len(w.pairs) >= 4000 and int((w.pairs["flags"] & 4).sum()) > 0
    assert np.array_equal(narrow, wide), np.argwhere(narrow != wide)[:5].tolist()


def test_count_pass_stops_at_max_pair_cap(oracle):
    """A low-complexity pair with far more dots than "max_pair_cap": refused with VAPOR_E_OVERFLOW after about cap dots of work,
    the other pairs of the call unaffected."""
    from vapor_amd import _lib as L
    from vapor_amd.engine import Engine
    e = Engine(0)
    try:
        e.set_param("max_pair_cap", 100000)
        rng = np.random.default_rng(19)
        al = _rand(rng, 20000)
        rd = _mutate(rng, al)
        poly = "A" * 300000
        ss = e.seqset([poly, rd, al])
        st = e.score_wide(ss, e.make_pairs([(0, 0, 0, 10, 3), (1, 2, 0, 10, 3)]))
        ss.close()
    finally:
        e.close()
    assert st[0, 15] == L.E_OVERFLOW and st[0, 14] > 100000 and st[0, 14] < 300000 ** 2
    _check_stats(st[1], oracle.pair_stats(10, rd, al), "beside the refused pair")
