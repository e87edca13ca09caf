"""The any-k route (vapor_anyk_batch): kmerhits at every k from 1 to 64 on the device, against the reference's goldens, the C
oracle (k <= 40, inversions), the test-local restatement of both match rules (anyk_model) and the plan and wide routes."""
import numpy as np
import pytest

import anyk_model as model
from conftest import load_golden

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
GOLD = load_golden("kmerhits_anyk.json.gz")


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    from vapor_amd import pipeline
    e = Engine(0)
    pipeline.set_engine(e)
    yield e
    pipeline.set_engine(None)
    e.close()


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes().decode()


def _mutate(rng, s, sub=0.04, ins=0.03, dele=0.03):
    out = []
    for c in s:
        r = rng.random()
        if r < dele:
            continue
        out.append("ACGT"[int(rng.integers(0, 4))] if r < dele + sub else c)
        if rng.random() < ins:
            out.append("ACGT"[int(rng.integers(0, 4))])
    return "".join(out)


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgtNn", "TGCAtgcaNn"))


def _anyk(eng, s1, s2, k, flags=3, off2=0):
    ss = eng.seqset([s1, s2])
    try:
        st, hits = eng.score_anyk(ss, eng.make_pairs([(0, 1, off2, k, flags)]), want_hits=True)
    finally:
        ss.close()
    return st[0], hits[0]


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_kmerhits_and_dotdata_golden(eng, case):
    from vapor_vali.Simple_function import dotdata, kmerhits
    k, inv = case["k"], case["inversions"]
    if "error" in case["out"]:
        with pytest.raises(KeyError):
            kmerhits(case["s1"], case["s2"], k, 1, inv)
        return
    got = kmerhits(case["s1"], case["s2"], k, 1, inv)
    assert model.matches(case["out"]["ok"], got), case["name"]
    if inv:
        assert dotdata(k, case["s1"], case["s2"]) == got


@pytest.mark.parametrize("case", GOLD["scorers"], ids=lambda c: c["name"])
def test_scorers_golden(eng, case):
    from vapor_vali import Simple_function as SF
    x = [case["read"], case["miss"], case["name"]]
    for key, fn in (("s1", SF.calcu_vapor_single_read_score_abs_dis_m1b),
                    ("s2", SF.calcu_vapor_single_read_score_within_10Perc_m1b),
                    ("s3", SF.calcu_vapor_single_read_score_directed_dis_m1b_redefine_diagnal)):
        got = fn(case["ref"], case["alt"], x, case["k"])
        assert [float(v) for v in got] == [float(v) for v in case[key]["ok"]], (case["name"], key)


def test_scorer_requests_any_k(eng):
    """pipeline.score_requests sends requests at another k to the any-k route (and gets a score per read, not a ValueError)."""
    from vapor_amd import pipeline
    from vapor_amd.drivers import Score
    reqs = [Score(kind, c["ref"], c["alt"], [(c["read"], c["miss"])], c["k"]) for c in GOLD["scorers"] for kind in ("s1", "s2", "s3")]
    out = pipeline.score_requests(eng, reqs)
    again = pipeline.score_requests_wide(eng, reqs, anyk=True)
    assert out == again
    assert all(isinstance(v, list) and len(v) == 1 for v in out)


@pytest.mark.parametrize("shape", [(2000, 4000), (10000, 20000)])
def test_exact_vs_oracle(eng, oracle, shape):
    """k <= 40 with inversions: the dots equal oracle.dotdata_array (order included), the statistics oracle.pair_stats."""
    rng = np.random.default_rng(shape[0])
    n1, n2 = shape
    al = _rand(rng, n2)
    rd = _mutate(rng, al[n2 // 4: n2 // 4 + n1], 0.02, 0.01, 0.01)
    rd = rd[: n1 // 2] + _revcomp(rd[n1 // 2: 3 * n1 // 4]) + rd[3 * n1 // 4:]
    ks = (3, 11, 15, 17, 25, 33, 39) if n1 <= 2000 else (15, 25)
    ss = eng.seqset([rd, al])
    try:
        rows = [(0, 1, 0, k, 3) for k in ks]
        st, hits = eng.score_anyk(ss, eng.make_pairs(rows), want_hits=True)
    finally:
        ss.close()
    for t, k in enumerate(ks):
        exp = oracle.dotdata_array(k, rd, al)
        assert np.array_equal(hits[t], exp), k
        ref = oracle.pair_stats(k, rd, al)
        assert st[t, :10].tolist() == ref[:10].tolist(), (k, st[t].tolist(), ref.tolist())
        assert st[t, 15] == 0


def test_forward_vs_model(eng):
    """VAPOR_PF_FORWARD (inversions=False), symbols outside the alphabet compared byte for byte: the restatement."""
    rng = np.random.default_rng(11)
    base = _rand(rng, 1500)
    s1 = base[:300] + "XXUX" + base[300:700].lower() + "NNNN" + base[700:] + "RYX"
    s2 = base[200:900] + "XUXX" + _mutate(rng, base[900:], 0.02, 0.01, 0.01) + "RYU"
    for k in (2, 4, 13, 21, 40, 45, 60):
        _st, got = _anyk(eng, s1, s2, k, flags=8 | 3)
        exp = model.kmerhits(s1, s2, k, False)
        assert [tuple(h) for h in got.tolist()] == exp, k


@pytest.mark.parametrize("k", [10, 20, 30, 40])
def test_plan_and_wide_routes_agree(eng, k):
    """k in {10, 20, 30, 40}: vapor_anyk_batch == vapor_wide_batch == the plan route, word for word (flags 1/2/3/7)."""
    rng = np.random.default_rng(k)
    al = _rand(rng, 6000)
    reads = [_mutate(rng, al[500:4500], 0.02, 0.01, 0.01), _revcomp(_mutate(rng, al[1000:3000], 0.01, 0.01, 0.01)),
             al[2000:2600] * 4]
    seqs = reads + [al]
    ss = eng.seqset(seqs)
    try:
        rows = [(r, 3, off, k, fl) for r in range(3) for off in (0, 7) for fl in (1, 2, 3, 7)]
        pr = eng.make_pairs(rows)
        a_st, a_hits = eng.score_anyk(ss, pr, want_hits=True)
        w_st, w_hits = eng.score_wide(ss, pr, want_hits=True)
        p_st = eng.score(ss, pr)
    finally:
        ss.close()
    assert np.array_equal(a_st, w_st)
    assert np.array_equal(a_st, p_st)
    for a, w in zip(a_hits, w_hits):
        assert np.array_equal(a, w)


def _edit_pairs(rng):
    al = _rand(rng, 3000)
    rd = _mutate(rng, al[400:2000], 0.03, 0.02, 0.02)
    rd = rd[:800] + _revcomp(rd[800:1200]) + rd[1200:]
    return rd, al


@pytest.mark.parametrize("k", [41, 50, 64])
def test_edit_distance_vs_model(eng, k):
    """k > 40: the restatement at 1.6 kb x 3 kb (key rank order, list order, reverse strand)."""
    rng = np.random.default_rng(k)
    rd, al = _edit_pairs(rng)
    st, got = _anyk(eng, rd, al, k)
    exp = model.kmerhits(rd, al, k, True)
    assert st[0] == len(exp) and st[15] == 0
    assert [tuple(h) for h in got.tolist()] == exp


def test_edit_distance_adversarial_indels(eng):
    """Queries at exactly k // 10 edits, the edits on piece boundaries and at the ends, and at k // 10 + 1."""
    rng = np.random.default_rng(5)
    for k in (41, 50, 57, 64):
        t = k // 10
        key = _rand(rng, k)
        s2 = []
        for shift in range(t + 1):
            q = list(key)
            step = max(1, k // (t + 1))
            for e in range(shift):
                p = min(k - 1, (e + 1) * step)
                if e % 3 == 0:
                    del q[p]
                    q.append("A")
                elif e % 3 == 1:
                    q.insert(p, "C")
                    q.pop(0)
                else:
                    q[p] = "T" if q[p] != "T" else "G"
            s2.append("".join(q))
        over = list(key)
        for e in range(t + 1):
            over[e * (k // (t + 1))] = "T" if over[e * (k // (t + 1))] != "T" else "G"
        s2.append("".join(over))
        s2.append(key[1:] + "G")
        s2.append("C" + key[:-1])
        seq2 = "".join(s + _rand(rng, 5) for s in s2)
        seq1 = _rand(rng, 11) + key + _rand(rng, 9)
        _st, got = _anyk(eng, seq1, seq2, k)
        assert [tuple(h) for h in got.tolist()] == model.kmerhits(seq1, seq2, k, True), k


def test_overflow_at_cap(eng):
    """A pair with more dots than max_pair_cap is VAPOR_E_OVERFLOW; the other pairs of the batch are unaffected."""
    from vapor_amd import _lib as L
    rng = np.random.default_rng(3)
    al = _rand(rng, 3000)
    rd = _mutate(rng, al[:2000], 0.02, 0.01, 0.01)
    homo = "A" * 400
    ss = eng.seqset([rd, al, homo])
    rows = [(0, 1, 0, 15, 3), (2, 2, 0, 7, 3), (0, 1, 0, 45, 3), (2, 2, 0, 45, 3), (0, 1, 0, 65, 3), (0, 1, 0, 0, 3)]
    try:
        st0, h0 = eng.score_anyk(ss, eng.make_pairs(rows), want_hits=True)
        eng.set_param("max_pair_cap", 50000)
        try:
            st1, h1 = eng.score_anyk(ss, eng.make_pairs(rows), want_hits=True)
        finally:
            eng.set_param("max_pair_cap", 1 << 28)
    finally:
        ss.close()
    assert st0[1, 0] == 394 * 394 and st0[3, 0] == 356 * 356
    for t in (1, 3):
        assert st1[t, 15] == L.E_OVERFLOW and st1[t, 14] > 50000 and len(h1[t]) == 0
    for t in (0, 2):
        assert st1[t].tolist() == st0[t].tolist() and np.array_equal(h1[t], h0[t])
    assert st0[4, 15] == L.E_ARG and st0[5, 15] == L.E_ARG


def test_limits_raise(eng):
    from vapor_vali.Simple_function import kmerhits
    with pytest.raises(ValueError, match="VAPOR_MAX_ANY_K"):
        kmerhits("ACGT" * 30, "ACGT" * 30, 65)
    with pytest.raises(ValueError, match="nth_base"):
        kmerhits("ACGT" * 30, "ACGT" * 30, 15, 2)
