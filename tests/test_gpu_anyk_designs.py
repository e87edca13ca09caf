"""The designed pairs of tests/anyk_designs.py on the any-k route (vapor_anyk_batch).  Every comparison is exact: the dots
equal anyk_model's, order included; words 0-13 of the record equal dot_designs.expected() under the pair's flags (10-13 where
they ask for R4, zeros elsewhere) and word 15 the expected status.  Each group runs in one score_anyk call, edit_split in one
per launch size; the k = 10, 20, 30, 40 designs with inversions also go through score_wide and score."""
import ctypes

import numpy as np
import pytest

import anyk_designs as ad

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    from vapor_amd import _lib as L
    assert (L.PF_FORWARD, L.E_KEYERROR) == (ad.PF_FORWARD, ad.E_KEYERROR)
    e = Engine(0)
    yield e
    e.close()


def _table(pairs):
    seqs, at = [], {}
    for p in pairs:
        for s in (p.s1, p.s2):
            if s not in at:
                at[s] = len(seqs)
                seqs.append(s)
    return seqs, [(at[p.s1], at[p.s2], p.off2, p.k, p.pair_flags) for p in pairs]


def _score(eng, pairs, edit_pairs=None, also=()):
    """(statistics, dots) of the pairs in one score_anyk call; also: "wide" / "plan" for the same rows on those routes."""
    seqs, rows = _table(pairs)
    ss = eng.seqset(seqs)
    try:
        pr = eng.make_pairs(rows)
        if edit_pairs is not None:
            eng.set_param("anyk_edit_pairs", edit_pairs)
        try:
            out = [eng.score_anyk(ss, pr, want_hits=True)]
        finally:
            eng.set_param("anyk_edit_pairs", ad.EDIT_PAIRS_DEFAULT)
        if "wide" in also:
            out.append(eng.score_wide(ss, pr, want_hits=True))
        if "plan" in also:
            out.append(eng.score(ss, pr))
    finally:
        ss.close()
    return out[0] if not also else out


def _diff(pairs, st, hits):
    errs = []
    for t, p in enumerate(pairs):
        want, code = p.expected()
        exp = p.hits()
        if not np.array_equal(hits[t], exp):
            bad = next((q for q in range(min(len(exp), len(hits[t]))) if tuple(hits[t][q]) != tuple(exp[q])), min(len(exp), len(hits[t])))
            errs.append("%s/%s: %d dots for %d, first difference at %d" % (p.group, p.name, len(hits[t]), len(exp), bad))
        if st[t, :14].tolist() != want:
            errs.append("%s/%s: words 0-13 %s for %s" % (p.group, p.name, st[t, :14].tolist(), want))
        if st[t, 15] != code:
            errs.append("%s/%s: status %d for %d" % (p.group, p.name, st[t, 15], code))
    return errs


def _check(pairs, st, hits):
    errs = _diff(pairs, st, hits)
    assert not errs, "%d differences:\n%s" % (len(errs), "\n".join(errs[:20]))


def _routes_agree(eng, pairs):
    picks = [p for p in pairs if p.k in (10, 20, 30, 40) and not p.forward]
    if not picks:
        return 0
    (a_st, a_hits), (w_st, w_hits), p_st = _score(eng, picks, also=("wide", "plan"))
    assert np.array_equal(a_st, w_st) and np.array_equal(a_st, p_st), [p.name for p in picks]
    for p, a, w in zip(picks, a_hits, w_hits):
        assert np.array_equal(a, w), p.name
    return len(picks)


def test_sort_sizes(eng):
    ps = ad.sort_sizes()
    assert {p.np for p in ps} == {512, 1024, 2048, 4096, 8192}
    _check(ps, *_score(eng, ps))


def test_every_k(eng):
    ps = ad.every_k()
    _check(ps, *_score(eng, ps))
    assert _routes_agree(eng, ps) == 4 + 3


def test_last_symbol(eng):
    ps = ad.last_symbol()
    st, hits = _score(eng, ps)
    _check(ps, st, hits)
    for p, h in zip(ps, hits):
        got = set(map(tuple, h.tolist()))
        assert all(((j, i) in got) == dot for j, i, dot in p.planted), p.name
    assert _routes_agree(eng, ps) == 1


def test_edit_rounds(eng):
    ps = ad.edit_rounds()
    assert {p.D for p in ps if "keys" in p.info} == set(ad.ROUND_D)
    _check(ps, *_score(eng, ps))


def test_golden_rounds(eng):
    """The eight pairs whose dots the reference states (tests/golden/kmerhits_anyk.json.gz holds them; the model equals it)."""
    ps = ad.golden_rounds()
    _check(ps, *_score(eng, ps))


@pytest.mark.parametrize("per", ad.SPLIT_PER)
def test_edit_split(eng, per):
    """Launches of 4, 8 and 64 allele k-mers: the dots on both sides of every cut, equal to the same pairs' at the default."""
    ps = [p for p in ad.edit_split() if p.edit_pairs == 252 * per]
    assert len(ps) == 2 and all(p.per == per and p.n_launches > 1 for p in ps)
    st, hits = _score(eng, ps, edit_pairs=252 * per)
    _check(ps, st, hits)
    st0, hits0 = _score(eng, ps)
    assert np.array_equal(st, st0) and all(np.array_equal(a, b) for a, b in zip(hits, hits0))


def test_edit_split_default(eng):
    """The shipped launch size: one launch for the small pairs, three for the read of 200 000 symbols."""
    from vapor_amd import _lib as L
    ps = ad.edit_split()
    assert ps[-1].edit_pairs is None and ps[-1].n_launches == 3 and all(ad.launches(p.n, p.nk2) == 1 for p in ps[:-1])
    _check(ps, *_score(eng, ps))
    for bad in (0, -1):
        with pytest.raises(L.VaporHipError):
            eng.set_param("anyk_edit_pairs", bad)
    eng.set_param("anyk_edit_pairs", ad.EDIT_PAIRS_DEFAULT)


def test_batch_state(eng):
    """A small edit pair after a large one, an exact pair after an edit pair, forward after inversions, a pair without k-mers,
    a refused pair, an edit pair again: each as the model has it and as the same pair has it alone; then the capacity protocol
    of the raw entry."""
    from vapor_amd import _lib as L
    ps = ad.batch_state()
    st, hits = _score(eng, ps)
    _check(ps, st, hits)
    for t, p in enumerate(ps):
        st1, hits1 = _score(eng, [p])
        assert st1[0].tolist() == st[t].tolist() and np.array_equal(hits1[0], hits[t]), p.name
    seqs, rows = _table(ps)
    n = len(ps)
    need = sum(len(h) for h in hits)
    fn = eng._wide_entry("vapor_anyk_batch")
    ss = eng.seqset(seqs)
    try:
        pr = np.ascontiguousarray(eng.make_pairs(rows), dtype=L.PAIR_DTYPE)
        res = []
        for cap in (need - 1, len(hits[0]), need):
            st2 = np.zeros((n, 16), dtype=np.int64)
            off = np.full(n + 1, -7, dtype=np.int64)
            out = np.full((max(cap, 1), 2), -1, dtype=np.int32)
            rc = fn(eng._ctx, ss._h, n, pr.ctypes.data, L.ptr(st2, ctypes.c_int64), L.ptr(out, ctypes.c_int32), cap, L.ptr(off, ctypes.c_int64))
            res.append((rc, st2, off, out))
    finally:
        ss.close()
    want_off = np.concatenate([[0], np.cumsum([len(h) for h in hits])])
    for rc, st2, off, out in res:
        assert off.tolist() == want_off.tolist() and off[n] == need           # hit_off is complete and gives the need
        assert np.array_equal(st2, st)                                         # and so are the statistics
    assert [r[0] for r in res] == [L.E_OVERFLOW, L.E_OVERFLOW, 0]
    assert np.array_equal(res[1][3][:len(hits[0])], hits[0])                   # (the pairs that fit are there)
    assert np.array_equal(res[2][3], np.concatenate(hits))
