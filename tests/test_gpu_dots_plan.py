"""Where the host plan of the explicit-dot routes (vapor_amd/csrc/vapor_dots_plan.h) decides something no other GPU test pins.
Expectations are anyk_model's dots and dot_designs' words (both held to the reference's goldens), never the library's.  Pinned
elsewhere and not repeated: the sort's sizes 512 .. 8192 and the edit cut at 4, 8, 64 and the shipped size
(test_gpu_anyk_designs.py: test_sort_sizes, test_edit_split, test_edit_split_default), the capacity protocol
(test_gpu_anyk_designs.py::test_batch_state, test_gpu_wide.py::test_mixed_batch_overflow_then_rerun), the dot bound as
"max_pair_cap" (test_gpu_wide.py::test_count_pass_stops_at_max_pair_cap), the cleaning's scratch up to the coordinate cap
(test_gpu_wide.py::test_clean_hits_wide_against_oracle, test_gpu_dot_designs.py's wide lists).  Beyond 2^31 - 1 dots the bound is
checked on the host alone (tests/test_dots_plan_cpu.py)."""
import ctypes

import numpy as np
import pytest

import anyk_designs as ad
import dot_designs as dd

pytestmark = pytest.mark.gpu

E_ARG, E_KEYERROR = -4, -3


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    from vapor_amd import _lib as L
    assert (L.E_ARG, L.E_KEYERROR, L.PF_FORWARD) == (E_ARG, E_KEYERROR, ad.PF_FORWARD)
    e = Engine(0)
    yield e
    e.close()


def _dna(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def _by_ji(h):
    return h[np.lexsort((h[:, 1], h[:, 0]))]


def _planted(rng, read, length=300):
    """An allele of `length` symbols that holds the read forward and, behind it, reverse complemented."""
    al = list(_dna(rng, length))
    al[5:5 + len(read)] = read
    at = 12 + len(read)
    al[at:at + len(read)] = ad.revcomp(read)
    assert len(al) == length
    return "".join(al)


def test_wide_hash_table_edges(eng):
    """k = 10, reads of 10, 137 and 138 bases: 1, 128 and 129 k-mers, tables of 4, 512 and 1024 buckets (2, 256 and 258 entries:
    the table exactly half full, and one entry past it)."""
    rng = np.random.default_rng(4091)
    ps = []
    for n in (10, 137, 138):
        rd = _dna(rng, n)
        ps.append(ad.Pair("read%d" % n, "hash_edges", rd, _planted(rng, rd), 10, False, "%d k-mers" % (n - 9), flags=7))
    assert [p.n for p in ps] == [2, 256, 258]
    seqs = [s for p in ps for s in (p.s1, p.s2)]
    pr = eng.make_pairs([(2 * t, 2 * t + 1, 0, 10, 7) for t in range(3)])
    ss = eng.seqset(seqs)
    try:
        wst, whits = eng.score_wide(ss, pr, want_hits=True)
        ast, ahits = eng.score_anyk(ss, pr, want_hits=True)
        pst = eng.score(ss, pr)
    finally:
        ss.close()
    for t, p in enumerate(ps):
        want, code = p.expected()
        assert code == 0 and len(p.hits()) >= 2 * (len(p.s1) - 9), p.name            # (both plantings give dots)
        assert np.array_equal(whits[t], _by_ji(p.hits())) and np.array_equal(ahits[t], p.hits()), p.name
        assert wst[t, :14].tolist() == want and wst[t, 15] == 0, (p.name, wst[t].tolist(), want)
    assert np.array_equal(wst, ast) and np.array_equal(wst, pst)


def _raw_batch(eng, entry, ss, rows, cap):
    from vapor_amd import _lib as L
    fn = eng._wide_entry(entry)
    pr = np.ascontiguousarray(eng.make_pairs(rows), dtype=L.PAIR_DTYPE)
    n = len(rows)
    st = np.full((n, 16), 99, dtype=np.int64)
    off = np.full(n + 1, -7, dtype=np.int64)
    out = np.full((max(cap, 1), 2), -1, dtype=np.int32)
    rc = fn(eng._ctx, ss._h, n, pr.ctypes.data, L.ptr(st, ctypes.c_int64), L.ptr(out, ctypes.c_int32), cap, L.ptr(off, ctypes.c_int64))
    return rc, st, off, out


@pytest.mark.parametrize("entry,bad_k", [("vapor_wide_batch", 15), ("vapor_anyk_batch", 65)])
def test_refusal_order_in_a_live_batch(eng, entry, bad_k):
    """Scored pairs between refused and empty ones.  Where a pair breaks two rules the earlier one's status stands: a sequence of
    2^20 symbols that also holds an X is too long (E_ARG), not a KeyError; so is a read with an X at an unsupported k or with a
    negative off2; the X alone is the KeyError.  A read shorter than k and an off2 at the allele's end are no refusals: status 0,
    no dots.  Every scored pair equals the same pair scored alone, and hit_off counts every pair."""
    rng = np.random.default_rng(4092)
    rd, rd2 = _dna(rng, 200), _dna(rng, 150)
    al = _planted(rng, rd[20:150])
    al = al[:280] + ad.revcomp(rd2[:20])
    bad = rd[:90] + "X" + rd[91:]
    too_long = "X" + "A" * ((1 << 20) - 1)
    seqs = [rd, al, rd2, bad, too_long, rd[:5]]
    RD, AL, RD2, BAD, LONG, SHORT = range(6)
    rows = [(RD, AL, 0, 10, 3), (LONG, AL, 0, 10, 3), (RD, AL, 7, 10, 7), (BAD, AL, 0, bad_k, 3), (SHORT, AL, 0, 10, 3), (RD2, AL, 0, 10, 3),
            (RD, AL, 300, 10, 3), (BAD, AL, 0, 10, 3), (BAD, AL, -1, 10, 3), (AL, LONG, 0, 10, 3), (RD, AL, 0, 10, 5)]
    status = [0, E_ARG, 0, E_ARG, 0, 0, 0, E_KEYERROR, E_ARG, E_ARG, 0]
    scored = [0, 2, 5, 10]
    wide = entry == "vapor_wide_batch"
    exp = {}
    for t in scored:
        s1, s2, off2, k, fl = rows[t]
        p = ad.Pair("row%d" % t, "refusal_order", seqs[s1], seqs[s2], k, False, "scored", off2=off2, flags=fl)
        exp[t] = (p.expected()[0], _by_ji(p.hits()) if wide else p.hits())
        assert len(exp[t][1]) > 0
    ss = eng.seqset(seqs)
    try:
        rc, st, off, out = _raw_batch(eng, entry, ss, rows, 1 << 14)
        alone = {t: _raw_batch(eng, entry, ss, [rows[t]], 1 << 14) for t in scored}
    finally:
        ss.close()
    assert rc == 0 and st[:, 15].tolist() == status
    want_off = [0]
    for t in range(len(rows)):
        want_off.append(want_off[-1] + (len(exp[t][1]) if t in exp else 0))
        if t not in exp:
            assert st[t].tolist() == [0, -1, -1] + [0] * 12 + [status[t]], (t, st[t].tolist())
    assert off.tolist() == want_off and want_off[-1] <= 1 << 14
    for t in scored:
        h = out[off[t]:off[t + 1]]
        assert np.array_equal(_by_ji(h) if wide else h, exp[t][1]), t
        assert st[t, :14].tolist() == exp[t][0], (t, st[t].tolist(), exp[t][0])
        rc1, st1, off1, out1 = alone[t]
        assert rc1 == 0 and st1[0].tolist() == st[t].tolist() and off1.tolist() == [0, len(h)], t
        assert np.array_equal(_by_ji(out1[:len(h)]), _by_ji(h)) and (wide or np.array_equal(out1[:len(h)], h)), t


def test_all_eight_flag_values_on_both_routes(eng):
    """flags 0 .. 7 on one 200 x 300 pair: which cluster passes run, whether the flag bytes are only zeroed, whether the directed
    statistics are computed (4 and 6 ask for them without C1 and get zeros)."""
    rng = np.random.default_rng(4093)
    rd = _dna(rng, 200)
    al = _planted(rng, rd[:130])
    ps = [ad.Pair("flags%d" % f, "flag_values", rd, al, 10, False, "flags %d" % f, flags=f) for f in range(8)]
    pr = eng.make_pairs([(0, 1, 0, 10, f) for f in range(8)])
    ss = eng.seqset([rd, al])
    try:
        wst = eng.score_wide(ss, pr)
        ast = eng.score_anyk(ss, pr)
    finally:
        ss.close()
    words = set()
    for f, p in enumerate(ps):
        want, code = p.expected()
        assert code == 0 and wst[f, :14].tolist() == want and wst[f, 15] == 0, (f, wst[f].tolist(), want)
        words.add(tuple(want))
    assert np.array_equal(wst, ast)
    assert ps[7].expected()[0][3] > 0 and ps[7].expected()[0][5] > 0 and ps[7].expected()[0][11] + ps[7].expected()[0][13] > 0     # (the pair has something to say under every flag)
    assert len(words) == 6                                                           # (0 = 4, 2 = 6; the others differ)


def _raw_lists(eng, fn, lists, flags):
    from vapor_amd import _lib as L
    n = len(lists)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(a) for a in lists], out=off[1:])
    allh = np.ascontiguousarray(np.concatenate(list(lists) + [np.zeros((1, 2), np.int32)]), dtype=np.int32)
    st = np.full((n, 16), 99, dtype=np.int64)
    hf = np.full(max(int(off[-1]), 1), 0xEE, dtype=np.uint8)
    fl = None if flags is None else L.ptr(np.asarray(flags, dtype=np.uint32), ctypes.c_uint32)
    L.check(fn(eng._ctx, n, L.ptr(allh, ctypes.c_int32), L.ptr(off, ctypes.c_int64), fl, L.ptr(st, ctypes.c_int64), L.ptr(hf, ctypes.c_uint8)))
    return st, [hf[off[t]:off[t + 1]] for t in range(n)]


def test_clean_hits_wide_empty_single_and_default_flags(eng):
    """An empty list between two others, a list of one dot, and flags = NULL (C1 and C2): the model's words and flag bytes, and
    vapor_clean_hits' on the same lists."""
    from vapor_amd import _lib as L
    rng = np.random.default_rng(4094)
    rd = _dna(rng, 200)
    p = ad.Pair("lists", "lists", rd, _planted(rng, rd[:130]), 10, False, "a 200 x 300 pair's dots")
    h = _by_ji(p.hits()).astype(np.int32)
    lists = [h, np.zeros((0, 2), np.int32), h[::3].copy(), np.asarray([[7, 3]], np.int32)]
    for flags in (None, [3, 3, 3, 3], [7, 5, 1, 2]):
        wst, wfl = _raw_lists(eng, eng._wide_entry("vapor_clean_hits_wide"), lists, flags)
        nst, nfl = _raw_lists(eng, L.load().vapor_clean_hits, lists, flags)
        for t, a in enumerate(lists):
            want, want_fl = dd.expected(a, 3 if flags is None else flags[t])
            assert wst[t, :14].tolist() == want and wst[t, 15] == 0, (flags, t, wst[t].tolist(), want)
            assert np.array_equal(wfl[t], want_fl) and np.array_equal(nfl[t], want_fl), (flags, t)
            assert nst[t, :14].tolist() == want and nst[t, 15] == 0, (flags, t, nst[t].tolist(), want)
        assert wst[1].tolist() == [0, -1, -1] + [0] * 13 and wst[3, :3].tolist() == [1, 7, 7]
