"""The designed pairs of tests/join_designs.py on the plan route (join_kernel -> clean kernels).  Every comparison is exact: the
dots sorted by (j, i) equal anyk_model's; words 0-13 of the record equal dot_designs.expected() under the pair's flags and word
15 the expected status; with shared joins off, the run records the join wrote number join_designs.records().  Each group then
runs with shared joins on and cut into tasks of one read and into one task of 64: the same dots and words.  Last, the wide and
the any-k route must agree with the plan on dots and words 0-13."""
import numpy as np
import pytest

import join_designs as jd

pytestmark = pytest.mark.gpu

# what _plan puts back.  join_tasks is really set from the device's CU count when the engine is made and cannot be read back, so
# every test gets an engine of its own: its first plan - the one whose records are counted - and the shared-join plan run at the
# engine's real defaults, and only the wide and any-k calls, which cut no join tasks, come after a change of join_tasks.
DEFAULTS = {"shared_join": 1, "reads_per_task": 64, "join_tasks": 256}


@pytest.fixture
def eng():
    from vapor_amd.engine import Engine
    from vapor_amd import _lib as L
    assert L.E_KEYERROR == jd.E_KEYERROR and L.MAX_SEQ_LEN >= 2 * jd.TA2 + 140
    e = Engine(0)
    yield e
    e.close()


def _table(pairs):
    seqs, at = [], {}
    for p in pairs:
        for s in (p.s2, p.s1):
            if s not in at:
                at[s] = len(seqs)
                seqs.append(s)
    return seqs, [(at[p.s1], at[p.s2], p.off2, p.k, p.flags) for p in pairs]


def _plan(eng, ss, pr, n, **params):
    """(statistics, record counts, dots per pair sorted by (j, i)) of one plan under the parameters."""
    for name, v in params.items():
        eng.set_param(name, v)
    try:
        plan = eng.plan(ss, pr)
        try:
            st = plan.run().copy()
            rec = plan.record_counts().copy()
            hits, _fl, off = plan.fetch_hits(range(n), want_flags=False)
        finally:
            plan.close()
    finally:
        for name in params:
            eng.set_param(name, DEFAULTS[name])
    out = []
    for t in range(n):
        h = hits[off[t]:off[t + 1]]
        out.append(h[np.lexsort((h[:, 1], h[:, 0]))])
    return st, rec, out


def _group(eng, pairs, one_task=False):
    seqs, rows = _table(pairs)
    n = len(pairs)
    ss = eng.seqset(seqs)
    try:
        pr = eng.make_pairs(rows)
        base = {"shared_join": 0}
        if one_task:
            base["join_tasks"] = 1
        st, rec, hits = _plan(eng, ss, pr, n, **base)
        errs = jd.diff(pairs, st, hits, rec)
        assert not errs, "%d differences:\n%s" % (len(errs), "\n".join(errs[:20]))
        for params in ({"shared_join": 1}, {"reads_per_task": 1, "join_tasks": 512}, {"reads_per_task": 64, "join_tasks": 1}):
            st2, _rec, hits2 = _plan(eng, ss, pr, n, **params)
            assert np.array_equal(st2[:, :14], st[:, :14]) and np.array_equal(st2[:, 15], st[:, 15]), params
            assert all(np.array_equal(a, b) for a, b in zip(hits, hits2)), params
        # the wide and the any-k route: the same dots, the same words 0-13
        w_st, w_hits = eng.score_wide(ss, pr, want_hits=True)
        a_st, a_hits = eng.score_anyk(ss, pr, want_hits=True)
        for name, o_st, o_hits in (("wide", w_st, w_hits), ("anyk", a_st, a_hits)):
            assert np.array_equal(o_st[:, :14], st[:, :14]) and np.array_equal(o_st[:, 15], st[:, 15]), name
            bad = [p.name for p, a, b in zip(pairs, hits, o_hits) if not np.array_equal(a, b)]
            assert not bad, (name, bad[:10])
    finally:
        ss.close()


@pytest.mark.parametrize("ks", [(10,), (40,), (20, 30)])
def test_buckets(eng, ks):
    _group(eng, [p for p in jd.buckets() if p.k in ks])


def test_tiles(eng):
    _group(eng, jd.tiles())


@pytest.mark.parametrize("group", ["strips", "strips_64", "strips_65", "strips_after"])
def test_strips(eng, group):
    """join_tasks = 1: the strip prefix runs over every read of the allele that has a k-mer - 9, 64 (a full task), 65 (two tasks),
    and 9 behind another allele's.  The reads without a k-mer never enter a task (the planner drops them): they are held to
    status 0, no dots and no records among the others."""
    pairs = jd.GROUPS[group]()
    assert sum(jd.joined(p) for p in pairs) == {"strips": 18, "strips_64": 64, "strips_65": 65, "strips_after": 11}[group]
    _group(eng, pairs, one_task=True)


def test_ends(eng):
    _group(eng, jd.ends())


def test_runs(eng):
    _group(eng, jd.runs())


def test_strands(eng):
    _group(eng, jd.strands())
