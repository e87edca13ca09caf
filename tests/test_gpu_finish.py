"""finish_kernel on designed read tables (tests/finish_cases.py) against tests/finish_model.py, a plain-Python float64 statement
of the scorers' gates, the per-read rule and the per-locus reduction that is no kernel.  Every comparison is bit for bit
(== on the doubles, NaN positions equal) and against the model: every read score, every locus's GS, GT, GQ, n, npos, nnonpos
and word 7, QS against the order the kernel documents (qs_kernel), and QS against np.mean's order (qs_numpy) for every locus
of at most 256 reads and at most 128 positives, where the two are the same function.  Beyond that QS is held to qs_numpy
within 2 m 2^-53 QS for m positives (finish_cases.qs_bound: either order of summing m positive doubles is within (m - 1) 2^-53
relative of the true sum, and the division adds a rounding on each side).

The bodies take an engine, so tests/test_finish_model_cpu.py runs them on the CPU twin as well.  The twin sums in numpy's
recursive order above 128 positives: there `numpy_order` holds it to qs_numpy exactly and to qs_kernel within the bound."""
import ctypes
from contextlib import contextmanager

import numpy as np
import pytest

import finish_cases as C
from vapor_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@contextmanager
def pool_plan(eng, with_failed=True):
    """(plan, statistics) of the pool's pairs, run once; without the two pairs that fail at plan creation on request (the
    indices of the others stay)."""
    P = C.pool()
    ss = eng.seqset(P.seqs)
    plan = eng.plan(ss, eng.make_pairs(P.rows if with_failed else P.rows[:P.n_ok]))
    try:
        st = plan.run().copy()
        full = st
        if not with_failed:                                 # (the model takes the records of the whole pool)
            full = np.zeros((len(P.rows), L.STATS_STRIDE), dtype=np.int64)
            full[:P.n_ok] = st
            full[P.n_ok:, 1:3] = -1
            full[P.n_ok:, L.ST_STATUS] = L.E_ARG
        C.check_pool(full)
        yield plan, full
    finally:
        plan.close()
        ss.close()


def set_reads(plan, t, n_loci, gt):
    """Plan.set_reads with the caller's genotype table."""
    plan.reads = np.ascontiguousarray(t, dtype=L.READ_DTYPE)
    plan.n_loci = int(n_loci)
    plan.gt = np.ascontiguousarray(gt, dtype=np.float64)
    assert plan.gt.shape == (L.GT_TABLE_N, L.GT_TABLE_N, 2)
    L.check(L.load().vapor_plan_set_reads(plan._h, len(plan.reads), plan.reads.ctypes.data_as(ctypes.c_void_p), plan.n_loci,
                                          L.ptr(plan.gt, ctypes.c_double)))
    plan.loci = np.zeros((max(plan.n_loci, 1), L.LOCUS_STRIDE), dtype=np.float64)
    plan.read_scores = np.zeros(max(len(plan.reads), 1), dtype=np.float64)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def without_failed(t):
    """The reads of a table that point at no failed pair."""
    n_ok = C.pool().n_ok
    return t[(t["ref_a"] < n_ok) & (t["alt_a"] < n_ok) & (t["ref_b"] < n_ok) & (t["alt_b"] < n_ok)]


def assert_records(loci, scores, st, t, n_loci, gt, numpy_order, tag):
    """Locus records and read scores of one run against the model of table `t` under genotype table `gt`."""
    exp_sc, exp_k = C.expected(st, t, n_loci, gt, "kernel")
    _sc, exp_n = C.expected(st, t, n_loci, gt, "numpy")
    assert loci.shape == (n_loci, L.LOCUS_STRIDE), tag
    if scores is not None:
        bad = np.flatnonzero(~same(scores, exp_sc))
        assert bad.size == 0, (tag, "read scores", bad[:5].tolist(), t[bad[:5]].tolist(), scores[bad[:5]].tolist(), exp_sc[bad[:5]].tolist())
    bad = np.argwhere(~same(loci[:, 1:], exp_k[:, 1:]))
    assert bad.size == 0, (tag, "locus words", bad[:5].tolist(), loci[bad[:5, 0]].tolist(), exp_k[bad[:5, 0]].tolist())
    n_reads = np.bincount(t["locus"], minlength=n_loci)
    scored = exp_k[:, 4] > 0
    inside = scored & (n_reads <= 256) & (exp_k[:, 5] <= 128)
    assert same(exp_k[inside, 0], exp_n[inside, 0]).all(), tag         # (the model's two orders are one function there)
    exact, near = (exp_n, exp_k) if numpy_order else (exp_k, exp_n)
    print("%s: %d reads, %d loci, %d beyond 256 reads / 128 positives; QS - qs_%s there: %s" % (
        tag, len(t), n_loci, int((scored & ~inside).sum()), "kernel" if numpy_order else "numpy",
        (loci[scored & ~inside, 0] - near[scored & ~inside, 0]).tolist()))
    bad = np.flatnonzero(~same(loci[:, 0], exact[:, 0]))
    assert bad.size == 0, (tag, "QS", bad[:5].tolist(), loci[bad[:5], 0].tolist(), exact[bad[:5], 0].tolist())
    bad = np.flatnonzero(~same(loci[inside, 0], near[inside, 0]))
    assert bad.size == 0, (tag, "QS, other order", bad[:5].tolist())
    for li in np.flatnonzero(scored & ~inside):
        assert abs(loci[li, 0] - near[li, 0]) <= C.qs_bound(near[li]), (tag, "QS bound", int(li), loci[li].tolist(), near[li].tolist())


def run_and_compare(plan, st, t, n_loci, gt, numpy_order, tag):
    set_reads(plan, t, n_loci, C.gt_tables()[gt])
    loci = plan.run_loci(want_scores=True).copy()
    scores = plan.read_scores[:len(t)].copy()
    assert_records(loci, scores, st, t, n_loci, gt, numpy_order, tag)
    return loci, scores


# ---------------------------------------------------------------------------------------------------------------------
# the bodies
# ---------------------------------------------------------------------------------------------------------------------
def check_gate_tables(eng, numpy_order=False):
    with pool_plan(eng) as (plan, st):
        for kind, t in C.gate_tables(st).items():
            run_and_compare(plan, st, t, C.count_loci(t), "project", numpy_order, "gates of kind %d" % kind)


def check_locus_table(eng, numpy_order=False):
    with pool_plan(eng) as (plan, st):
        t, nl = C.locus_table(st)
        run_and_compare(plan, st, t, nl, "project", numpy_order, "loci")
        loci, _sc = run_and_compare(plan, st, t, nl, "cell", numpy_order, "loci, cell table")
        # (the cell that was read, once more in words: GQ = 100 n + nnonpos + 0.25 for the loci the table serves)
        served = (loci[:, 4] > 0) & (loci[:, 4] < L.GT_TABLE_N)
        assert served.sum() >= 20 and (loci[served, 3] == 100 * loci[served, 4] + loci[served, 6] + 0.25).all()
        assert (loci[served, 6] != loci[served, 4] - loci[served, 5]).any()       # (a positive below 0.005 counts as not positive)
        beyond = loci[:, 4] >= L.GT_TABLE_N
        assert beyond.sum() >= 10 and (loci[beyond, 2] == 1).all() and np.isnan(loci[beyond, 3]).all()
        assert {63.0, 64.0, 65.0} <= set(loci[:, 4].tolist())


def check_genotype_tables(eng, numpy_order=False):
    """The three tables on one plan, one after the other and back to the first: the context's cached table (Plan.set_reads hands
    over the project's), a plan's own, and the release of either when the next one comes."""
    from vapor_amd import finish
    with pool_plan(eng) as (plan, st):
        t, nl = C.locus_table(st)
        plan.set_reads(t, nl)
        assert np.array_equal(finish.gt_table(), C.gt_tables()["project"])
        first = plan.run_loci(want_scores=True).copy()
        assert_records(first, plan.read_scores[:len(t)].copy(), st, t, nl, "project", numpy_order, "project table through Plan.set_reads")
        got = {}
        for gt in ("cell", "zero", "project", "zero", "cell", "project"):
            got.setdefault(gt, []).append(run_and_compare(plan, st, t, nl, gt, numpy_order, "table %s" % gt)[0])
        assert same(got["project"][0], first).all()
        for v in got.values():
            assert same(v[0], v[1]).all()
        scored = first[:, 4] > 0
        zero = got["zero"][0]
        # under the all-0/0 table the GS > .15 rule alone decides (beyond the table the genotype is 0/1 anyway)
        assert ((zero[scored, 2] == 1) == ((zero[scored, 1] > .15) | (zero[scored, 4] >= L.GT_TABLE_N))).all()
        assert (zero[scored & (zero[:, 1] == 0.15), 2] == 0).sum() >= 4 and (zero[scored, 2] == 1).any()


def check_second_run(eng, numpy_order=False):
    """vapor_plan_run_loci twice: the second call leaves the statistics on the device - unless a pair has a host-side status,
    whose record the host has to hand over again.  The same records either way."""
    for with_failed in (True, False):
        with pool_plan(eng, with_failed) as (plan, st):
            t = C.gate_tables(st)[0]
            if not with_failed:
                t = without_failed(t)
            nl = C.count_loci(t)
            a, sa = run_and_compare(plan, st, t, nl, "project", numpy_order, "first run, failed pairs %s" % with_failed)
            b = plan.run_loci(want_scores=True).copy()
            sb = plan.read_scores[:len(t)].copy()
            assert_records(b, sb, st, t, nl, "project", numpy_order, "second run, failed pairs %s" % with_failed)
            assert same(a, b).all() and same(sa, sb).all()
            assert np.array_equal(plan.run(), st[:plan.n])                    # (and the statistics route still gives the same)
            c = plan.run_loci().copy()
            assert same(a, c).all()


def check_async_steps(eng, numpy_order=False):
    """Three enqueued steps and one sync: the records are the pinned second copy the kernel writes itself."""
    with pool_plan(eng, with_failed=False) as (plan, st):
        t, nl = C.locus_table(st)
        t = without_failed(t)
        want, _sc = run_and_compare(plan, st, t, nl, "cell", numpy_order, "blocking run")
        plan.loci[:] = -7.0
        for _ in range(3):
            plan.run_loci_async()
        got = plan.sync().copy()
        assert_records(got, None, st, t, nl, "cell", numpy_order, "after three asynchronous steps")
        assert same(got, want).all()


def check_device_out(eng, device, numpy_order=False):
    """The records written into a torch tensor of n_loci x 8 doubles equal the host copy.  (In a process that has not used
    torch's device yet this test also pays for that, about ten seconds once; the suite's later torch tests then do not.)"""
    import torch
    with pool_plan(eng) as (plan, st):
        t, nl = C.locus_table(st)
        set_reads(plan, t, nl, C.gt_tables()["cell"])
        out = torch.full((nl, L.LOCUS_STRIDE), -3.0, dtype=torch.float64).to(device)      # (filled on the host: copies only, no kernel of torch's)
        host = plan.run_loci(device_out=out.data_ptr(), want_scores=True).copy()
        if device != "cpu":
            torch.cuda.synchronize()
        dev = out.cpu().numpy()
        assert same(dev, host).all()
        assert_records(dev, plan.read_scores[:len(t)].copy(), st, t, nl, "cell", numpy_order, "device_out")


def check_refusals(eng, numpy_order=False):
    """What vapor_plan_set_reads refuses, and that a refused table leaves the plan's table alone."""
    with pool_plan(eng) as (plan, st):
        t = C.gate_tables(st)[2][:200].copy()
        nl = C.count_loci(t)
        want, _sc = run_and_compare(plan, st, t, nl, "cell", numpy_order, "before the refusals")
        gt = C.gt_tables()["zero"]
        bad = t.copy()
        bad["locus"][50] = bad["locus"][49] - 1                 # not sorted by locus
        with pytest.raises(L.VaporHipError):
            set_reads(plan, bad, nl, gt)
        with pytest.raises(L.VaporHipError):
            set_reads(plan, t, nl - 1, gt)                      # a locus past n_loci
        for kind in (4, -1):
            bad = t.copy()
            bad["kind"][7] = kind
            with pytest.raises(L.VaporHipError):
                set_reads(plan, bad, nl, gt)
        for field, kind, idx in (("ref_a", 2, plan.n), ("alt_a", 2, -1), ("ref_b", 0, plan.n), ("alt_b", 0, 1 << 30)):
            bad = t.copy()
            bad["kind"][9] = kind
            bad[field][9] = idx
            with pytest.raises(L.VaporHipError):
                set_reads(plan, bad, nl, gt)
        plan.n_loci = nl
        plan.loci = np.zeros((nl, L.LOCUS_STRIDE), dtype=np.float64)
        assert same(plan.run_loci().copy(), want).all()


def check_empty_read_table(eng, numpy_order=False):
    with pool_plan(eng) as (plan, st):
        t = np.zeros(0, dtype=L.READ_DTYPE)
        loci, _sc = run_and_compare(plan, st, t, 5, "cell", numpy_order, "no reads, five loci")
        assert np.isnan(loci[:, [0, 1, 2, 3, 5, 6, 7]]).all() and (loci[:, 4] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
def test_gates(eng):
    check_gate_tables(eng)


def test_locus_sizes_and_summation_order(eng):
    check_locus_table(eng)


def test_genotype_tables_on_one_plan(eng):
    check_genotype_tables(eng)


def test_second_run_keeps_the_statistics_on_the_device(eng):
    check_second_run(eng)


def test_asynchronous_steps(eng):
    check_async_steps(eng)


def test_device_out(eng):
    check_device_out(eng, "cuda")


def test_set_reads_refusals(eng):
    check_refusals(eng)


def test_empty_read_table(eng):
    check_empty_read_table(eng)
