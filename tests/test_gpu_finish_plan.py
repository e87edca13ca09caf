"""The finishing and grid calls around their host plan (vapor_amd/csrc/vapor_finish_plan.h): what the existing
finish and refine tests do not reach.  The read tables are rows of tests/finish_cases.py's gate tables on its pool of pairs, the
expected records and scores are tests/finish_model.py's through finish_cases.expected, the expected choice is refine.pick's.

  * the grid's refusals on a live plan of 3 loci and 4 reads, each with its message, and the plan running on afterwards;
    vapor_plan_set_grid before vapor_plan_set_reads; vapor_plan_set_reads dropping the grid.  Two of the grid's five refusals
    cannot be met through a plan: its read ranges are counts, so none decreases, and the winners' slots pass 2^31 only beyond 2^31
    reads.  Those two are tools/finish_plan_check.cpp's alone.
  * vapor_plan_run_grid with each of its three outputs null in turn, over groups of 1, 2, 64 and 128 candidates and a group
    without reads;
  * vapor_plan_run_grid, then vapor_plan_run_loci: the arrays of the earlier call are not written again;
  * vapor_grid_pick against vapor_plan_set_grid + vapor_plan_run_grid on the same tables, with 5 groups (odd: the image's tables
    start where a packed block's would not) and with 6.

The repeat of a light run whose pair outgrew its slot, with grid outputs present, is not here: on one plan with unchanged engine
parameters the blocking first run sizes every slot for the dots the same sequences give again, so no second run overflows.  That
branch is the decision table of tools/finish_plan_check.cpp."""
import ctypes

import numpy as np
import pytest

import finish_cases as C
import test_gpu_finish as F
from vapor_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def rows_of(st):
    """The reads of the four gate tables that point at no failed pair: what the tables here are drawn from."""
    return np.concatenate([F.without_failed(C.gate_tables(st)[kind]) for kind in (0, 1, 2, 3)])


def table_of(rows, pick, locus):
    t = rows[np.asarray(pick, dtype=np.int64)].copy()
    t["locus"] = locus
    return t


def candidates_table(st, sizes, n_reads, seed):
    """(table, first_locus, read_first): group g has sizes[g] candidates (loci) of n_reads[g] reads each, drawn from the gate tables."""
    rows = rows_of(st)
    rng = np.random.default_rng(seed)
    pick, locus, first, read_first = [], [], [0], [0]
    for n, r in zip(sizes, n_reads):
        for _ in range(n):
            pick += rng.integers(0, len(rows), r).tolist()
            locus += [len(read_first) - 1] * r
            read_first.append(read_first[-1] + r)
        first.append(first[-1] + n)
    return table_of(rows, pick, locus), np.asarray(first, dtype=np.int32), np.asarray(read_first, dtype=np.int32)


def expected_choice(recs, scores, first, read_first):
    """What vapor_plan_run_grid hands out, from every candidate's record and scores: refine.pick per group."""
    from vapor_amd import refine
    widx, out, win, off = [], [], [], [0]
    for a, b in zip(first[:-1], first[1:]):
        w = refine.pick(recs[a:b])
        widx.append(w)
        out.append(np.concatenate([recs[a + w], recs[a]]))
        win.append(scores[read_first[a + w]:read_first[a + w + 1]])
        off.append(off[-1] + len(win[-1]))
    return np.asarray(widx, dtype=np.int32), np.asarray(out), np.concatenate(win), np.asarray(off, dtype=np.int64)


def run_grid(plan, n_groups, n_scores, null=None):
    """vapor_plan_run_grid with output `null` (0 winner_idx, 1 group_out, 2 winner_scores) left out; the arrays are pre-filled."""
    idx = np.full(n_groups, -5, dtype=np.int32)
    rec = np.full((n_groups, 2 * L.LOCUS_STRIDE), -5.0)
    sc = np.full(max(n_scores, 1), -5.0)
    off = np.full(n_groups + 1, -5, dtype=np.int64)
    args = [L.ptr(idx, ctypes.c_int32), L.ptr(rec, ctypes.c_double), L.ptr(sc, ctypes.c_double)]
    if null is not None:
        args[null] = None
    L.check(L.load().vapor_plan_run_grid(plan._h, args[0], args[1], args[2], L.ptr(off, ctypes.c_int64)))
    return idx, rec, sc, off


def refused(what, call):
    with pytest.raises(L.VaporHipError) as e:
        call()
    assert e.value.code == L.E_ARG and str(e.value).endswith(": " + what), str(e.value)


def test_grid_refusals_on_a_live_plan(eng):
    with F.pool_plan(eng, with_failed=False) as (plan, st):
        refused("vapor_plan_set_grid: call vapor_plan_set_reads first", lambda: plan.set_grid([0, 1]))
        refused("vapor_plan_run_grid: call vapor_plan_set_grid first", lambda: run_grid(plan, 1, 1))
        rows = rows_of(st)
        t = table_of(rows, [3, len(rows) // 4, len(rows) // 2, len(rows) - 5], [0, 0, 1, 2])      # 3 loci of 2, 1 and 1 reads
        gt = C.gt_tables()["cell"]
        F.set_reads(plan, t, 3, gt)
        refused("vapor_plan_run_grid: call vapor_plan_set_grid first", lambda: run_grid(plan, 1, 1))

        def runs_on(tag):
            loci = plan.run_loci(want_scores=True).copy()
            F.assert_records(loci, plan.read_scores[:len(t)].copy(), st, t, 3, "cell", False, tag)
            return loci
        runs_on("before the refusals")
        plan.set_grid([0, 1, 3])                                                     # (a grid the refused ones leave in place)
        want = [a.copy() for a in run_grid(plan, 2, 3)]
        for what, first_locus in (("grid: the groups must cover the loci", [0, 1, 2]),
                                  ("grid: the groups must cover the loci", [1, 3]),
                                  ("grid: the groups must cover the loci", [0, 1, 4]),
                                  ("grid: a group holds 1 .. VAPOR_MAX_CANDIDATES consecutive loci", [0, 0, 3]),
                                  ("grid: a group holds 1 .. VAPOR_MAX_CANDIDATES consecutive loci", [0, 1, 1, 3]),
                                  ("grid: a group holds 1 .. VAPOR_MAX_CANDIDATES consecutive loci", [0, 1, 0, 3]),
                                  ("grid: a group holds 1 .. VAPOR_MAX_CANDIDATES consecutive loci", [0, -1, 3]),
                                  ("grid: the candidates of a group score the same reads", [0, 2, 3]),
                                  ("grid: the candidates of a group score the same reads", [0, 3])):
            refused(what, lambda: plan.set_grid(first_locus))
            runs_on("after '%s' for %s" % (what, first_locus))
        for a, b in zip(run_grid(plan, 2, 3), want):
            assert a.tobytes() == b.tobytes()
        # a new read table drops the grid
        F.set_reads(plan, t, 3, gt)
        refused("vapor_plan_run_grid: call vapor_plan_set_grid first", lambda: run_grid(plan, 2, 3))
        runs_on("after the new read table")
        # no groups over these loci do not cover them; over no loci they do, and there is nothing to run
        refused("grid: the groups must cover the loci", lambda: plan.set_grid([0]))
        F.set_reads(plan, t[:0], 0, gt)
        plan.set_grid([0])
        refused("vapor_plan_run_grid: call vapor_plan_set_grid first", lambda: run_grid(plan, 1, 1))


# 5 groups over 134 loci: winner_idx (5 entries) and read_first (135) have odd lengths, first_locus and score_off (6) even ones
SIZES, N_READS = (1, 2, 128, 2, 1), (3, 2, 2, 0, 1)


@pytest.fixture(scope="module")
def grid_case(eng):
    """One plan with the candidates' read table set and run: (plan, table, first_locus, read_first, the device's records and
    scores, the expected choice from the model's)."""
    with F.pool_plan(eng, with_failed=False) as (plan, st):
        t, first, read_first = candidates_table(st, SIZES, N_READS, 11)
        nl = int(first[-1])
        F.set_reads(plan, t, nl, C.gt_tables()["project"])
        loci = plan.run_loci(want_scores=True).copy()
        scores = plan.read_scores[:len(t)].copy()
        F.assert_records(loci, scores, st, t, nl, "project", False, "the candidates")
        exp_sc, exp_loci = C.expected(st, t, nl, "project", "kernel")
        yield plan, t, first, read_first, loci, scores, expected_choice(exp_loci, exp_sc, first, read_first)


def assert_choice(got, want, null=None):
    (idx, rec, sc, off), (widx, wout, wwin, woff) = got, want
    assert off.tolist() == woff.tolist()
    if null != 0:
        assert idx.tolist() == widx.tolist()
    if null != 1:
        assert F.same(rec, wout).all()
    if null != 2:
        assert F.same(sc[:len(wwin)], wwin).all()
    for q, a in enumerate((idx, rec, sc)):
        if null == q:
            assert (a == -5).all()                                                   # (an output left out is not written)


def test_run_grid_with_each_output_null(grid_case):
    plan, t, first, read_first, _loci, _scores, want = grid_case
    assert (want[0] != 0).any() and len(want[2]) == 3 + 2 + 2 + 0 + 1
    plan.set_grid(first)
    assert_choice(run_grid(plan, len(SIZES), len(want[2])), want)
    for null in (0, 1, 2):
        assert_choice(run_grid(plan, len(SIZES), len(want[2]), null), want, null)
    # score_off left out as well: the engine's own call reads it, this one does not
    idx = np.zeros(len(SIZES), dtype=np.int32)
    L.check(L.load().vapor_plan_run_grid(plan._h, L.ptr(idx, ctypes.c_int32), None, None, None))
    assert idx.tolist() == want[0].tolist()


def test_run_loci_after_run_grid_writes_nothing_of_the_grid_call(grid_case):
    plan, t, first, _read_first, loci, scores, want = grid_case
    plan.set_grid(first)
    got = run_grid(plan, len(SIZES), len(want[2]))
    assert_choice(got, want)
    kept = [a.copy() for a in got]
    for a in got[:3]:
        a[...] = -9                                                                  # (what a write after the call would replace)
    again = plan.run_loci(want_scores=True).copy()
    assert F.same(again, loci).all() and F.same(plan.read_scores[:len(t)], scores).all()
    assert all((a == -9).all() for a in got[:3]) and got[3].tolist() == kept[3].tolist()


def test_grid_pick_equals_set_grid_and_run_grid(eng, grid_case):
    plan, t, first, read_first, loci, scores, want = grid_case
    six = np.asarray([0, 1, 3, 67, 131, 133, 134], dtype=np.int32)                  # the 128 candidates as two groups of 64
    for fl in (first, six):
        plan.set_grid(fl)
        n_sc = int((read_first[fl[:-1] + 1] - read_first[fl[:-1]]).sum())
        by_plan = run_grid(plan, len(fl) - 1, n_sc)
        by_call = eng.grid_pick(loci, fl, read_first, scores)
        assert by_call[0].tolist() == by_plan[0].tolist() and by_call[3].tolist() == by_plan[3].tolist() and int(by_plan[3][-1]) == n_sc
        assert by_call[1].tobytes() == by_plan[1].tobytes() and by_call[2].tobytes() == by_plan[2][:n_sc].tobytes()
        if fl is first:
            assert_choice(by_plan, want)
        else:
            exp = expected_choice(loci, scores, fl, read_first)
            assert_choice(by_plan, exp)
