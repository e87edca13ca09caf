"""Designed dot plots (tests/dot_designs.py) through every route that turns a dot plot into the statistics record:
clean_kernel in its three instantiations, clean_big_kernel, the wide route's kernels, and the plan route (join, run records,
clean_kernel with the level-1 cache, shared joins).  Every comparison is exact, against dot_designs.expected(): words 0-13,
status word 15 == 0 and the per-dot flag bytes, at pair flags 1, 2, 3, 5 and 7.

The bodies take an engine; tests/test_dot_designs_cpu.py and tests/test_cpu_twin.py run the narrow ones on the CPU twin."""
import numpy as np
import pytest

import dot_designs as D
from vapor_amd import _lib as L

pytestmark = pytest.mark.gpu

WORDS = ("n_hits", "first_j", "last_j", "c1_kept", "c1_sum_abs", "c2_kept", "c2_count10", "n_diag", "n_lower", "c2_kept_diag",
         "dir_c2x", "dir_n", "dir_sum2", "dir_lists")


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _diff(errs, name, route, fl, got, want, got_flags=None, want_flags=None):
    if got[15] != 0:
        errs.append("design %s, route %s, flags %d: status %d" % (name, route, fl, got[15]))
    for w in range(14):
        if int(got[w]) != int(want[w]):
            errs.append("design %s, route %s, flags %d, word %d (%s): got %d, expected %d" % (name, route, fl, w, WORDS[w], got[w], want[w]))
    if want_flags is not None and not np.array_equal(got_flags, want_flags):
        bad = np.flatnonzero(np.asarray(got_flags) != np.asarray(want_flags)) if len(got_flags) == len(want_flags) else []
        errs.append("design %s, route %s, flags %d: flag bytes differ (%d dots, first at %s)" % (name, route, fl, len(bad), list(bad[:3])))


def _report(errs):
    assert not errs, "%d disagreements, the first:\n%s" % (len(errs), "\n".join(errs[:25]))


def check_lists(fn, route, cases):
    """Every case at every flag set through one list entry point (fn = eng.clean_hits or eng.clean_hits_wide): one call, one
    batch, per flag set."""
    errs = []
    lists = [c.hits for c in cases]
    for fl in D.FLAG_SETS:
        st, hf = fn(lists, flags=[fl] * len(lists))
        for t, c in enumerate(cases):
            want, want_flags = c.ref.expected(fl)
            _diff(errs, c.name, route, fl, st[t], want, hf[t], want_flags)
    _report(errs)


def check_small_lists(eng, band, wide=False, n_random=200):
    cases = D.small_cases(band, n_random)
    if band is not None:
        per = -(-D.rw_of(cases) // 256)                 # launch_clean: bitmap words per thread of the batch
        assert (per <= 4, 4 < per <= 8, per > 8)[band], (band, per)
    check_lists(eng.clean_hits_wide if wide else eng.clean_hits, ("wide_lists" if wide else "clean_kernel<%s>" % ("4", "8", "MAX")[band]), cases)


def check_big_lists(eng, wide=False):
    check_lists(eng.clean_hits_wide if wide else eng.clean_hits, "wide_lists_big" if wide else "clean_big_kernel", D.big_cases())


def check_wide_lists(eng, part):
    cases = D.wide_cases()
    check_lists(eng.clean_hits_wide, "wide_lists", cases[part::3])


def check_plan(eng, cases, route, flag_sets=D.FLAG_SETS, wide=False):
    """The cases as (read, allele, off2, k) pairs through a plan (join -> run records -> clean) and plan.fetch_hits: words 0-13,
    status, the dots and their flag bytes; then, wide, through eng.score_wide as well: words 0-13 the oracle's and all sixteen
    words the plan's.  Returns the plan's statistics."""
    seqs, rows, owner = [], [], []
    for c in cases:
        b = len(seqs)
        seqs += [c.read, c.allele]
        for fl in flag_sets:
            rows.append((b, b + 1, c.off2, c.k, fl))
            owner.append(c)
    ss = eng.seqset(seqs)
    pairs = eng.make_pairs(rows)
    errs = []
    try:
        plan = eng.plan(ss, pairs)
        try:
            st = plan.run().copy()
            hits, hf, off = plan.fetch_hits(range(plan.n), want_flags=True)
            rec = plan.record_counts().copy()
        finally:
            plan.close()
        for t, c in enumerate(owner):
            fl = rows[t][4]
            want, want_flags = c.ref.expected(fl)
            h, f = hits[off[t]:off[t + 1]], hf[off[t]:off[t + 1]]
            o = np.lexsort((f, h[:, 1], h[:, 0]))
            eo = np.lexsort((want_flags, c.hits[:, 1], c.hits[:, 0]))
            if not np.array_equal(h[o], c.hits[eo]):
                errs.append("design %s, route %s, flags %d: the dots differ from dotdata's (%d, expected %d)" % (c.name, route, fl, len(h), len(c.hits)))
                continue
            _diff(errs, c.name, route, fl, st[t], want, f[o], want_flags[eo])
        if wide:
            wst = eng.score_wide(ss, pairs)
            for t, c in enumerate(owner):
                _diff(errs, c.name, "score_wide", rows[t][4], wst[t], c.ref.expected(rows[t][4])[0])
                if not np.array_equal(wst[t], st[t]):
                    errs.append("design %s, flags %d: score_wide %s != score %s" % (c.name, rows[t][4], wst[t].tolist(), st[t].tolist()))
    finally:
        ss.close()
    _report(errs)
    return st, rec


def check_sequences(eng, wide=False):
    cases = D.sequence_cases()
    st, rec = check_plan(eng, cases, "plan", wide=wide)
    return st, rec


def check_doubled_33kb(eng, wide=False):
    c = D.doubled_33kb_case()
    st, rec = check_plan(eng, [c], "plan_big", flag_sets=(7, 2, 5), wide=wide)
    assert int(st[0, 0]) > 65535                        # more dots than clean_kernel's 16-bit counters take: clean_big_kernel
    return st, rec


# The window of the served group is 3 000 bases and the derived stretch is 450 .. 2 550.  With k = 20 a read k-mer that matches the
# window at j inside the stretch matches the inversion allele's other strand at j' = 3000 - 20 - j: a forward segment
# (d, j0, n) of the read becomes the reverse-complement run (2980 - j0 - t, j0 + d + t), i - j = 2 j0 + d - 2980 + 2 t.
# rc_run_in_winner: the segment (-20, 1500, 12) becomes a run with i - j = 0, 2, ..., 22 beside three segments in the left
# flank, which the inversion leaves alone: i - j = 12 x 40, 300 x 11 and 3500 x 11.  Level 1 (range 3500) puts all but the last
# into list 0; level 2 (range 300) puts the whole run and the 40 into sub-list 0: one longest sub-list of 52 whose median, 12, is
# taken over a 12-dot reverse-complement run, and the far pass walks that run at c = 12.
RC_RUN_IN_WINNER = D.Design("rc_run_in_winner", "a kept reverse-complement run inside the winning list (against the inversion allele)",
                            [(-20, 1500, 12), (12, 100, 40), (300, 200, 11), (3500, 300, 11)])


def served_group():
    """A window, and an inversion and a tandem duplication of its middle described as derived sequences; reads built from
    designs against the window, moved 1 000 along both axes so that their segments lie inside the derived stretch: there a
    design's forward segments are reverse-complement runs of the inversion allele (records of more than one dot, which only a
    shared join's cut of an inverted slice makes) and are doubled in the duplication allele."""
    def make():
        designs = [RC_RUN_IN_WINNER] + [D.BY_NAME[n].shift(1000, 1000) for n in
                                        ("x0_inside_even", "median_half", "anti_in_winner", "tie_l1", "far_exact", "anti_60")]
        names = [d.name for d in designs]
        reads, win = [], None
        for d in designs:
            # (every read against the same window: build_pair draws the allele first, so one seed gives one window)
            rd, al = D.build_pair(np.random.default_rng(4321), 20, d, min_len=3000, max_len=3001)
            assert win is None or al == win
            win = al
            reads.append(rd)
        n, f = len(win), 450
        mid = win[f:n - f]
        derived = [([(0, 0, f, False), (0, f, n - 2 * f, True), (0, n - f, f, False)], False),
                   ([(0, 0, n - f, False), (0, f, n - 2 * f, False), (0, n - f, f, False)], False)]
        texts = [win, win[:f] + D.revcomp(mid) + win[n - f:], win[:n - f] + mid + win[n - f:]]
        cases = []
        for r, (name, rd) in enumerate(zip(names, reads)):
            for a, tag in enumerate(("window", "inversion", "duplication")):
                cases.append((r, a, D.SeqCase("%s/%s@k20" % (name, tag), 20, rd, texts[a], (0, 7)[r % 2] if r else 0)))
        return win, reads, derived, cases
    return D._once("served", make)


def check_served_group(eng, route, want_shared=True):
    win, reads, derived, cases = served_group()
    seqs = [win] + reads
    first_der = len(seqs)
    rows, owner = [], []
    for r, a, c in cases:
        for fl in (7, 5, 3):
            rows.append((1 + r, 0 if a == 0 else first_der + a - 1, c.off2, c.k, fl))
            owner.append(c)
    errs = []
    eng.set_param("remap_in_clean", route)
    try:
        ss = eng.seqset(seqs, derived=derived)
        try:
            plan = eng.plan(ss, eng.make_pairs(rows))
            try:
                st = plan.run().copy()
                hits, hf, off = plan.fetch_hits(range(plan.n), want_flags=True)
                tm = plan.timings()
            finally:
                plan.close()
        finally:
            ss.close()
    finally:
        eng.set_param("remap_in_clean", 1)
    if want_shared:
        assert tm["pairs_served_by_shared_joins"] > 0, tm
        assert tm["remap_in_clean"] == (1 if route == 2 else 0), tm      # remap_kernel / the clean workgroups' remap_for_target
    for t, c in enumerate(owner):
        fl = rows[t][4]
        want, want_flags = c.ref.expected(fl)
        h, f = hits[off[t]:off[t + 1]], hf[off[t]:off[t + 1]]
        o = np.lexsort((f, h[:, 1], h[:, 0]))
        eo = np.lexsort((want_flags, c.hits[:, 1], c.hits[:, 0]))
        if not np.array_equal(h[o], c.hits[eo]):
            errs.append("design %s, route served(%d), flags %d: the dots differ from dotdata's" % (c.name, route, fl))
            continue
        _diff(errs, c.name, "served(%d)" % route, fl, st[t], want, f[o], want_flags[eo])
    _report(errs)


# ---- route 1: eng.clean_hits, small lists: clean_kernel<4>, <8>, <CLEAN_PER_MAX> with one-dot records ----
@pytest.mark.parametrize("band", [0, 1, 2])
def test_small_lists_in_each_clean_kernel(eng, band):
    check_small_lists(eng, band)


# ---- route 2: eng.clean_hits, big lists: clean_big_kernel ----
def test_big_lists(eng):
    check_big_lists(eng)


# ---- route 3: eng.clean_hits_wide ----
def test_wide_route_small_lists_unchanged(eng):
    check_small_lists(eng, None, wide=True, n_random=60)
    check_lists(eng.clean_hits_wide, "wide_lists", [D._case(D.OWN_3270), D._case(D.OWN_4096)])


def test_wide_route_big_lists_unchanged(eng):
    check_big_lists(eng, wide=True)


@pytest.mark.parametrize("part", [0, 1, 2])
def test_wide_route_beyond_65535(eng, part):
    check_wide_lists(eng, part)


# ---- routes 4 and 5: eng.score / plan.fetch_hits and eng.score_wide on sequence-built designs ----
def test_sequences_on_the_plan_and_wide_routes(eng):
    st, rec = check_sequences(eng, wide=True)
    assert int((rec < st[:, 0]).sum()) > len(rec) // 2          # (run records: fewer records than dots)


def test_doubled_33kb_reaches_the_big_kernel_from_run_records(eng):
    st, rec = check_doubled_33kb(eng, wide=True)
    assert int(rec[0]) * 8 < int(st[0, 0])


@pytest.mark.parametrize("route", [0, 2])
def test_group_served_by_a_shared_join(eng, route):
    check_served_group(eng, route)
