"""The window-aligned join task table on the device (parameter "join_align", vapor_amd/csrc/vapor_planner.h: plan_launch_aligned).

A pair's records must not depend on how the sorted pair list is cut into tasks: strips are cut per read, runs at 32-aligned read
positions, tiles per allele.  That is asserted here, not assumed: one small batch in which every way the two tables can differ
occurs - windows of 3 to 4 kb with 1, 2, 5, 6 and 9 reads of 1.5 kb, one window of 26 kb (two join tiles), one window with a
lower-case stretch and one read with an N (three launch modes), one INS locus, and behind the loci's pairs two reads against
a single window each (pairs no shared join serves: the planner shares the INS locus's like the others) - planned with
join_tasks 3 and 7 and reads_per_task 4, so that groups are cut into several ranges and there are more groups than tasks, is run
with join_align 0 and 2 on two plans over the same sequence set: the sixteen statistics of every pair, the record counts and
the per-locus records are equal bit for bit, while timings() reports other task counts and fewer table builds.  With
join_align 1 a blocking run_loci() and four asynchronous steps alternating over two plans - three of them on the aligned table
beside the balanced one, which timings() must show - give the same records again, and the oracle's (tests/workload_oracle.py, as tests/test_gpu_workloads.py compares them; the locus of the lower-case window is
left to the bit-for-bit comparisons: the oracle's scorers are stated for upper-case windows)."""
import numpy as np
import pytest

import workload_oracle as wo

pytestmark = pytest.mark.gpu

READ_LEN = 1500
#        type      window  reads
LOCI = [("DEL", 3500, 1), ("TANDUP", 3200, 2), ("DEL", 4000, 5), ("TANDUP", 3600, 6), ("DEL", 3300, 9), ("DEL", 26000, 3),
        ("DEL", 3400, 4), ("DEL", 3700, 3), ("INS", 3000, 2), ("DEL", 3100, 5)]
LOWER_LOCUS, N_LOCUS = 6, 7


def make_batch():
    """A vapor_amd.workload.Workload made locus by locus as make_workload makes its own, with the windows above."""
    from vapor_amd import _lib as L
    from vapor_amd import synth
    from vapor_amd import workload as wl
    rng = np.random.default_rng(20261020)
    lits, alts, segs, rows = [], [], [], []          # rows: (read, ("lit" | "alt", index), flags)
    read_locus, read_kind, len_ref, len_alt, types = [], [], [], [], []
    for li, (t, n_win, n_reads) in enumerate(LOCI):
        ref = synth.random_dna(rng, n_win)
        span = int(rng.integers(300, 900))
        s = int(rng.integers(n_win // 4, n_win // 2))
        if li == LOWER_LOCUS:
            ref = ref[:200] + ref[200:420].lower() + ref[420:]           # (before the breakpoint: both alleles carry it)
        ri = len(lits)
        lits.append(ref)
        if t == "DEL":
            alt, sg = ref[:s] + ref[s + span:], [(ri, 0, s, False), (ri, s + span, n_win - s - span, False)]
        elif t == "TANDUP":
            alt = ref[:s + span] + ref[s:s + span] + ref[s + span:]
            sg = [(ri, 0, s + span, False), (ri, s, span, False), (ri, s + span, n_win - s - span, False)]
        else:
            ins = synth.random_dna(rng, span)
            alt, sg = ref[:s] + ins + ref[s:], [(ri, 0, s, False), (len(lits), 0, span, False), (ri, s, n_win - s, False)]
            lits.append(ins)
        ai = len(alts)
        alts.append(alt)
        segs.append(sg)
        for r in range(n_reads):
            hap = alt if rng.random() < 0.5 else ref
            lo = max(0, s + span + 300 - READ_LEN)
            hi = max(lo, min(s - 150, len(hap) - READ_LEN))
            st = int(rng.integers(lo, hi + 1))
            rd = synth.mutate(rng, hap[st:st + READ_LEN + READ_LEN // 8].upper(), cigar=False)[0][:READ_LEN]
            if li == N_LOCUS and r == 1:
                rd = rd[:700] + "N" + rd[701:]
            q = len(lits)
            lits.append(rd)
            rows.append((q, ("lit", ri), wl.SCORER_FLAGS[t]))
            rows.append((q, ("alt", ai), wl.SCORER_FLAGS[t]))
            read_locus.append(li)
            read_kind.append({"DEL": 0, "TANDUP": 3}.get(t, 1))
            len_ref.append(len(ref))
            len_alt.append(len(alt))
        types.append(t)
    # two pairs that belong to no read of the table and share no join: a read against one window only
    first_read = {li: rows[2 * read_locus.index(li)][0] for li in (2, 4)}
    rows.append((first_read[2], ("lit", rows[2 * read_locus.index(3)][1][1]), wl.SCORER_FLAGS["DEL"]))
    rows.append((first_read[4], ("alt", 9), wl.SCORER_FLAGS["TANDUP"]))
    pairs = np.zeros(len(rows), dtype=L.PAIR_DTYPE)
    pairs["seq1"] = [q for q, _a, _f in rows]
    pairs["seq2"] = [i if kind == "lit" else len(lits) + i for _q, (kind, i), _f in rows]
    pairs["k"] = 10
    pairs["flags"] = [f for _q, _a, f in rows]
    return wl.Workload("join_align", lits + alts, pairs, np.asarray(read_locus), np.asarray(read_kind), np.asarray(len_ref), np.asarray(len_alt),
                       len(LOCI), types, len(lits), [(sg, False) for sg in segs])


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch():
    return make_batch()


@pytest.fixture(scope="module")
def expected(batch, oracle):
    """The oracle's answers, once (every locus but the one of the lower-case window)."""
    return wo.expect(oracle, batch, [li for li in range(batch.n_loci) if li != LOWER_LOCUS])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run_mode(eng, ss, w, align, join_tasks):
    """(statistics, record counts, per-locus records, timings) of a plan over `ss` made with join_align `align`."""
    from vapor_amd import workload as wl
    eng.set_param("join_align", align)
    eng.set_param("join_tasks", join_tasks)
    eng.set_param("reads_per_task", 4)
    p = eng.plan(ss, w.pairs)
    p.set_reads(wl.read_table(w), w.n_loci)
    st = p.run().copy()
    tm = p.timings()
    cnt = p.record_counts().copy()
    loci = p.run_loci().copy()
    p.close()
    return st, cnt, loci, tm


@pytest.mark.parametrize("join_tasks", [3, 7])
def test_records_do_not_depend_on_the_task_table(eng, batch, join_tasks):
    w = batch
    assert len(w.pairs) == 82
    ss = w.upload(eng)
    st0, cnt0, loci0, tm0 = run_mode(eng, ss, w, 0, join_tasks)
    st2, cnt2, loci2, tm2 = run_mode(eng, ss, w, 2, join_tasks)
    ss.close()
    print("join_tasks %d: balanced %d tasks, %d builds; aligned %d tasks, %d builds; %d launches" %
          (join_tasks, tm0["join_tasks"], tm0["table_builds"], tm2["join_tasks"], tm2["table_builds"], tm0["join_launches"]))
    assert (st0[:, 15] == 0).all() and int(st0[:80, 0].min()) > 0
    assert np.array_equal(st0, st2), np.argwhere(st0 != st2)[:6]
    assert np.array_equal(cnt0, cnt2), np.flatnonzero(cnt0 != cnt2)[:6]
    assert np.array_equal(bits(loci0), bits(loci2))
    # three launch modes (plain, an allele and a read with symbols outside upper-case ACGT), shared joins and pairs beside them
    assert tm0["join_launches"] == tm2["join_launches"] >= 3
    assert tm0["pairs_served_by_shared_joins"] == tm2["pairs_served_by_shared_joins"] == 80
    assert tm0["join_tasks"] != tm2["join_tasks"] and tm2["table_builds"] < tm0["table_builds"], (tm0, tm2)


def test_default_mode_blocking_and_asynchronous_steps(eng, batch, expected):
    """join_align 1 with join_tasks 3 and reads_per_task 4, where the planner's model makes the rule pay on this batch (an eighth of
    the tasks' sum saved, the dearest task a tenth dearer at most): blocking runs take the balanced table; of four asynchronous
    steps alternating over two plans the first finds no other plan's step enqueued and keeps it, the other three take the aligned
    one - by the host's own books, so timings() must show it - and every run's records are the same bits and the oracle's."""
    from vapor_amd import workload as wl
    w = batch
    ss = w.upload(eng)
    _st0, _cnt0, loci0, tm0 = run_mode(eng, ss, w, 0, 3)
    _st2, _cnt2, _loci2, tm2 = run_mode(eng, ss, w, 2, 3)
    balanced, aligned = (tm0["join_tasks"], tm0["table_builds"]), (tm2["join_tasks"], tm2["table_builds"])
    assert balanced != aligned
    eng.set_param("join_align", 1)
    eng.set_param("join_tasks", 3)
    eng.set_param("reads_per_task", 4)
    table = wl.read_table(w)
    plans = []
    for _ in range(2):
        p = eng.plan(ss, w.pairs)
        p.set_reads(table, w.n_loci)
        plans.append(p)
    sel = [li for li in range(w.n_loci) if li != LOWER_LOCUS]
    st = plans[0].run().copy()
    blocking = plans[0].run_loci(want_scores=True).copy()
    sc = plans[0].read_scores[:len(table)].copy()
    tm = plans[0].timings()
    assert (tm["join_tasks"], tm["table_builds"]) == balanced
    wo.check_plan(w, st, sc, blocking, expected, loci=sel, tag="join_align 1 blocking")
    assert np.array_equal(bits(blocking), bits(loci0))
    plans[1].run_loci(want_host=False)                  # (sizes the slots)
    plans[0].run_loci_async()
    assert (plans[0].timings()["join_tasks"], plans[0].timings()["table_builds"]) == balanced      # (nothing in flight beside it)
    for i in range(1, 4):
        plans[i % 2].run_loci_async()
        tm = plans[i % 2].timings()
        assert (tm["join_tasks"], tm["table_builds"]) == aligned, (i, tm, balanced, aligned)
    for q in plans:
        again = q.sync().copy()
        assert np.array_equal(bits(again), bits(blocking))
        wo.check_plan(w, st, None, again, expected, loci=sel, tag="join_align 1 asynchronous")
    # a plan that runs alone keeps the balanced table on its asynchronous steps too, and a blocking run after them
    plans[0].run_loci_async()
    tm = plans[0].timings()
    assert (tm["join_tasks"], tm["table_builds"]) == balanced
    assert np.array_equal(bits(plans[0].sync().copy()), bits(blocking))
    assert np.array_equal(bits(plans[1].run_loci().copy()), bits(blocking))
    tm = plans[1].timings()
    assert (tm["join_tasks"], tm["table_builds"]) == balanced
    for q in plans:
        q.close()
    ss.close()
