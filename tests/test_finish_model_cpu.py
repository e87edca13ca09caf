"""tests/finish_model.py and tests/finish_cases.py kept honest without a GPU: the model against the reference's own outputs
(tests/golden), its np.mean order against np.mean, every mutant of the model killed by the designed tables, the check bodies
of tests/test_gpu_finish.py on the CPU twin (oracle/cpu_twin.cpp), and the host statements of the same operation in
vapor_amd/finish.py and vapor_amd/workload.py on the same tables."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import dot_designs as D
import finish_cases as C
import finish_model as M
import test_gpu_finish as G
from conftest import load_golden


@pytest.fixture(scope="module")
def twin(oracle):
    """vapor_amd._lib bound to the CPU twin for the duration of this module."""
    from vapor_amd import _lib
    so = oracle.build_twin()
    saved = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(so))
    yield so
    _lib._lib = saved


@pytest.fixture()
def eng(twin):
    from vapor_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def stats(twin):
    """The statistics of the pool's plan (every builder assertion of finish_cases runs on them)."""
    from vapor_amd.engine import Engine
    e = Engine(0)
    with G.pool_plan(e) as (_plan, st):
        C.gate_tables(st)
        C.locus_table(st)
    e.close()
    return st


def _nan_equal(a, b):
    return a == b or (a != a and b != b)


# ---------------------------------------------------------------------------------------------------------------------
# the model against the reference's outputs
# ---------------------------------------------------------------------------------------------------------------------
def _record(k, read, allele, off2):
    return D.SeqCase("golden", k, read, allele, off2).ref.words() + [0, 0]


@pytest.mark.parametrize("case", load_golden("scorers.json.gz")["cases"], ids=lambda c: c["name"])
def test_model_scorers_give_the_reference_outputs(oracle, case):
    k, x, miss = case["k"], case["read"], case["miss"]
    lr, la = len(case["ref"]), len(case["alt"])
    if "error" in case["s1"]:
        with pytest.raises(KeyError):
            _record(k, x, case["ref"], miss)
        failed = [0, -1, -1] + [0] * 12 + [-3]                            # what a plan returns for such a pair
        for kind in (0, 1, 2, 3):
            assert M.score(kind, failed, failed, failed, failed, lr, la) is None
        return
    r, a = _record(k, x, case["ref"], miss), _record(k, x, case["alt"], miss)
    ru, au = _record(k, x, case["ref"].upper(), miss), _record(k, x, case["alt"].upper(), miss)
    for key, fn, rr, aa, kind in (("s1", M.s1, ru, au, 1), ("s2", M.s2, r, a, 2), ("s3", M.s3, r, a, 3)):
        want = [float(v) for v in case[key]["ok"]]
        assert [float(v) for v in fn(rr, aa, lr, la)] == want, key
        got = M.score(kind, rr, aa, rr, aa, lr, la)
        assert (got is None) if 0 in want else (got == 1 - want[1] / want[0]), key
    # a deletion (SF:1716-1726)
    v = [M.score(1, ru, au, ru, au, lr, la), M.score(2, r, a, r, a, lr, la)]
    v = [s for s in v if s is not None]
    assert M.score(0, ru, au, r, a, lr, la) == (min(v) if v else None)


def _check_locus(scores, qs, gs, gt, gq, tag):
    from vapor_amd import finish
    got = M.locus(scores, finish.gt_table().tolist())
    assert got[0] == qs and got[1] == gs, tag
    assert got[4] == len(scores) and got[5] == len([s for s in scores if s > 0]) and got[7] == 0.0, tag
    if len(scores) < M.GT_TABLE_N:
        assert got[2] == gt and _nan_equal(got[3], gq), tag
    else:
        assert got[2] == 1 and got[3] != got[3], tag                      # (beyond the table: 0/1 without a quality)
    if len(scores) <= 256 and got[5] <= 128:
        assert M.qs_kernel(scores) == qs, tag


def test_model_loci_give_the_reference_outputs():
    import deep_cases as dc
    n = 0
    for c in load_golden("genotype.json.gz")["cases"]:
        org = c["organize"]["ok"]
        scores = [float(s) for s in c["scores"]]
        if org[1] == "NA":
            got = M.locus(scores, None)
            assert got[4] == 0.0 and all(v != v for q, v in enumerate(got) if q != 4)
            continue
        _check_locus(scores, float(org[1]), float(org[2]), ["0/0", "0/1", "1/1"].index(c["gt"]["ok"][0]), float(c["gt"]["ok"][1]), len(scores))
        n += 1
    assert n > 100
    for c in dc.DEEP:
        scores, qs, gs, gt, gq = dc.expected(c)
        _check_locus(scores, qs, gs, gt, gq, c["name"])


def test_qs_numpy_is_np_mean(stats):
    rng = np.random.default_rng(5152)
    lists = []
    for n in range(1, 301):
        lists.append((rng.random(n) * 10.0 ** rng.integers(-3, 3, n)).tolist())
        lists.append(rng.random(n).tolist())
    t, nl = C.locus_table(stats)
    sc = C.expected(stats, t, nl)[0]
    for li in range(nl):
        s = sc[t["locus"] == li]
        if (s > 0).any():
            lists.append(s[s > 0].tolist())
    assert max(map(len, lists)) >= 400
    for p in lists:
        assert M.qs_numpy(p) == np.mean(p), len(p)
        assert M.qs_numpy(p) == np.mean(np.array(p)), len(p)


# ---------------------------------------------------------------------------------------------------------------------
# the designed tables can tell every mutant from the model
# ---------------------------------------------------------------------------------------------------------------------
LOCUS_RULES = ("nonpos_unrounded", "table_le_65", "table_lt_64", "gs_ge", "sum_left_to_right", "partials_left_to_right", "partials_by_slot")


def test_every_mutant_is_killed(stats):
    P = C.pool()
    gates = C.gate_tables(stats)
    t_loci, nl = C.locus_table(stats)
    tables = [("gates %d" % k, t, C.count_loci(t)) for k, t in gates.items()] + [("loci", t_loci, nl)]
    # a failed pair's record as a plan returns it holds nothing to score with; to show that the model looks at word 15, the
    # two failed pairs get the words of a pair that scores
    poisoned = stats.copy()
    for f in P.failed:
        poisoned[f, :15] = stats[P.by_name["fin_abs250@k40"], :15]
    right = {}
    for name, t, n in tables:
        for st_name, st in (("", stats), ("poisoned ", poisoned)):
            sc = C.model_scores(st, t)
            right[st_name + name] = (sc, {(g, o): C.model_loci(sc, t, n, C.gt_tables()[g], o) for g in ("project", "zero", "cell") for o in ("numpy", "kernel")})
    assert all(G.same(np.array([np.nan if s is None else s for s in right[n][0]]), np.array([np.nan if s is None else s for s in right["poisoned " + n][0]])).all()
               for n, _t, _n in tables)
    killed = {}
    for m in M.MUTANTS:
        mod = M.mutant(m)
        # (a wrong rule of the reduction has to show on the locus table, which is made for it, a wrong scorer on the gate tables)
        for name, t, n in (tables[-1:] if m in LOCUS_RULES else tables[:-1]):
            key = ("poisoned " if m == "failed_record_used" else "") + name
            st = poisoned if m == "failed_record_used" else stats
            sc = C.model_scores(st, t, mod)
            if sc != right[key][0]:
                killed[m] = (name, "read scores")
                break
            for (g, o), want in right[key][1].items():
                if not G.same(C.model_loci(right[key][0], t, n, C.gt_tables()[g], o, mod), want).all():
                    killed[m] = (name, "locus records", g, o)
                    break
            if m in killed:
                break
    print(killed)
    assert sorted(killed) == sorted(M.MUTANTS), sorted(set(M.MUTANTS) - set(killed))


# ---------------------------------------------------------------------------------------------------------------------
# the bodies of tests/test_gpu_finish.py on the CPU twin
# ---------------------------------------------------------------------------------------------------------------------
def test_gates_on_the_twin(eng):
    G.check_gate_tables(eng, numpy_order=True)


def test_locus_table_on_the_twin(eng):
    G.check_locus_table(eng, numpy_order=True)


def test_genotype_tables_on_the_twin(eng):
    G.check_genotype_tables(eng, numpy_order=True)


def test_second_run_and_asynchronous_steps_on_the_twin(eng):
    G.check_second_run(eng, numpy_order=True)
    G.check_async_steps(eng, numpy_order=True)


def test_device_out_refusals_and_empty_table_on_the_twin(eng):
    G.check_device_out(eng, "cpu", numpy_order=True)                       # ("device" memory is host memory on the twin)
    G.check_refusals(eng, numpy_order=True)
    G.check_empty_read_table(eng, numpy_order=True)


# ---------------------------------------------------------------------------------------------------------------------
# the host statements of the same operation
# ---------------------------------------------------------------------------------------------------------------------
def _host_scalar(st, rd):
    """One read through finish.score_* and the drivers' rule as vapor_amd's drivers apply it."""
    from vapor_amd import finish
    fn = {1: finish.score_abs_dis_m1b, 2: finish.score_within_10Perc_m1b, 3: finish.score_directed_dis_m1b_redefine_diagnal}
    ra, aa, rb, ab, kind, _loc, lr, la = rd

    def one(k, r, a):
        x = fn[k](st[r], st[a], lr, la)
        return None if 0 in x else 1 - float(x[1]) / float(x[0])
    if kind == 0:
        v = [s for s in (one(1, ra, aa), one(2, rb, ab)) if s is not None]
        return min(v) if v else None
    return one(kind, ra, aa)


def _host_batch(st, t):
    from vapor_amd import finish
    kind = t["kind"]
    k1 = np.where(kind == 0, 1, kind)
    a, b, valid = finish.batch_scores(k1, st[t["ref_a"]], st[t["alt_a"]], t["len_ref"], t["len_alt"])
    sc = np.where(valid, finish.read_scores(a, b), np.nan)
    dele = kind == 0
    if dele.any():
        a2, b2, v2 = finish.batch_scores(np.where(dele, 2, 0), st[t["ref_b"]], st[t["alt_b"]], t["len_ref"], t["len_alt"])
        s2 = np.where(v2, finish.read_scores(a2, b2), np.nan)
        sc = np.where(dele, np.fmin(sc, s2), sc)                          # (fmin: the one that is not NaN, NaN when both are)
    return sc


def test_host_scorers_on_the_gate_tables(stats):
    for kind, t in C.gate_tables(stats).items():
        want = C.expected(stats, t)[0]
        got = np.array([np.nan if s is None else s for s in (_host_scalar(stats, rd) for rd in t.tolist())], dtype=np.float64)
        assert G.same(got, want).all(), (kind, "finish.score_*", np.flatnonzero(~G.same(got, want))[:5].tolist())
        got = _host_batch(stats, t)
        assert G.same(got, want).all(), (kind, "finish.batch_scores", np.flatnonzero(~G.same(got, want))[:5].tolist())


def test_host_locus_statements_on_the_locus_table(stats):
    from vapor_amd import finish
    t, nl = C.locus_table(stats)
    sc, _k = C.expected(stats, t, nl, "project", "kernel")
    _sc, want = C.expected(stats, t, nl, "project", "numpy")
    per = [[s for s in sc[t["locus"] == li].tolist() if s == s] for li in range(nl)]
    tails = finish.row_tails(per)
    for li, scores in enumerate(per):
        w = want[li]
        one = finish.row_tail(scores)
        assert tails[li][:4] == one[:4] or (tails[li][:3] == one[:3] and tails[li][3] != tails[li][3]), li
        if not scores:
            assert finish.locus_summary(scores) is None and one == ["NA"] * 5 and tails[li] == ["NA"] * 5 and w[4] == 0
            continue
        qs, gs, idx, gq = finish.locus_summary(scores)
        assert float(qs) == w[0] and gs == w[1], (li, "locus_summary")     # np.mean
        assert float(one[0]) == w[0] and one[1] == w[1], (li, "row_tail")  # _mean_like_numpy below 128 values, np.mean above
        assert float(tails[li][0]) == w[0] and tails[li][1] == w[1], (li, "row_tails")
        assert one[4] == ",".join(str(round(s, 2)) for s in scores) == tails[li][4]
        assert len([s for s in scores if not round(s, 2) > 0]) == w[6]
        if len(scores) < M.GT_TABLE_N:                                     # (the host computes (k, l) cells the table does not hold)
            assert (idx, finish.gt_name(idx)) == (int(w[2]), one[2]) and one[2] == tails[li][2], li
            assert _nan_equal(float(gq), w[3]) and _nan_equal(float(one[3]), w[3]) and _nan_equal(float(tails[li][3]), w[3]), li


def test_finish_workload_counts_on_the_tables(stats):
    """workload.finish_workload (the batch pipeline's host finish) reads pairs 2r / 2r + 1 for read r and has no within_10Perc
    kind of its own: the reads of kind 1 and 3, and the deletions whose two scorers take the same choice, with the statistics
    laid out that way.  Its counts, GS, GT and GQ are the model's (its QS is a plain sum and promises no order)."""
    from vapor_amd import workload as wl
    gates = C.gate_tables(stats)
    t0 = gates[0]
    t_loci, _nl = C.locus_table(stats)
    n_checked = 0
    for t in (gates[1], gates[3], t0[(t0["ref_a"] == t0["ref_b"]) & (t0["alt_a"] == t0["alt_b"])],
              t_loci[(t_loci["kind"] != 2) & ((t_loci["kind"] != 0) | ((t_loci["ref_a"] == t_loci["ref_b"]) & (t_loci["alt_a"] == t_loci["alt_b"])))]):
        nl = C.count_loci(t)
        st2 = np.empty((2 * len(t), stats.shape[1]), dtype=np.int64)
        st2[0::2], st2[1::2] = stats[t["ref_a"]], stats[t["alt_a"]]
        w = SimpleNamespace(read_kind=t["kind"], len_ref=t["len_ref"], len_alt=t["len_alt"], read_locus=t["locus"], n_loci=nl)
        got = wl.finish_workload(w, st2)
        _sc, want = C.expected(stats, t, nl, "project", "numpy")
        scored = want[:, 4] > 0
        assert np.isnan(got[~scored]).all()
        assert (got[scored, 4] == want[scored, 4]).all() and (got[scored, 1] == want[scored, 1]).all()
        small = scored & (want[:, 4] < M.GT_TABLE_N)
        assert (got[small, 2] == want[small, 2]).all() and G.same(got[small, 3], want[small, 3]).all()
        assert (np.abs(got[scored, 0] - want[scored, 0]) <= np.array([C.qs_bound(r) for r in want[scored]])).all()
        n_checked += int(scored.sum())
    assert n_checked > 300
