"""The designed pairs of the join (join_designs) without a GPU: the restated geometry equals the headers', anyk_model and the C
oracle give the same dots for every design, every design reaches the class it is named for (a miss is a failure, never a skip),
and every mutant of the dots or of the record count is told from the right answer by a design of its own group."""
import os
import re

import numpy as np
import pytest

import join_designs as jd
import queue_case
from conftest import ROOT


def _src(name):
    with open(os.path.join(ROOT, "vapor_amd", "csrc", name)) as f:
        return f.read()


def _all():
    return [(g, p) for g, make in jd.GROUPS.items() for p in make()]


def test_restated_constants_equal_the_headers():
    kern, recs, plan = _src("vapor_kernels.h"), _src("vapor_records.h"), _src("vapor_planner.h")
    big = re.search(r"struct JoinBig \{([^}]*)\}", kern).group(1)
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+) = (\d+)", big)}
    assert (got["TA2"], got["TA4"], got["NB_LOG2"], got["FILT_LOG2"], got["QCAP"]) == (jd.TA2, jd.TA4, jd.NB_LOG2, jd.FILT_LOG2, jd.QCAP)
    assert "using JoinCfg = JoinBig;" in kern
    assert int(re.search(r"constexpr int JCHUNK = (\d+);", kern).group(1)) == jd.JCHUNK
    assert int(re.search(r"#define VAPOR_JQ_FAST_SLACK (\d+)", kern).group(1)) == jd.JQ_FAST_SLACK
    assert int(re.search(r"#define VREC_MAX_LEN (\d+)", kern).group(1)) == jd.VREC_MAX_LEN
    assert int(re.search(r"constexpr int MAX_READS_PER_TASK = (\d+);", recs).group(1)) == jd.MAX_READS_PER_TASK
    assert int(re.search(r"constexpr int X4_MERGE_MAX_K = (\d+);", kern).group(1)) == 40
    assert int(re.search(r"constexpr int X4_TWO_PER_LANE_MAX_K = (\d+);", kern).group(1)) == 20      # RB = 16 beyond it
    # the multipliers of canon_hash and the mode rule
    for word in ("0xC2B2AFu", "0x9E3779B1u", "0x85EBCA77u", "0xC2B2AE3Du", "0x2C1B3C6Du", "x ^= x >> 15"):
        assert word in kern, word
    assert "(s1.n_exc > 0 && s2.n_exc > 0) ? 4 : (s2.n_exc > 0 ? 3 : (s1.n_exc > 0 ? 5 : 2))" in plan


def test_bucket_equals_queue_case_at_k10():
    rng = np.random.default_rng(1)
    for _ in range(300):
        km = jd._rand(rng, 10)
        assert jd.bucket(km) == queue_case.bucket(km) == jd.bucket(jd.revcomp(km))
    for k in (20, 30, 40):
        km = jd._rand(rng, k)
        assert jd.bucket(km) == jd.bucket(jd.revcomp(km)) == jd.hashes("ACG" + km + "T", k)[3] >> (32 - jd.NB_LOG2)


def test_model_equals_oracle_on_every_design(oracle):
    n = 0
    for _g, p in _all():
        try:
            exp = oracle.dotdata_array(p.k, p.s1, p.allele)
            code = 0
        except KeyError:
            exp, code = np.zeros((0, 2), dtype=np.int32), jd.E_KEYERROR
        assert code == p.refused and np.array_equal(p.hits(), exp), p.name
        n += 1
    assert n == sum(len(make()) for make in jd.GROUPS.values()) > 500


def test_routes():
    for g, p in _all():
        if "route" in p.info:
            assert p.route == p.info["route"], p.name
        if "plane" in p.info:
            assert p.plane == p.info["plane"], p.name
        if p.name.endswith("_x4"):
            assert p.route == "x4", p.name
    for g in ("ends", "runs"):
        assert {p.route for p in jd.GROUPS[g]()} == set(jd.ROUTES)
        assert {(p.route, p.k) for p in jd.GROUPS[g]()} >= {(r, k) for r in jd.ROUTES for k in ((10, 30) if g == "runs" else jd.KS)}
    assert {p.RB for p in jd.runs()} == {16, 32} and {p.RB for p in jd.ends()} == {16, 32}


def test_buckets_reach_their_classes():
    ps = {p.name: p for p in jd.buckets()}
    for k in jd.KS:
        for m in (jd.BUCKET_M if k in (10, 40) else jd.THRESHOLD_M):
            for n in (jd.BUCKET_N if k in (10, 40) else (1,)):
                name = "k%d_m%d_n%d" % (k, m, n)
                p, low = ps[name], ps[name + "_x4"]
                assert p.mode == 2 and low.mode == 4 and (low.s1, low.s2) == (p.s1.lower(), p.s2.lower())
                assert p.nk1 == jd.JCHUNK and p.nk2_all <= jd.TA2
                assert jd.reaches(p, sizes=[m], totals=[n * m]), name
                w = jd.unit_kmers(m, n, k)
                assert len(p.hits()) >= n * w * m and len(low.hits()) == len(p.hits()), name
                # the multiplicity itself, from the sequences alone: every read position of the unit's lanes has m same-strand dots
                per_i = np.bincount(p.same_strand()[:, 1], minlength=jd.JCHUNK)
                lanes = range((64 - n) // 2, (64 - n) // 2 + n)
                assert all(per_i[16 * b + t] == m for b in lanes for t in range(w)), name
    have = {(p.k, p.info["m"], p.info["lanes"]) for p in ps.values() if "m" in p.info and p.mode == 2}
    for k in (10, 40):
        # both sides of every edge: 3 | 4 (one register), 511 | 512 (two), and a total of 128 | 129 (the fast path's slack)
        assert {(k, m, n) for m in jd.BUCKET_M for n in jd.BUCKET_N} <= have and {(k, 2, 64), (k, 3, 64), (k, 4, 32), (k, 5, 32)} <= have
        assert (2 * 64, 4 * 32) == (jd.FAST_MAX, jd.FAST_MAX)
        p = ps["k%d_mixed_3_4_512" % k]
        assert jd.reaches(p, mixed=(3, 4, 512), sizes=[512], totals=[530])
        p = ps["k%d_total_128_129" % k]
        cl = jd.bucket_classes(p)
        assert {t for c in cl if c[1] == 0 for t in c[4]} == {128} and {t for c in cl if c[1] == jd.JCHUNK for t in c[4]} == {129}
        assert all(c[5] == {4} for c in cl if c[1] == 0) and all(c[5] == {4, 5} for c in cl if c[1] == jd.JCHUNK)
    for k in (20, 30):
        assert {(k, m, 1) for m in jd.THRESHOLD_M} <= have


def test_tiles_reach_their_edges():
    ps = jd.tiles()
    for plane, TA in ((2, jd.TA2), (4, jd.TA4)):
        mine = [p for p in ps if p.info["plane"] == plane and p.name != "polyA_tile"]
        assert all(p.plane == plane and p.TA == TA for p in mine)
        for k in (10,) + ((30,) if plane == 4 else ()):
            assert {p.nk2_all for p in mine if p.k == k} == {TA, TA + 1, 2 * TA + 1}
            for nk2 in (TA, TA + 1, 2 * TA + 1):
                offs = {p.off2 for p in mine if p.k == k and p.nk2_all == nk2}
                assert offs >= {o for o in (0, TA - 1, TA, TA + 1, 2 * TA, nk2) if o <= nk2 + k - 1}, (plane, k, nk2)
        assert {p.k for p in mine if p.nk2_all == 2 * TA + 1 and p.off2 == TA} == set(jd.KS)
        for p in mine:
            assert p.nk2_all == p.info["nk2_all"], p.name
            a = set((p.same_strand()[:, 0].astype(np.int64) + p.off2).tolist())
            assert set(p.info["dots_a"]) <= a, p.name
            if len(p.allele) < p.k:
                assert len(p.hits()) == 0 and p.expected()[0][:3] == [0, -1, -1]
        # a dot on the last position of a tile and one on the first of the next, in and out of the window
        edge = [p for p in mine if p.name.endswith("_edge") and p.nk2_all > TA]
        assert any(p.info["dots_a"] == [TA - 1, TA] for p in edge) and any(p.info["dots_a"] == [TA] and p.off2 == TA for p in edge)
        assert any(p.off2 == TA + 1 and p.info["dots_a"] == [] for p in edge)
        if plane == 4:
            assert all(any(c.islower() for c in p.s1) and any(c.islower() for c in p.s2) for p in mine)
    p = ps[-1]
    assert p.name == "polyA_tile" and p.s2[:jd.TA2 + 9] == "A" * (jd.TA2 + 9) and p.s2[jd.TA2 + 9] != "A" and "C" + "A" * 12 + "G" in p.s1
    assert len(p.hits()) >= 3 * jd.TA2 == p.info["n_dots_min"] and len(p.hits()) < jd.MAX_DOTS
    assert jd.reaches(p, sizes=[jd.TA2])
    assert max(len(p.s2) for p in ps) <= 49252 + 40 and max(len(p.hits()) for p in ps) < jd.MAX_DOTS


def test_strips_reach_their_lengths():
    for k in jd.STRIP_K:
        mine = [p for p in jd.strips() if p.k == k]
        assert [p.nk1 for p in mine] == [0, 1, 2, 15, 0, 16, 17, 0, 1023, 1024, 1025, 2049, 0] and {p.nk1 for p in mine} == set(jd.STRIP_NK1)
        assert sorted(len(p.s1) for p in mine if p.nk1 == 0) == [1, k - 1, k - 1, k - 1]
        assert len({p.s2 for p in mine}) == 1 and len(mine[0].s2) == 3000
        for p in mine:
            assert p.nk1 == p.info["nk1"] and p.s1 in p.s2, p.name
            assert set(range(p.nk1)) == set(p.same_strand()[:, 1].tolist()), p.name          # every read position carries a dot
    # what the device sees: the planner (plan_pairs, vapor_planner.h) cuts tasks from the pairs that are not refused and have a
    # k-mer on both sides - restated in jd.joined(), its line held here - so a task's reads are the joined ones of an allele
    with open(os.path.join(ROOT, "vapor_amd", "csrc", "vapor_planner.h")) as f:
        assert "if (s1.len - a.k + 1 > 0 && s2.len - a.k + 1 > 0) order->push_back((int32_t)i);" in f.read()
    assert sum(jd.joined(p) for p in jd.strips()) == 2 * 9 and all(jd.joined(p) == (p.nk1 > 0) for p in jd.strips())
    for make, n in ((jd.strips_64, jd.MAX_READS_PER_TASK), (jd.strips_65, jd.MAX_READS_PER_TASK + 1)):
        ps = make()
        in_task = [p for p in ps if jd.joined(p)]
        assert len(in_task) == n and len({(p.mode, p.k, p.s2, p.off2) for p in in_task}) == 1, n       # one launch, one allele
        assert ps[0].nk1 == 0 == ps[-1].nk1 and sum(1 for p in ps if not jd.joined(p)) >= 20 and all(p.nk1 == p.info["nk1"] for p in ps)
        assert {p.nk1 for p in in_task} == set(jd.STRIP_NK1) - {0}
    ps = jd.strips_after()
    assert [p.s2 == ps[0].s2 for p in ps] == [True] * 3 + [False] * 13 and [p.nk1 for p in ps[:3]] == [0, 1491, 21]
    assert all(p.nk1 == p.info["nk1"] for p in ps) and ps[3].nk1 == 0 and len({p.s2 for p in ps[3:]}) == 1
    assert [jd.joined(p) for p in ps[:4]] == [False, True, True, False] and sum(jd.joined(p) for p in ps) == 11 <= jd.MAX_READS_PER_TASK


def test_ends_reach_the_padding():
    ps = {p.name: p for p in jd.ends()}
    for route in jd.ROUTES:
        for k in jd.KS:
            for base in "AT":
                t, r, a = (ps["%s_k%d_%s_%s" % (route, k, c, base)] for c in jd.END_CASES)
                assert t.s1.endswith("G" + base * 12) and t.s2.endswith("G" + base * 12)
                assert r.s1.endswith("G" + base * 12) and r.s2.endswith("G" + base * 40)
                assert a.s1.endswith("G" + base * 40) and a.s2.endswith("G" + base * 12)
                for p in (t, r, a):
                    assert p.route == route and p.refused == 0
                    # the last k-mer of the shorter tail is a dot, on the last k-mer of the side that ends first
                    i_end, j_end = p.nk1 - 1, p.nk2 - 1
                    hs = set(map(tuple, p.same_strand().tolist()))
                    want = (j_end, i_end) if p is t else (j_end - 28, i_end) if p is r else (j_end, i_end - 28)
                    assert want in hs, p.name
    p = ps["k40_read_N_first_last"]
    assert p.s1[0] == "N" == p.s1[-1] and p.mode == 5 and min(p.same_strand()[:, 1]) == 1 and max(p.same_strand()[:, 1]) == p.nk1 - 2
    p = ps["k40_allele_lower_first_last"]
    assert p.s2[0].islower() and p.s2[-1].islower() and p.mode == 3 and len(p.hits()) >= 461
    p = ps["k40_allele_ends_lower"]
    assert p.mode == 3 and max(p.same_strand()[:, 0]) == p.nk2 - 2
    p = ps["k40_read_refused"]
    assert p.refused == jd.E_KEYERROR and p.nk1 > 0 and p.expected() == ([0, -1, -1] + [0] * 11, jd.E_KEYERROR) and jd.records(p) == 0
    p = ps["k40_short_read_with_X"]
    assert p.refused == 0 and p.nk1 == 0 and "X" in p.s1 and len(p.hits()) == 0
    p = ps["k40_N_after_a_dot"]
    on = set(p.same_strand()[:, 1].tolist())
    for h, (lo, hi) in zip(p.info["heads_at"], p.info["dead"]):
        assert h % 32 == 0 and h in on and not (set(range(lo, hi + 1)) & on) and p.s1[hi] == "N"
    assert [lo - 1 - h for h, (lo, hi) in zip(p.info["heads_at"], p.info["dead"])] == [0, 1, 31]     # runs of 1, 2 and 32 dots
    assert [hi - h for h, (lo, hi) in zip(p.info["heads_at"], p.info["dead"])] == [40, 41, 71]
    for k in (10, 40):
        p = ps["k%d_N_across_strips" % k]
        on = set(p.same_strand()[:, 1].tolist())
        assert p.mode == 5 and p.s1[1023] == p.s1[1024] == "N" and p.nk1 > 1024 + 200
        assert 1023 - k in on and 1025 in on and not (set(range(1024 - k, 1025)) & on)
        p = ps["k%d_lower_across_strips" % k]
        assert p.mode == 3 and 1023 - k in set(p.same_strand()[:, 1].tolist()) and 1024 not in set(p.same_strand()[:, 1].tolist())


def test_runs_reach_their_heads():
    for p in jd.runs():
        assert p.RB == p.info["rb"] and p.route == p.info["route"], p.name
        same = p.same_strand()
        hd = jd.heads(p)
        if "diag" in p.info:
            a0, i0, n = p.info["diag"]
            on = (same[:, 0] + p.off2 - same[:, 1] == a0 - i0) & (same[:, 1] >= i0) & (same[:, 1] < i0 + n)
            assert on.sum() == n, p.name                                                       # the planted diagonal, whole
            ends_there = not ({(a0 - p.off2 - 1, i0 - 1), (a0 - p.off2 + n, i0 + n)} & set(map(tuple, same.tolist())))
            assert ends_there, p.name
            want = p.info["diag_heads"] if p.forms_runs else n
            assert hd[on].sum() == want, (p.name, int(hd[on].sum()), want)
        if "rc_min" in p.info:
            assert len(p.hits()) - len(same) >= p.info["rc_min"] > 0, p.name
        if p.forms_runs:
            assert jd.records(p) < len(p.hits()) or len(p.hits()) == 0, p.name
        else:
            assert jd.records(p) == len(p.hits()) and jd.n_invalid(p.s2) > 0, p.name
    names = {p.name for p in jd.runs()}
    for route in jd.ROUTES:
        for k in (10, 30):
            RB = 16 if route.startswith("x4") and k == 30 else 32
            for s in (0, 1, RB - 1, RB, RB + 1):
                assert "%s_k%d_start%d" % (route, k, s) in names
            for n in (RB - 1, RB, RB + 1, 2 * RB, 2 * RB + 1):
                assert "%s_k%d_len%d" % (route, k, n) in names
            assert {"%s_k%d_%s" % (route, k, x) for x in ("tile_edge", "off2_cut", "inverted")} <= names
    edge = [p for p in jd.runs() if p.name.endswith("tile_edge")]
    assert all(p.info["diag"][0] < p.TA < p.info["diag"][0] + p.info["diag"][2] for p in edge)


def test_strands_reach_their_kmers():
    for p in jd.strands():
        from collections import Counter
        c = Counter(map(tuple, p.hits().tolist()))
        assert p.info["dup"] and all(c[d] == 2 for d in p.info["dup"]), p.name
        assert all(c[d] == 1 for d in p.info["both"]), p.name
        j1, j2 = p.info["both"][0][0], p.info["both"][1][0]
        assert j2 - (j1 + p.k) == 5
        assert len(p.info["no_dots"]) == len({s for s in (0, 15, 16, 31, 32, p.k - 1) if s < p.k})
        for j, i in p.info["no_dots"]:
            a, b = p.allele[j:j + p.k], p.s1[i:i + p.k]
            assert sum(x != y for x, y in zip(a, b)) == 1 and c[(j, i)] == 0, p.name
        syms = sorted(next(t for t in range(p.k) if p.allele[j + t] != p.s1[i + t]) for j, i in p.info["no_dots"])
        assert syms == sorted({s for s in (0, 15, 16, 31, 32, p.k - 1) if s < p.k}), p.name
    assert {(p.k, p.plane, len(p.info["dup"])) for p in jd.strands()} == {(k, pl, n) for k in jd.KS for pl in (2, 4) for n in (1, 3)}


def test_records_rule_on_hand_counted_cases():
    """records() on pairs small enough to count by hand."""
    al = "GATTACAGGCTTAACGTCCATGCAAGTCTAGGACCTTGAACTGCATCGATCGGATACCTAG" * 2
    al = al[:60] + "TTGACCGATAGGCATTAGACCAGTTTAGACGATACCATGGTAATCGGCTAAGCTAGGCAT"
    P = jd.Pair
    # 41 dots on one diagonal from read position 0: heads at 0 and 32
    p = P("hand", "hand", al[10:60], al, 10, "")
    assert len(p.hits()) == 41 and jd.records(p) == 2
    # the same from off2 = 15: dots a = 15 .. 50 at i = 5 .. 40, heads at a = off2 and at i = 32
    p = P("hand", "hand", al[10:60], al, 10, "", off2=15)
    assert len(p.hits()) == 36 and jd.records(p) == 2
    # an allele with a symbol outside the folded alphabet against a lower-case read: the 4-bit planes without runs
    p = P("hand", "hand", al[10:60].lower(), al.lower() + "X", 10, "")
    assert (p.mode, p.forms_runs) == (4, False) and jd.records(p) == len(p.hits()) == 41
    p = P("hand", "hand", al[10:60].lower(), al.lower(), 30, "")
    assert (p.mode, p.RB) == (4, 16) and len(p.hits()) == 21 and jd.records(p) == 2


def test_every_mutant_is_caught():
    assert len(jd.MUTANTS) >= 12
    for how, (group, kind, _why) in jd.MUTANTS.items():
        killer = jd.kills(group, how)
        assert killer is not None, how
        p = next(p for p in jd.GROUPS[group]() if p.name == killer)
        pairs = jd.GROUPS[group]()
        assert jd.mutant(p, how, pairs, pairs.index(p))[0] == kind, how


def test_every_design_holds_its_claims():
    bad = [p.name for _g, p in _all() if not jd.claims_hold(p)]
    assert not bad, bad[:10]


def test_a_random_pair_of_the_same_lengths_misses_the_class():
    """What the class assertions are worth: in every group, a design replaced by a random pair of its lengths (its name, k, off2
    and claims kept) no longer holds its claims."""
    rng = np.random.default_rng(3)
    picks = {"buckets": ("k10_m4_n32", "k40_m512_n1", "k10_total_128_129", "k40_mixed_3_4_512"),
             "tiles": ("p2_k10_2TA+1_off0_edge", "p4_k30_TA+1_off%d_last" % (jd.TA4 - 1), "polyA_tile"),
             "strips": ("k10_r8_nk1023", "k40_r3_nk15"), "strips_64": ("n64_k10_r10_nk1025",), "strips_65": ("n65_k10_r1_nk1",),
             "strips_after": ("after_k10_r11_nk2049",),
             "ends": ("plain_k10_together_A", "plain_k40_read_first_T", "aexc_k20_allele_first_A", "k40_N_after_a_dot", "k10_N_across_strips"),
             "runs": ("plain_k10_start31", "x4_k30_len17", "plain_k10_tile_edge", "plain_k30_off2_cut", "rexc_k10_inverted"),
             "strands": ("k10_selfrc_x1", "k40_selfrc_x3")}
    assert set(picks) == set(jd.GROUPS)
    for g, names in picks.items():
        by = {p.name: p for p in jd.GROUPS[g]()}
        for name in names:
            p = by[name]
            q = jd.Pair(p.name, p.group, jd._rand(rng, len(p.s1)), jd._rand(rng, len(p.s2)), p.k, p.why, off2=p.off2, flags=p.flags, **p.info)
            assert jd.claims_hold(p) and not jd.claims_hold(q), name


def test_group_sizes_are_small():
    """No design exceeds about 200 000 dots or a 49 252-base allele; the totals per group are what the summary quotes."""
    for g, make in jd.GROUPS.items():
        ps = make()
        assert max(len(p.hits()) for p in ps) < jd.MAX_DOTS and max(len(p.s2) for p in ps) <= 2 * jd.TA2 + 140, g


@pytest.mark.parametrize("group", sorted(jd.GROUPS))
def test_expected_words_exist(group):
    """dot_designs.expected() states words 0-13 of every design (computed once per process, shared with the GPU test)."""
    for p in jd.GROUPS[group]():
        w, code = p.expected()
        assert len(w) == 14 and w[0] == len(p.hits()) and code == p.refused, p.name


def test_the_gpu_comparison_tells_every_mutant():
    """The GPU test's comparison (join_designs.diff), fed a mutant's answer in the device's place, reports the design."""
    for how, (group, kind, _why) in jd.MUTANTS.items():
        pairs = jd.GROUPS[group]()
        t = [p.name for p in pairs].index(jd.kills(group, how))
        p = pairs[t]
        _kind, value = jd.mutant(p, how, pairs, t)
        st = np.zeros((1, 16), dtype=np.int64)
        st[0, :14] = p.expected()[0]
        assert jd.diff([p], st, [p.hits()], [jd.records(p)]) == []
        hits, rec = (np.asarray(value, dtype=np.int32), jd.records(p)) if kind == "hits" else (p.hits(), value)
        assert len(jd.diff([p], st, [hits], [rec])) == 1, how
