"""tests/dot_designs.py checked without a GPU: its reference against the vectors the reference program wrote, its designs
against the mutants of that reference (what the designs can tell apart is computed from the reference alone), its sequence
builder against the oracle's dotdata, and the narrow list bodies of tests/test_gpu_dot_designs.py on the CPU twin (the
sequence bodies run in tests/test_cpu_twin.py)."""
import ctypes

import numpy as np
import pytest

import dot_designs as D
from conftest import load_golden


def test_expected_reproduces_the_reference_vectors(oracle):
    """Every field of tests/golden/cleaners.json.gz that test_cleaners_golden compares, from expected() instead of a device."""
    from vapor_amd import finish
    cases = load_golden("cleaners.json.gz")["cases"]
    for c in cases:
        h = np.asarray(c["hits"], dtype=np.int32).reshape(-1, 2)
        w, fl = D.expected(h, 7)
        st = np.asarray(w + [0, 0], dtype=np.int64)
        if "r4" in c and "ok" in c["r4"]:
            assert st[10] == int(round(2 * float(c["r4"]["ok"]))), c["name"]
            assert float(finish._dir_value(st)) == float(c["dir"]["ok"]), c["name"]
        assert h[(fl & 1) > 0].tolist() == c["c1"]["ok"], c["name"]
        assert sorted(map(tuple, h[(fl & 2) > 0].tolist())) == sorted(map(tuple, c["c2_diag"]["ok"])), c["name"]
        assert sorted(map(tuple, h[(fl & 4) > 0].tolist())) == sorted(map(tuple, c.get("c2_anti_on_left", {"ok": []})["ok"])), c["name"]
        if "count10" in c:
            assert st[6] == c["count10"], c["name"]
        if "meanabs" in c:
            assert float(st[4]) / float(st[3]) == c["meanabs"], c["name"]
        assert st[0] == len(h) and st[1] == h[:, 0].min() and st[2] == h[:, 0].max()


def test_flag_masks_follow_the_twin(oracle):
    h = D.BY_NAME["anti_60"].dots()
    full, fb = D.expected(h, 7)
    assert full[3] and full[5] and full[9] and full[13] and set(fb.tolist()) == {1 | 2, 1 | 4}
    for fl in D.FLAG_SETS:
        w, f = D.expected(h, fl)
        assert w[:3] == full[:3] and w[7:9] == full[7:9]
        assert w[3:5] == (full[3:5] if fl & 1 else [0, 0])
        assert [w[5], w[6], w[9]] == ([full[5], full[6], full[9]] if fl & 2 else [0, 0, 0])
        assert w[10:14] == (full[10:14] if fl & 4 else [0, 0, 0, 0])
        assert np.array_equal(f, fb & ((1 if fl & 1 else 0) | (6 if fl & 2 else 0)))


def test_named_designs_reach_their_rules(oracle):
    """What the comments in dot_designs._named() promise, read off the reference: c2x, the number of longest sub-lists, and that
    C1 keeps every segment of at least 11 dots whole."""
    want = {"single": (10, 1), "range1_zero": (10, 1), "tie_l1": (0, 2), "tie_l2": (0, 2), "tie_3way": (0, 3), "tie_10way": (0, 10),
            "range2_zero": (40, 1), "edge_int_r100": (20, 1), "edge_prime_r97": (26, 1), "max_ties_l9": (0, 2), "max_beats_l9": (200, 1),
            "max_not_in_l9": (10, 1), "median_half": (23, 1), "median_odd": (26, 1), "x0_inside_even": (-60, 1), "x0_inside_odd": (-61, 1),
            "x0_y0": (-60, 1), "far_exact": (0, 1), "anti_in_winner": (0, 1), "g10_only": (0, 0), "gap10": (0, 0)}
    for name, (c2x, n_lists) in want.items():
        w = D._case(D.BY_NAME[name]).ref.words()
        assert (w[10], w[13]) == (c2x, n_lists), (name, w)
    for d in D.NAMED:
        c = D._case(d)
        seg = sum(n * (2 if q in d.dup else 1) for q, (_d, _j, n) in enumerate(d.fwd) if n >= 11) + sum(n for _j, _i, n in d.anti if n >= 11)
        assert c.ref.words()[3] >= seg, d.name
    # far rule and count10 at their exact values: one dot less is counted than when the rule is met by one
    assert D._case(D.BY_NAME["far_exact"]).ref.words()[11] == 10 and D._case(D.BY_NAME["far_below"]).ref.words()[11] == 11
    assert D._case(D.BY_NAME["far_above"]).ref.words()[11] == 0
    assert [D._case(D.BY_NAME[n]).ref.words()[6] for n in ("c10_exact", "c10_below", "c10_above")] == [10, 0, 11]
    # groups of 10 / 11 and 50 / 51, gaps of 9 / 10
    assert D._case(D.BY_NAME["g10_g11"]).ref.words()[3] == 11 and D._case(D.BY_NAME["g50_g51"]).ref.words()[9] == 51
    assert D._case(D.BY_NAME["g50_only"]).ref.words()[9] == 50 and D._case(D.BY_NAME["tie_below_51"]).ref.words()[9] == 60
    assert D._case(D.BY_NAME["gap9"]).ref.words()[3] == 24 and D._case(D.BY_NAME["gap10"]).ref.words()[3] == 0
    # every dot its own group: C1 keeps none, C2's largest group is 1 so it keeps all
    for d in (D.OWN_3270, D.OWN_4096):
        w = D._case(d).ref.words()
        assert w[3] == 0 and w[5] == w[0] == d.n_dots()


def test_r4_lists_is_the_oracles_function_step_by_step(oracle):
    """r4_lists() spells dis_to_diagnal_most_abundant_defined out to count the longest sub-lists; its c is that function's."""
    n = 0
    for c in D.small_cases() + D.sequence_cases() + D.wide_cases()[::5]:
        kept = [x for x, k in zip(c.hits.tolist(), c.ref.k1) if k]
        if kept:
            cc, n_lists, lists = D.r4_lists(kept)
            ref = oracle.dis_to_diagnal_most_abundant_defined(list(kept))
            assert cc == ref and type(cc) is type(ref) and n_lists == len(lists) >= 1, c.name
            n += 1
    assert n > 300


def test_transforms_keep_ties_and_edges(oracle):
    for name in ("tie_l1", "tie_l2", "tie_10way", "median_half", "edge_int_r100", "max_not_in_l9", "x0_inside_even", "x0_y0", "far_exact"):
        d = D.BY_NAME[name]
        w = D.Reference(d.dots()).words()
        for e in (d.scale(7), d.shift(70000, 0), d.shift(500, 500), d.stretch(900)):
            v = D.Reference(e.dots()).words()
            f = 900 if e.name.endswith("x900") else 1
            off = 2 * 70000 if "+(70000" in e.name and v[13] == 1 else 0
            assert v[13] == w[13] and v[10] == f * w[10] - off, (e.name, v, w)
        # a shift along j leaves the far rule's cases alone (where c is a median and moves with the shift)
        assert w[13] != 1 or D.Reference(d.shift(70000, 0).dots()).words()[11:13] == w[11:13], name


@pytest.mark.parametrize("which", ["small", "big", "wide", "sequence"])
def test_every_mutant_differs_somewhere_in_every_case_set(oracle, which):
    """Computed from the reference alone: each deliberately wrong variant of expected() differs from it on at least one case of
    the set in one of words 0-13.  (If one survives, a design is missing - the mutant stays.)"""
    cases = {"small": lambda: D.small_cases(), "big": D.big_cases, "wide": D.wide_cases, "sequence": D.sequence_cases}[which]()
    if which == "small":
        cases = cases + D.small_cases(0)[-2:] + D.small_cases(2)[-4:]
    if which == "wide":
        assert all(int(c.hits.max()) > D.MAX_SEQ for c in cases)
        lim = (1 << 24) // 10
        assert sum(1 for d in D.stretched() if d.d_range()[1] - d.d_range()[0] > lim) >= 3
    killed = D.killers([(c.name, c.ref) for c in cases])
    assert sorted(killed) == sorted(D.MUTANTS) and len(D.MUTANTS) == 12
    assert not [m for m, v in killed.items() if not v], killed


def test_sequence_cases_reach_the_record_format_cases(oracle):
    by = {c.name: c for c in D.sequence_cases()}
    # the X == 0 dot strictly inside a same-strand run: (30, 30) with c = -30, on a 30-dot diagonal that starts at j = 10
    names = [n for n in by if n.startswith("x0_inside_even@k")]
    assert len(names) >= 2                                # (once at k = 10, where loose dots join in, and once above)
    for name in names:
        c = by[name]
        w = c.ref.words()
        dots = set(map(tuple, c.hits.tolist()))
        assert w[10] == -60 and w[13] == 1
        assert all((30 + t, 30 + t) in dots for t in range(-20, 10)) and (9, 9) not in dots      # t0 = 20 > 0 in that run
        assert c.ref.k1[c.hits.tolist().index([30, 30])]
    # kept reverse-complement dots in the winning list: the anti segment's dot with i - j == 0 is in the one longest sub-list
    c = [v for n, v in by.items() if n.startswith("anti_in_winner@")][0]
    kept = [x for x, k in zip(c.hits.tolist(), c.ref.k1) if k]
    cc, n_lists, lists = D.r4_lists(kept)
    assert n_lists == 1 and cc == 0 and [305, 305] in kept and lists[0].count(0) == 41
    # odd c2x
    assert [v for n, v in by.items() if n.startswith("median_half@")][0].ref.words()[10] == 23
    # a segment gives exactly its n dots wherever random k-mers cannot collide (k >= 20)
    for c in D.sequence_cases():
        if c.k >= 20 and c.off2 == 0:
            assert np.array_equal(c.hits, c.design.dots()), c.name
    assert D.doubled_33kb_case().ref.words()[0] > 65535


def test_served_group_reaches_reverse_complement_runs(oracle):
    """The group of tests/test_gpu_dot_designs.py that a shared join serves, read off the reference: against the inversion allele
    one case has a reverse-complement run of 12 dots inside the one longest sub-list (its median is taken over the run), others
    have such runs outside it, and the derived alleles' dot plots are not the window's."""
    import test_gpu_dot_designs as G
    _win, _reads, _derived, cases = G.served_group()
    by = {c.name: c for _r, _a, c in cases}

    def look(c):
        kept = [x for x, k in zip(c.hits.tolist(), c.ref.k1) if k]
        cc, n_lists, lists = D.r4_lists(kept)
        return cc, n_lists, D.anti_runs(kept, set(lists[0]) if n_lists == 1 else set())

    cc, n_lists, (inside, _out) = look(by["rc_run_in_winner/inversion@k20"])
    assert (cc, n_lists, inside) == (12, 1, 12)
    assert look(by["rc_run_in_winner/window@k20"])[2] == (0, 0)          # (the window has no such run: the read is forward there)
    cc, n_lists, (inside, outside) = look(by["x0_inside_even+(1000,1000)/inversion@k20"])
    assert n_lists == 1 and inside >= 2 and outside == 40
    assert sum(1 for n, c in by.items() if "/inversion" in n and look(c)[2][1] >= 11) >= 5
    names = sorted({n.split("/")[0] for n in by})
    assert len(names) == 7
    for n in names:
        w, inv, dup = (by["%s/%s@k20" % (n, t)] for t in ("window", "inversion", "duplication"))
        assert not np.array_equal(inv.hits, w.hits) and not np.array_equal(dup.hits, w.hits), n
        assert len(dup.hits) > len(w.hits), n                             # (segments inside the doubled stretch appear twice)
        assert inv.ref.words() != w.ref.words() and dup.ref.words() != w.ref.words(), n


# ---- the narrow list bodies of tests/test_gpu_dot_designs.py on the CPU twin ----
@pytest.fixture(scope="module")
def eng(oracle):
    from vapor_amd import _lib
    from vapor_amd.engine import Engine
    saved = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(oracle.build_twin()))
    e = Engine(0)
    yield e
    e.close()
    _lib._lib = saved


def test_list_bodies_on_the_twin(eng):
    import test_gpu_dot_designs as G
    assert not eng.wide_available()                      # (the twin has no wide route: those bodies run on the GPU only)
    for band in (0, 1, 2):
        G.check_small_lists(eng, band)
    G.check_big_lists(eng)
