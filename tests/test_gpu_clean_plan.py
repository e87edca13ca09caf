"""The clean launch at the two places where vapor_clean_plan.h decides something the other GPU tests do not reach:

(1) Tiny served pairs after the fit.  A share group of one 80-base window and a deletion, a tandem duplication and an inversion
    derived from it, a handful of 60-base reads at k = 10: no pair holds more than 27 records, so after the first blocking run the
    clean kernel's LDS copy is sized for 28 records and its layout asks for some 420 bytes - less than the 640 bytes
    remap_for_target uses of the same allocation when the clean workgroups cut the served pairs' records themselves
    (remap_in_clean 2).  The launch then asks for the scratch floor.  Statistics, dots and flags of the run sized by the estimate,
    of the run sized by the measurement and the records of an asynchronous step are equal between remap_kernel (0) and the clean
    workgroups (2), and the oracle's.
(2) The compiled widths on the plan route.  clean_kernel<4> serves value ranges of up to 1024 words, <8> up to 2048,
    <CLEAN_PER_MAX> beyond: pairs whose len1 + len2 + 2 is 32 768, 32 769, 65 536 and 65 537 bases sit on both sides of both
    edges (tests/test_gpu_dot_designs.py reaches the three widths through the list route, and the plan route at 2 000 - 4 000
    and 98 000 bases, never at an edge).  A 300-base read against a random window with the read's end planted at the window's start
    and at its end, so that the largest values of both axes fall into the last bitmap words, and two more pieces of the read in
    between, one of them reverse-complemented."""
import numpy as np
import pytest

import dot_designs as D
import test_gpu_dot_designs as G
from vapor_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def tiny_group():
    def make():
        rng = np.random.default_rng(6406)
        win = D._rand_dna(rng, 80)
        mid = win[30:50]
        derived = [([(0, 0, 30, False), (0, 50, 30, False)], False),                                        # deletion
                   ([(0, 0, 30, False), (0, 30, 20, False), (0, 30, 20, False), (0, 50, 30, False)], False),  # tandem duplication
                   ([(0, 0, 30, False), (0, 30, 20, True), (0, 50, 30, False)], False)]                      # inversion
        texts = [win, win[:30] + win[50:], win[:30] + mid + mid + win[50:], win[:30] + D.revcomp(mid) + win[50:]]
        reads = [win[8:68], texts[1], texts[2][20:80], texts[3][10:70], win[:29] + D._other(rng, win[29]) + win[30:60]]
        cases = []
        for r, rd in enumerate(reads):
            for a, tag in enumerate(("window", "deletion", "duplication", "inversion")):
                cases.append((r, a, D.SeqCase("tiny_read%d/%s@k10" % (r, tag), 10, rd, texts[a], (0, 3)[r % 2])))
        return win, reads, derived, cases
    return D._once("tiny_served", make)


def _same(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def run_tiny_group(eng, route):
    win, reads, derived, cases = tiny_group()
    seqs = [win] + reads
    first_der = len(seqs)
    rows = [(1 + r, 0 if a == 0 else first_der + a - 1, c.off2, c.k, L.PF_C1 | L.PF_C2 | L.PF_DIR) for r, a, c in cases]
    # the finish kernel's view: read r is scored by its pair against the window and its pair against the deletion allele
    table = np.zeros(len(reads), dtype=L.READ_DTYPE)
    table["ref_a"] = table["ref_b"] = 4 * np.arange(len(reads))
    table["alt_a"] = table["alt_b"] = 4 * np.arange(len(reads)) + 1
    table["len_ref"], table["len_alt"] = 80, 60
    eng.set_param("remap_in_clean", route)
    try:
        ss = eng.seqset(seqs, derived=derived)
        try:
            plan = eng.plan(ss, eng.make_pairs(rows))
            try:
                estimated = plan.run().copy()               # the LDS copy sized by the plan's estimate (at least 1024 records)
                measured = plan.run().copy()                # ... and by the largest record count the first run saw
                hits, hf, off = plan.fetch_hits(range(plan.n), want_flags=True)
                rec = plan.record_counts().copy()
                tm = plan.timings()
                plan.set_reads(table, 1)
                blocking = plan.run_loci().copy()
                plan.run_loci_async()
                step = plan.sync().copy()
            finally:
                plan.close()
        finally:
            ss.close()
    finally:
        eng.set_param("remap_in_clean", 1)
    return rows, estimated, measured, hits, hf, off, rec, tm, blocking, step


def test_tiny_served_pairs_after_the_fit(eng):
    _win, _reads, _derived, cases = tiny_group()
    got = {route: run_tiny_group(eng, route) for route in (0, 2)}
    errs = []
    for route, (rows, estimated, measured, hits, hf, off, rec, tm, blocking, step) in got.items():
        # the test says something only if the group is shared, route 2 serves in the clean workgroups and the pairs are tiny
        assert tm["shared_joins"] > 0 and tm["pairs_served_by_shared_joins"] >= 2 * tm["shared_joins"], tm
        assert tm["remap_in_clean"] == (1 if route == 2 else 0), tm
        # (a read across the inverted stretch brings its 11 reverse-complement dots as records of one dot each, twice against the
        # duplication: 27 records at the most.  At this value range, 6 words, a staged copy of up to 48 records asks for less than
        # the 640 bytes of scratch: 4 * 42 + 64 + 8 + 8 * 48 = 624)
        assert 0 < int(rec.max()) <= 32 and (60 + 100 + 2 + 31) // 32 == 6, rec
        assert tm["clean_workgroups_per_cu"] == 8, tm
        assert np.array_equal(estimated, measured), (route, np.argwhere(estimated != measured)[:5])
        assert not measured[:, 14].any() and not measured[:, 15].any(), (route, measured[:, 14:])
        assert _same(blocking, step), (route, blocking, step)
        for t, (_r, _a, c) in enumerate(cases):
            want, want_flags = c.ref.expected(rows[t][4])
            h, f = hits[off[t]:off[t + 1]], hf[off[t]:off[t + 1]]
            o = np.lexsort((f, h[:, 1], h[:, 0]))
            eo = np.lexsort((want_flags, c.hits[:, 1], c.hits[:, 0]))
            if not np.array_equal(h[o], c.hits[eo]):
                errs.append("%s, route %d: the dots differ from dotdata's (%d, expected %d)" % (c.name, route, len(h), len(c.hits)))
                continue
            G._diff(errs, c.name, "tiny(%d)" % route, rows[t][4], measured[t], want, f[o], want_flags[eo])
    G._report(errs)
    a, b = got[0], got[2]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[6], b[6]) and _same(a[8], b[8]) and _same(a[9], b[9])
    assert sum(len(c.hits) for _r, _a, c in cases) > 300          # (the reads do match their alleles)


def edge_case(total):
    def make():
        rng = np.random.default_rng(total)
        read = D._rand_dna(rng, 300)
        n = total - 2 - len(read)
        win = D._rand_dna(rng, n)
        a, b, m, s = read[:140], read[200:], D.revcomp(read[50:200]), read[240:]
        win = s + win[len(s):n // 4] + a + win[n // 4 + len(a):n // 2] + m + win[n // 2 + len(m):n - len(b)] + b
        assert len(win) == n and len(read) + len(win) + 2 == total
        return D.SeqCase("edge_%d@k20" % total, 20, read, win)
    return D._once("edge_%d" % total, make)


@pytest.mark.parametrize("total,rw,width", [(32768, 1024, 4), (32769, 1025, 8), (65536, 2048, 8), (65537, 2049, 16)])
def test_width_edges_on_the_plan_route(eng, total, rw, width):
    c = edge_case(total)
    assert (len(c.read) + len(c.allele) + 2 + 31) // 32 == rw
    per = -(-rw // 256)                                            # clean_plan::width at 256 threads
    assert (4 if per <= 4 else 8 if per <= 8 else 16) == width
    st, _rec = G.check_plan(eng, [c], "plan_rw%d" % rw)
    assert 300 < int(st[0, 0]) < 2000                              # the planted pieces, and hardly a chance dot
    # both axes reach the bitmap's last words: i + j at the window's end, i - j + len2 at its start
    h = c.hits
    assert (int((h[:, 1] + h[:, 0]).max()) >> 5) >= rw - 4 and (int((h[:, 1] - h[:, 0]).max()) + len(c.allele) >> 5) >= rw - 4
