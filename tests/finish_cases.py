"""Designed inputs for the finishing step (finish_kernel, its CPU twin and the host statements in vapor_amd/finish.py).

A plain helper module (no pytest hooks).  vapor_plan_set_reads takes len_ref / len_alt and the genotype table from the caller
and checks neither against the sequences, so one small plan is enough: its integer statistics are read once, and the read
tables below place every ratio on, just below and just above its threshold by choosing the lengths, and show which (n, nnonpos)
cell was read by choosing the table.  It holds
  * pool(): one plan's worth of small pairs - the sequence cases of tests/dot_designs.py, pairs spelled from the small designs
    below, and two pairs that fail when the plan is made;
  * check_pool(): what the pool has to contain, asserted on the statistics a plan returned;
  * gate_tables(): per scorer kind, reads over ordered (ref, alt) choices whose lengths sit at the gates;
  * locus_table(): loci of every size and positive count at which the reduction changes its path, drawn from the gate tables'
    reads;
  * gt_tables(): the project's genotype table and two designed ones;
  * expected(): per-read scores and locus records of a table from tests/finish_model.py.
Everything is built once per process and never changed."""
import numpy as np

import dot_designs as D
import finish_model as M
from vapor_amd import _lib as L

BIG = 60000                    # a length at which every gate fails (n_hits and spans of the pool stay below 6 000)
FLAGS = 7                      # C1 | C2 | DIR: every word of the record is filled
LOCUS_SIZES = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513)
POSITIVE_COUNTS = (0, 1, 7, 8, 9, 16, 17, 64, 127, 128)

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------
# the pair pool
# ---------------------------------------------------------------------------------------------------------------------
def _designs():
    Ds = D.Design
    return [
        # one diagonal each: n_hits = n, last_j - first_j = n - 1; dense (n_hits > span / 6), so both span gates can sit at
        # their thresholds while the hit gate passes
        Ds("fin_span39", "span 39 = 3 * 13: 0.6 is met exactly at length 65", [(0, 200, 40)]),
        Ds("fin_span49", "span 49 = 7 * 7: 0.7 is met exactly at length 70", [(0, 300, 50)]),
        Ds("fin_span21", "span 21 = 3 * 7: 0.6 at length 35, 0.7 at length 30", [(0, 250, 22)]),
        # mean |j - i| of 250, 249, 200 and 199: S1 scores 1 - 249/250 = 0.004 (positive, rounds to 0.0) and 1 - 199/200 (rounds to 0.01)
        Ds("fin_abs250", "mean |j - i| = 250", [(250, 200, 40)]),
        Ds("fin_abs249", "mean |j - i| = 249", [(249, 200, 40)]),
        Ds("fin_abs200", "mean |j - i| = 200", [(200, 200, 40)]),
        Ds("fin_abs199", "mean |j - i| = 199", [(199, 200, 40)]),
        # c = -300 (the 40-dot diagonal wins alone); the two 11-dot diagonals 20 either side of it are far (|x - y| = 20 at
        # |x| < 200) with x - y = -20 and +20: DIR_N = 22, DIR_SUM2 = 0
        Ds("fin_dir_sum0", "far dots whose x - y cancel", [(-300, 600, 40), (-280, 310, 11), (-320, 440, 11)]),
        Ds("fin_dots3", "three loose dots: n_hits = 3, C1 keeps nothing", noise=[(300, 100), (700, 500), (1100, 900)]),
        Ds("fin_dots2", "two loose dots", noise=[(300, 100), (700, 500)]),
        Ds("fin_dots1", "one loose dot", noise=[(300, 100)]),
    ]


class Pool:
    """seqs, rows (seq1, seq2, off2, k, flags) and names of the pairs; the last two pairs fail at plan creation."""

    def __init__(self):
        self.seqs, self.rows, self.names = [], [], []
        for c in D.sequence_cases():
            self._add(c.name, c.read, c.allele, c.off2, c.k)
        rng = np.random.default_rng(5150)
        for q, d in enumerate(_designs()):
            k = (30, 40)[q % 2]
            rd, al = D.build_pair(rng, k, d)
            self._add("%s@k%d" % (d.name, k), rd, al, 0, k)
        self._add("fin_dots0@k40", D._rand_dna(rng, 2100), D._rand_dna(rng, 2300), 0, 40)
        # the sequences of fin_span39 once more under other pair flags: a cleaner the pair does not ask for keeps nothing (C2 on
        # its own always keeps its largest group), so these are the dense pairs with C2_KEPT == 0 and with C1_KEPT == 0
        s1, s2 = self.rows[self.names.index("fin_span39@k30")][:2]
        for name, flags in (("fin_span39_no_c2@k30", L.PF_C1 | L.PF_DIR), ("fin_span39_no_c1@k30", L.PF_C2)):
            self.rows.append((s1, s2, 0, 30, flags))
            self.names.append(name)
        self.n_ok = len(self.rows)
        self.rows.append((0, 1, 0, 11, FLAGS))                            # k = 11: VAPOR_E_ARG
        self.rows.append((0, len(self.seqs) + 5, 0, 20, FLAGS))           # seq2 outside the set: VAPOR_E_ARG
        self.names += ["failed_k11", "failed_seq2"]
        self.failed = (self.n_ok, self.n_ok + 1)
        self.by_name = {n: t for t, n in enumerate(self.names)}
        assert len(self.by_name) == len(self.names) and len(self.rows) < 100

    def _add(self, name, read, allele, off2, k):
        self.seqs += [read, allele]
        self.rows.append((len(self.seqs) - 2, len(self.seqs) - 1, off2, k, FLAGS))
        self.names.append(name)


def pool():
    return _once("pool", Pool)


def _span(s):
    return int(s[L.ST_LAST_J] - s[L.ST_FIRST_J])


def check_pool(st):
    """What the read tables rely on, from the statistics a plan of the pool returned."""
    P = pool()
    st = np.asarray(st)
    assert st.shape == (len(P.rows), L.STATS_STRIDE)
    ok = st[:P.n_ok]
    assert not ok[:, L.ST_STATUS].any()
    for f in P.failed:
        assert st[f, L.ST_STATUS] == L.E_ARG
        # (a failed pair's record holds nothing a scorer could use: finish_kernel relies on that, it does not look at word 15)
        assert st[f, 0] == 0 and not st[f, 3:15].any()
    n, k1, k2 = ok[:, L.ST_N_HITS], ok[:, L.ST_C1_KEPT], ok[:, L.ST_C2_KEPT]
    dn, ds = ok[:, L.ST_DIR_N], ok[:, L.ST_DIR_SUM2]
    span = ok[:, L.ST_LAST_J] - ok[:, L.ST_FIRST_J]
    for v in (0, 1, 2, 3):
        assert (n == v).any(), "no pair with n_hits == %d" % v
    assert (n > 3).any()
    assert ((k1 == 0) & (n > 2)).any(), "C1_KEPT == 0 with n_hits > 2"
    assert ((k2 == 0) & (n > 0)).any(), "C2_KEPT == 0 with n_hits > 0"
    assert ((dn == 0) & (k1 > 0)).any(), "DIR_N == 0 with C1_KEPT > 0"
    assert ((ds == 0) & (dn > 0)).any(), "DIR_SUM2 == 0 with DIR_N > 0"
    assert (ds < 0).any(), "DIR_SUM2 < 0"
    assert ((span % 3 == 0) & (n > 2)).any() and ((span % 7 == 0) & (n > 2) & (span % 3 != 0)).any(), "spans divisible by 3 and by 7"
    for name, want in (("fin_abs250@k40", 250), ("fin_abs249@k30", 249), ("fin_abs200@k40", 200), ("fin_abs199@k30", 199)):
        s = st[P.by_name[name]]
        assert s[L.ST_C1_KEPT] == 40 and s[L.ST_C1_SUM_ABS] == 40 * want, (name, s[:7].tolist())
    assert int(n.max()) < BIG // 10 and int(span.max()) < BIG // 2


# ---------------------------------------------------------------------------------------------------------------------
# read tables
# ---------------------------------------------------------------------------------------------------------------------
def _table(rows, locus):
    """rows: (ref_a, alt_a, ref_b, alt_b, kind, len_ref, len_alt); locus: the locus of each row (not decreasing)."""
    t = np.zeros(len(rows), dtype=L.READ_DTYPE)
    if len(rows):
        a = np.asarray(rows, dtype=np.int64)
        for q, f in enumerate(("ref_a", "alt_a", "ref_b", "alt_b", "kind")):
            t[f] = a[:, q]
        t["len_ref"], t["len_alt"] = a[:, 5], a[:, 6]
        t["locus"] = locus
        assert (a[:, 5:] >= 1).all() and (np.diff(t["locus"]) >= 0).all()
    return t


def _lens(s):
    """The lengths at which the gates of record `s` sit: hit ratio 0.1 at 10 N (N / (10 N) > 0.1 is false, 10 N - 1 passes,
    10 N + 1 fails), span S over 0.6 at 5 S / 3 and over 0.7 at 10 S / 7 - met exactly when S is divisible by 3 / by 7, else the
    integer below and its two neighbours - and `ok`, the largest length at which every gate of the record passes."""
    n, sp = int(s[L.ST_N_HITS]), _span(s)
    hit = [v for v in (10 * n - 1, 10 * n, 10 * n + 1) if v >= 1]
    s6 = [v for v in ((5 * sp) // 3 - 1, (5 * sp) // 3, (5 * sp) // 3 + 1) if v >= 1]
    s7 = [v for v in ((10 * sp) // 7 - 1, (10 * sp) // 7, (10 * sp) // 7 + 1) if v >= 1]
    ok = max(1, min(10 * n - 1, (10 * sp) // 7 - 1))
    return hit, s6, s7, ok


def _subset(st):
    """The pairs every ordered (ref, alt) choice is made from: one per property check_pool asks for, by name or by the first
    pair that has the property."""
    P = pool()
    ok = st[:P.n_ok]
    n, k1, k2 = ok[:, L.ST_N_HITS], ok[:, L.ST_C1_KEPT], ok[:, L.ST_C2_KEPT]
    span = ok[:, L.ST_LAST_J] - ok[:, L.ST_FIRST_J]
    first = lambda m: int(np.flatnonzero(m)[0])
    named = ["fin_span39@k30", "fin_span49@k40", "fin_span21@k30", "fin_abs250@k40", "fin_abs249@k30", "fin_abs200@k40", "fin_abs199@k30",
             "fin_dir_sum0@k40", "fin_dots3@k30", "fin_span39_no_c2@k30", "fin_span39_no_c1@k30"]
    sub = [P.by_name[x] for x in named]
    sub.append(first((ok[:, L.ST_DIR_N] == 0) & (k1 > 0)))
    sparse = first((ok[:, L.ST_DIR_SUM2] < 0) & (span > 7 * n))           # sparse: the hit gates can sit at 10 N with the spans passing
    sub.append(sparse)
    sub.append(first((ok[:, L.ST_DIR_SUM2] > 0) & (span > 7 * n)))
    sub.append(first((k2 > 0) & (ok[:, L.ST_C2_COUNT10] > 0) & (span > 7 * n) & (ok[:, L.ST_C2_COUNT10] != k2)))
    few = [P.by_name[x] for x in ("fin_dots0@k40", "fin_dots1@k30", "fin_dots2@k40")]
    out = []
    for p in sub:
        if p not in out:
            out.append(p)
    return out, few, sub[0], sparse                                       # (sub[0]: dense, its span gates can sit at their thresholds)


def _gate_rows(st, kind):
    P = pool()
    sub, few, dense, sparse = _subset(st)
    rows = []

    def add(r, a, lr, la, rb=None, ab=None):
        if lr >= 1 and la >= 1:
            rows.append((r, a, r if rb is None else rb, a if ab is None else ab, kind, lr, la))

    # every ordered choice, ref == alt included: at lengths where every gate of both records passes, and with one side failing
    for r in sub:
        for a in sub:
            okr, oka = _lens(st[r])[3], _lens(st[a])[3]
            for lr, la in ((okr, oka), (okr, BIG) if (r + a) % 2 else (BIG, oka)):
                add(r, a, lr, la)
                if kind == 0 and r != a:
                    add(r, a, lr, la, a, r)                               # (S2 on the swapped choice: either score can be the smaller)
    # the gates of every pair of the subset beside itself, a dense and a sparse partner, and of the pairs with 0, 1 and 2 dots
    # beside the dense one
    pairs = []
    for p in sub:
        for q in (p, dense, sparse):
            pairs += [(p, q), (q, p)]
    for p in few:
        pairs += [(p, dense), (dense, p)]
    for r, a in dict.fromkeys(pairs):
        hr, r6, r7, okr = _lens(st[r])
        ha, a6, a7, oka = _lens(st[a])
        if kind == 1:
            for lr in hr + r6:
                for la in (lr - 1, lr, lr + 1, oka, BIG):                # (min(len_ref, len_alt) with len_ref <, == and > len_alt)
                    add(r, a, lr, la)
            for la in a6 + ha:
                for lr in (1, okr, BIG):
                    add(r, a, lr, la)
        elif kind == 2:
            for lr in hr + [1, BIG]:                                      # (max: each side alone over the threshold)
                for la in ha + [1, BIG]:
                    add(r, a, lr, la)
        elif kind == 3:
            for lr in hr + r7:
                for la in (1, oka, BIG):
                    add(r, a, lr, la)
            for la in ha + a7:
                for lr in (1, okr, BIG):
                    add(r, a, lr, la)
        else:
            for rb, ab in ((r, a), (a, r)):
                for lr in hr + r6:
                    for la in (oka, lr):
                        add(r, a, lr, la, rb, ab)
    # a failed pair in each position, one at a time, beside choices that score without it
    good = [(dense, sub[1]), (sub[3], sub[4]), (sparse, sparse)]
    for f in P.failed:
        for r, a in good:
            okr, oka = _lens(st[r])[3], _lens(st[a])[3]
            for lr, la in ((1, 1), (okr, oka)):
                add(r, a, lr, la)
                add(f, a, lr, la)
                add(r, f, lr, la)
                add(r, a, lr, la, f, a)
                add(r, a, lr, la, r, f)
                add(f, a, lr, la, f, a)
                if kind == 0:                                             # (S1's pair failed, S2's did not: S2's score stands)
                    add(f, a, lr, la, r, a)
                    add(r, f, lr, la, r, a)
    return rows


def gate_tables(st):
    """{kind: READ_DTYPE table}, loci of 23 reads (below the genotype table's bound, so every locus reads a cell)."""
    def make():
        check_pool(st)
        out = {}
        for kind in (0, 1, 2, 3):
            rows = _gate_rows(st, kind)
            out[kind] = _table(rows, np.arange(len(rows)) // 23)
            assert 500 < len(rows) < 6000, (kind, len(rows))
        check_gate_tables(st, out)
        return out
    return _once("gates", make)


def count_loci(t):
    return int(t["locus"].max()) + 1 if len(t) else 0


def check_gate_tables(st, tabs):
    """The outcomes the gate tables have to reach, from the model's scorers on the statistics."""
    seen = set()
    for kind, t in tabs.items():
        for rd in t.tolist():
            ra, aa, rb, ab, k, _loc, lr, la = rd
            if k in (0, 1):
                x = M.s1(st[ra], st[aa], lr, la)
                seen.add(("s1", "r_only" if x == [1.1, 2.1] else "a_only" if x == [2.1, 1.1] else "none" if x == [0, 0] else "both"))
                seen.add(("s1_len", "lt" if lr < la else "gt" if lr > la else "eq"))
            if k == 2:
                x = [float(int(st[ra][0])) / lr > 0.1, float(int(st[aa][0])) / la > 0.1]
                seen.add(("s2_max", tuple(x)))
            if k == 0:
                v1, v2 = M._RIGHT._one(M.s1, st[ra], st[aa], lr, la), M._RIGHT._one(M.s2, st[rb], st[ab], lr, la)
                if v1 is not None and v2 is not None:
                    seen.add(("del", "s1_smaller" if v1 < v2 else "s2_smaller" if v2 < v1 else "equal"))
                elif v1 is not None or v2 is not None:
                    seen.add(("del", "s1_only" if v1 is not None else "s2_only"))
                else:
                    seen.add(("del", "neither"))
    want = {("s1", x) for x in ("both", "r_only", "a_only", "none")} | {("s1_len", x) for x in ("lt", "gt", "eq")}
    want |= {("s2_max", x) for x in ((True, False), (False, True), (True, True), (False, False))}
    want |= {("del", x) for x in ("s1_smaller", "s2_smaller", "equal", "s1_only", "s2_only", "neither")}
    assert want <= seen, sorted(want - seen)
    # a failed pair in every position: the scorer that reads it scores nothing, a deletion's other scorer still does
    n_ok = pool().n_ok
    for kind, t in tabs.items():
        s = expected(st, t)[0]
        fa, fb = (t["ref_a"] >= n_ok) | (t["alt_a"] >= n_ok), (t["ref_b"] >= n_ok) | (t["alt_b"] >= n_ok)
        for f in ("ref_a", "alt_a", "ref_b", "alt_b"):
            assert (t[f] >= n_ok).any(), (kind, f)
        if kind == 0:
            assert np.isnan(s[fa & fb]).all() and (~np.isnan(s[fa & ~fb])).any() and (~np.isnan(s[~fa & fb])).any()
        else:
            assert np.isnan(s[fa]).all() and (~np.isnan(s[~fa & fb])).any()
    sc = np.concatenate([expected(st, t)[0] for t in tabs.values()])
    assert ((sc > 0) & (sc < 0.005)).any() and ((sc >= 0.005) & (sc < 0.015)).any()
    assert (sc == 0.0).any() and (sc < 0).any() and np.isnan(sc).any()


def _read_pools(st):
    """Reads of the gate tables by what they score: distinct positives (rounding above 0), positives below 0.005, scores that
    are not positive, skipped reads.  Each entry the seven fields of a read."""
    tabs = gate_tables(st)
    pos, tiny, nonpos, skip, seen = [], [], [], [], set()
    for kind in (1, 3, 0, 2):
        t = tabs[kind]
        sc = expected(st, t)[0]
        for rd, s in zip(t.tolist(), sc.tolist()):
            row = tuple(rd[:5]) + tuple(rd[6:])
            if s != s:
                if len(skip) < 64:
                    skip.append(row)
            elif s not in seen:
                seen.add(s)
                (tiny if 0 < s < 0.005 else pos if s > 0 else nonpos).append(row)
    assert len(pos) >= 24 and tiny and len(nonpos) >= 8 and len(skip) >= 8, (len(pos), len(tiny), len(nonpos), len(skip))
    return pos, tiny, nonpos, skip


# (reads, positives, skipped) of every locus of the locus table, in table order; a locus of two or more positives has one
# of them below 0.005, so that nnonpos is not n - npos
LOCI = [(0, 0, 0),
        (1, 1, 0), (1, 0, 0), (1, 0, 1),
        (7, 7, 0), (7, 1, 3), (8, 8, 0), (8, 7, 1), (9, 9, 0), (9, 8, 1),
        (15, 9, 3), (16, 16, 0), (17, 17, 0), (17, 16, 1),
        (20, 3, 0), (40, 6, 0), (60, 9, 0), (13, 2, 0), (26, 3, 6),       # GS = 3/20, 6/40, 9/60 (not above .15), 2/13 (above)
        (0, 0, 0),
        (63, 16, 0), (64, 64, 0), (64, 17, 0), (65, 64, 1), (65, 9, 0), (70, 8, 6),        # 63, 64, 64, 64, 65, 64 scored reads
        (5, 0, 5),                                                        # every read skipped
        (127, 127, 0), (127, 64, 40), (128, 128, 0), (128, 127, 1), (129, 128, 1), (129, 129, 0),
        (255, 128, 100), (256, 128, 64), (256, 200, 20), (256, 39, 0),    # 200 positives inside one chunk; GS = 39/256
        (257, 127, 100), (257, 257, 0), (300, 128, 150), (300, 64, 0), (513, 128, 300), (513, 400, 50),
        (0, 0, 0)]


def locus_table(st):
    """(READ_DTYPE table, n_loci).  The roles of a locus's reads - positive, not positive, skipped - are dealt by a seeded
    permutation, so the rank of a positive among the positives differs from its lane and from its slot in the chunk."""
    def make():
        pos, tiny, nonpos, skip = _read_pools(st)
        rng = np.random.default_rng(5151)
        rows, locus = [], []
        cur = [0, 0, 0, 0]

        def take(poolq, q):
            cur[q] += 1
            return poolq[(cur[q] * 7) % len(poolq)]
        for li, (n, npos, nskip) in enumerate(LOCI):
            role = np.zeros(n, dtype=np.int64)                            # 0 not positive, 1 positive, 2 skipped, 3 positive below 0.005
            where = rng.permutation(n)
            role[where[:npos]] = 1
            if npos >= 2:
                role[where[0]] = 3
            role[where[npos:npos + nskip]] = 2
            if n in (300, 513) and npos:                                  # positives on both sides of the 256-read chunk boundary
                assert (role[:256] % 2 == 1).any() and (role[256:] % 2 == 1).any()
            for r in role.tolist():
                rows.append(take((nonpos, pos, skip, tiny)[r], r))
                locus.append(li)
        t = _table(rows, np.asarray(locus, dtype=np.int64))
        check_locus_table(st, t)
        return t, len(LOCI)
    return _once("loci", make)


def check_locus_table(st, t):
    sc = expected(st, t, n_loci=len(LOCI))[0]
    sizes, counts, differ, of = set(), set(), 0, 0
    for li, (n, npos, nskip) in enumerate(LOCI):
        s = sc[t["locus"] == li]
        assert len(s) == n and int((s > 0).sum()) == npos and int(np.isnan(s).sum()) == nskip, (li, n, npos, nskip)
        sizes.add(n)
        counts.add(npos)
        p = [x for x in s.tolist() if x > 0]
        if npos >= 8:
            of += 1
            ltr = 0.0
            for x in p:
                ltr += x
            differ += (ltr / npos) != M.qs_numpy(p)
    assert sizes >= set(LOCUS_SIZES) and counts >= set(POSITIVE_COUNTS)
    assert 2 * differ >= of, (differ, of)                                 # (otherwise a wrong order of summation could not show)
    assert LOCI[0] == LOCI[-1] == (0, 0, 0) and (0, 0, 0) in LOCI[1:-1] and (5, 0, 5) in LOCI
    # GS exactly on 3/20 three ways (and once beside skipped reads), 2/13 and 39/256 above .15
    for spec, above in (((20, 3, 0), False), ((40, 6, 0), False), ((60, 9, 0), False), ((26, 3, 6), False), ((13, 2, 0), True), ((256, 39, 0), True)):
        n, npos, nskip = spec
        assert spec in LOCI and (float(npos) / float(n - nskip) > .15) == above


def gt_tables():
    """{name: (65, 65, 2) float64}: the project's table; "cell", whose GQ names the cell that was read; "zero", all 0/0, where
    the GS > .15 rule alone decides the genotype."""
    def make():
        from vapor_amd import finish
        n = L.GT_TABLE_N
        k, l = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        cell = np.zeros((n, n, 2), dtype=np.float64)
        cell[:, :, 0] = (k + 2 * l) % 3
        cell[:, :, 1] = 100 * k + l + 0.25
        zero = np.zeros((n, n, 2), dtype=np.float64)
        zero[:, :, 1] = 1.0
        return {"project": np.ascontiguousarray(finish.gt_table()), "cell": cell, "zero": zero}
    return _once("gt", make)


# ---------------------------------------------------------------------------------------------------------------------
# the model over a table
# ---------------------------------------------------------------------------------------------------------------------
def model_scores(st, t, model=M._RIGHT):
    """The model's score of every read of table `t` (None = skipped) on the statistics `st`, as a list."""
    recs = [r.tolist() for r in np.asarray(st)]
    return [model.score(k, recs[ra], recs[aa], recs[rb], recs[ab], lr, la) for ra, aa, rb, ab, k, _loc, lr, la in t.tolist()]


def model_loci(scores, t, nl, gt, order, model=M._RIGHT):
    per = [[] for _ in range(nl)]
    for s, li in zip(scores, t["locus"].tolist()):
        per[li].append(s)
    table = gt.tolist()
    return np.array([model.locus(p, table, order) for p in per], dtype=np.float64).reshape(nl, L.LOCUS_STRIDE)


def expected(st, t, n_loci=None, gt="project", order="kernel"):
    """(scores with NaN for a skipped read, (n_loci, 8) locus records) of table `t` from the model."""
    nl = count_loci(t) if n_loci is None else n_loci
    key = ("exp", t.tobytes(), nl, np.asarray(st).tobytes())
    scores = _once(key, lambda: model_scores(st, t))
    sc = np.array([np.nan if s is None else s for s in scores], dtype=np.float64)
    loci = _once(key + (gt, order), lambda: model_loci(scores, t, nl, gt_tables()[gt], order))
    return sc, loci


def qs_bound(loci_row):
    """|QS in one order - QS in another| for m positive doubles: each order is within (m - 1) 2^-53 relative of the true sum,
    and the division by m adds one rounding on each side."""
    return 2.0 * loci_row[5] * 2.0 ** -53 * loci_row[0]
