"""Designed dot plots for everything behind the join: the two cleaners, the counts and the directed statistics (R4:
dis_to_diagnal_most_abundant_defined, SF:582-591, plus eu_dis_dir_calcu, SF:718-722).

A plain helper module (no pytest hooks).  It holds
  * Design: a dot plot written down as segments, with the transforms that keep its ties and edges (scale, shift) and the one
    that widens it for the wide route (stretch);
  * NAMED: designs that each reach one rule - the comment beside each says which - and random_designs();
  * expected(): words 0-13 of the statistics record and the per-dot flag bytes, from the float64 statements of the reference's
    own operations in oracle/oracle.py (no integer shortcut on this side);
  * MUTANTS: deliberately wrong variants of expected(), used only to show that the designs can tell them from the right one;
  * build_pair(): a (read, allele) pair of sequences whose dot plot is the design.

Coordinates are the project's (j, i): j the position in the allele (seq2), i in the read (seq1)."""
import numpy as np

from oracle import oracle

MAX_SEQ = 65535
MAX_WIDE = 1048575
FLAG_SETS = (1, 2, 3, 5, 7)          # clean_body has separate code for C1 only, C2 only and both; 5 and 7 add R4


# ---------------------------------------------------------------------------------------------------------------------
# designs
# ---------------------------------------------------------------------------------------------------------------------
class Design:
    """fwd: (d, j0, n) -> dots (j0 + t, j0 + d + t); anti: (j0, i0, n) -> dots (j0 + t, i0 - t); noise: loose (j, i) dots;
    dup: indices of forward segments whose dots are listed twice."""

    def __init__(self, name, rule, fwd=(), anti=(), noise=(), dup=(), lists_only=False, wide_only=False):
        self.name, self.rule = name, rule
        self.fwd, self.anti, self.noise, self.dup = [tuple(s) for s in fwd], [tuple(s) for s in anti], [tuple(s) for s in noise], tuple(dup)
        self.lists_only = lists_only or bool(dup)        # (cannot be spelled as a pair of sequences)
        self.wide_only = wide_only

    def _new(self, tag, fwd, anti, noise):
        return Design(self.name + tag, self.rule, fwd, anti, noise, self.dup, self.lists_only, self.wide_only)

    def dots(self):
        rows = []
        for q, (d, j0, n) in enumerate(self.fwd):
            t = np.arange(n, dtype=np.int64)
            seg = np.stack([j0 + t, j0 + d + t], axis=1)
            rows += [seg] * (2 if q in self.dup else 1)
        for j0, i0, n in self.anti:
            t = np.arange(n, dtype=np.int64)
            rows.append(np.stack([j0 + t, i0 - t], axis=1))
        if self.noise:
            rows.append(np.asarray(self.noise, dtype=np.int64).reshape(-1, 2))
        h = np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)
        assert h.size == 0 or h.min() >= 0, (self.name, "negative coordinate")
        h = h[np.lexsort((h[:, 1], h[:, 0]))]             # dotdata's list order
        return np.ascontiguousarray(h, dtype=np.int32)

    def n_dots(self):
        return sum(n * (2 if q in self.dup else 1) for q, (_d, _j, n) in enumerate(self.fwd)) + sum(n for _j, _i, n in self.anti) + len(self.noise)

    def scale(self, s):
        """Every segment s times as long (same start): the multiset of i - j over the segments keeps its proportions, so every
        tie stays a tie, and every dot of the forward segments is still there.  An anti segment grows towards larger i; a noise
        dot moves 40 000 out along its larger coordinate, away from the i + j groups of the grown segments."""
        return self._new("*%d" % s, [(d, j0, n * s) for d, j0, n in self.fwd], [(j0, i0 + n * (s - 1), n * s) for j0, i0, n in self.anti],
                         [(j + 40000, i) if j > i else (j, i + 40000) for j, i in self.noise])

    def shift(self, dj, di):
        """The whole design moved by (dj, di).  dj == di leaves every i - j alone; dj alone leaves i, c - (i - j) and j + c alone,
        i.e. every case of the far rule."""
        return self._new("+(%d,%d)" % (dj, di), [(d + di - dj, j0 + dj, n) for d, j0, n in self.fwd],
                         [(j0 + dj, i0 + di, n) for j0, i0, n in self.anti], [(j + dj, i + di) for j, i in self.noise])

    def stretch(self, f):
        """Every i - j times f (the wide route only): a segment keeps the smaller of its two start coordinates, so the plot
        stays inside 0 .. max |d| * f + its old extent.  The lists of R4 keep their members."""
        def place(j0, i0):
            d = (i0 - j0) * f
            lo = min(j0, i0)
            return (lo - d, lo) if d < 0 else (lo, lo + d)
        fwd = []
        for d, j0, n in self.fwd:
            j1, i1 = place(j0, j0 + d)
            fwd.append((i1 - j1, j1, n))
        anti = []
        for j0, i0, n in self.anti:                       # (i0 - j0 times f at its first dot; i stays at or above its old values)
            d = (i0 - j0) * f
            anti.append((j0, j0 + d, n) if d >= 0 else (i0 - d, i0, n))
        return self._new("x%d" % f, fwd, anti, [place(j, i) for j, i in self.noise])

    def extent(self):
        h = self.dots()
        return int(h[:, 0].max()), int(h[:, 1].max())

    def d_range(self):
        h = self.dots().astype(np.int64)
        d = h[:, 1] - h[:, 0]
        return int(d.min()), int(d.max())


def own_groups(n, one_sided=False):
    """n dots, each a group of its own on both axes: dot t has i + j = 10 t, and i - j = 0, -10, +10, -20, +20, ... - or, one_sided,
    10 t for even t and 10 t - 20 for odd t, which keeps j at 0 or 10 and so max i + max j, which sizes the bitmap, at 10 n.
    |i - j| <= i + j with the same parity, and neighbouring values are exactly 10 apart on either axis: the smallest gap that
    separates groups."""
    t = np.arange(n, dtype=np.int64)
    a = 10 * t
    d = np.where(t % 2 == 1, 10 * t - 20, 10 * t) if one_sided else 10 * ((t + 1) // 2) * np.where(t % 2 == 1, -1, 1)
    return [(int(x), int(y)) for x, y in zip((a - d) // 2, (a + d) // 2)]


# How many dots an LDS-staged list may hold, and what cluster_dual's counters then do (vapor_clean_plan.h, namespace clean_plan):
#   vapor_clean_hits asks geom(rw, LISTS_WANT = 4096) for the staged records, rw = ListPack's ceil((max i + max j + 4) / 32) bitmap
#   words for the batch; geom_for starts from min(4096, CLEAN_HCAP_MAX = 8192) and only shrinks it while the LDS share of a workgroup
#   is too small, so hcap <= 4096, and the share at one to three workgroups per CU holds all 4096 at every rw.  A list of more
#   records goes to clean_big_kernel; 4096 is the most a staged list holds.
#   groups_lds(rw, hcap) = 2 * max((g + 1) / 2, rw * 32 / 100 + 8) with g = min(rw * 32 / 10 + 8, hcap) 16-bit counters;
#   cluster_dual declines a list with groups_D + groups_A + 2 > that and leaves it to two cluster_axis passes.
#   * rw = 1024 (clean_kernel<4>; both layouts fit three workgroups per CU there, so the dual one is used): i + j < 32 768 has
#     room for 3 277 values 10 apart; g = 3 284 counters.  OWN_3270 has 3 270 + 3 270 groups: more than the counters hold.
#   * rw = 2048 / 4096 (clean_kernel<8> / <CLEAN_PER_MAX>, sequential layout): g = 4 096 = hcap.  OWN_4096 fills every record slot
#     and every group counter of the staged copy; one dot more would go to clean_big_kernel.
OWN_3270 = Design("own_3270", "every dot its own group on both axes, as many as i + j < 32 768 holds", noise=own_groups(3270, one_sided=True), lists_only=True)
OWN_4096 = Design("own_4096", "every dot its own group on both axes, as many as a staged list holds", noise=own_groups(4096), lists_only=True)

NOISE = [(900, 40), (40, 900), (1300, 700)]                # loose dots, at least 10 from every group on both axes


def _named():
    D = Design
    out = [
        # one diagonal and nothing else; range1 == 0 at both levels, every value in the 11th list, c = 5
        D("single", "single diagonal", [(5, 200, 40)], noise=NOISE),
        D("single_d0", "single diagonal on i == j (shifted to the corner 65 535 / 65 535 by the list routes)", [(0, 200, 40)]),
        # two segments, one value of i - j: range1 == 0
        D("range1_zero", "range1 == 0", [(5, 200, 20), (5, 300, 25)]),
        # lists 0 and 10 equally long -> two longest sub-lists, c = 0 (not -40, the first list's median)
        D("tie_l1", "level-1 tie (two lists equally long)", [(-40, 200, 30), (60, 300, 30)], noise=NOISE),
        # list 0 = {10 x 20, 90 x 20} wins level 1 alone; inside it 10 -> sub-list 0, 90 -> sub-list 10: a tie, c = 0 (not 10)
        D("tie_l2", "level-2 tie inside a unique level-1 winner", [(10, 200, 20), (90, 300, 20), (1010, 400, 15)]),
        D("tie_3way", "3-way tie", [(-50, 200, 20), (0, 300, 20), (50, 400, 20)]),
        # ten diagonals 10 apart over a range of 90: lists 0..8 and 10 hold one each (list 9 is empty)
        D("tie_10way", "10-way tie", [(10 * t, 200 + 60 * t, 11) for t in range(10)]),
        # the winner holds one value: range2 == 0, all of it in the 11th sub-list, c = 20
        D("range2_zero", "range2 == 0", [(20, 200, 30), (300, 300, 12)]),
        # range 100, edges on integers: 10 is NOT below edge 1 = 10.0 -> list 1 = {10, 19} = 25 beats list 0 = {0} = 20, c = 10
        # (with <= list 0 = {0, 10} = 34 would win and c would be 0)
        D("edge_int_r100", "value exactly on an integer edge, range % 10 == 0", [(0, 200, 20), (10, 300, 14), (19, 400, 11), (100, 500, 11)]),
        # range 97 (prime): only edges 0 and 10 are integers; 12 < 12.7 -> list 0, 13 -> list 1; list 1 = {13, 22} = 32 wins, c = 13
        D("edge_prime_r97", "values beside a fractional edge, prime range", [(3, 200, 11), (12, 300, 15), (13, 400, 20), (22, 500, 12), (100, 600, 11)]),
        # the maximum is alone in the 11th list: as long as list 9 (a tie, c = 0), longer (c = 100), and a case where list 9 plus
        # the maximum would beat list 0 (c = 5, one list) if the maximum were counted into list 9
        D("max_ties_l9", "maximum alone in the 11th list, tying with list 9", [(0, 200, 11), (95, 300, 30), (100, 400, 30)]),
        D("max_beats_l9", "maximum alone in the 11th list, beating list 9", [(0, 200, 11), (95, 300, 20), (100, 400, 30)]),
        D("max_not_in_l9", "maximum alone in the 11th list; list 9 + maximum would beat list 0", [(5, 200, 40), (96, 300, 25), (105, 400, 25)]),
        # sub-list 0 of list 0 = {10 x 20, 13 x 20}: even size, middles 10 and 13 -> c = 11.5, c2x = 23
        D("median_half", "even-sized winner with different middles (odd c2x)", [(10, 200, 20), (13, 300, 20), (45, 400, 11), (400, 500, 11)]),
        D("median_odd", "odd-sized winner", [(10, 200, 20), (13, 300, 21), (45, 400, 11), (400, 500, 11)]),
        # c = -30; the segment on i == j from j = 10 has the dot (30, 30): j + c == 0 strictly inside it (far: y >= 1)
        D("x0_inside_even", "negative c, j + c crosses 0 inside a segment, even c2x (the dot exists)", [(-30, 200, 40), (0, 10, 30)]),
        # c = -30.5 (middles -31 and -30): 2 j - 61 is never 0
        D("x0_inside_odd", "negative c, j + c crosses 0 inside a segment, odd c2x (no such dot)",
          [(-31, 200, 20), (-30, 300, 20), (0, 10, 30), (400, 300, 11)]),
        # c = -30 and the winner starts at (30, 0): x == 0 and y == 0 -> |0 - 0| / (0 + 1) = 0, not far
        D("x0_y0", "a dot with j + c == 0 and i == 0", [(-30, 30, 40), (200, 300, 12)]),
        # c = 0 (d = 0 x 40 wins); on d = 5, |x - y| = 5: j = 50 is exactly 0.1 (not far), 49 is far, 51 is not
        D("far_exact", "10 |X - Y| == |X| hit exactly", [(0, 200, 40), (5, 40, 21)]),
        D("far_below", "10 |X - Y| == |X| missed by one from below (the segment ends at j = 49)", [(0, 200, 40), (5, 39, 11)]),
        D("far_above", "10 |X - Y| == |X| missed by one from above (the segment starts at j = 51)", [(0, 200, 40), (5, 51, 11)]),
        # d = 4: 25 * 4 == 4 * 25 at j = 25 exactly (0.16 is not < 0.16); j = 26 counts, j = 24 does not
        D("c10_exact", "25 |j - i| == 4 j hit exactly", [(4, 15, 21)]),
        D("c10_below", "25 |j - i| == 4 j missed by one (the segment ends at j = 24)", [(4, 14, 11)]),
        D("c10_above", "25 |j - i| == 4 j missed by one (the segment starts at j = 26)", [(4, 26, 11)]),
        # kept dots with j == 0: (0, 8) in one, (0, 0) in the other (the only dot that a missing j > 0 filter could count)
        D("j0_kept", "a kept dot with j == 0", [(8, 0, 15), (60, 100, 12)]),
        D("j0_i0_kept", "a kept dot with j == 0 and i == 0", [(0, 0, 15), (60, 100, 12)]),
        D("g10_g11", "groups of exactly 10 and 11 dots", [(0, 200, 10), (50, 300, 11)]),
        D("g10_only", "a group of exactly 10 dots and nothing else (C1 keeps nothing)", [(0, 200, 10)]),
        D("g50_g51", "groups of exactly 50 and 51 dots", [(0, 200, 50), (50, 300, 51)]),
        D("g50_only", "groups of 50 and 30: none above 50, the largest stays", [(0, 200, 50), (50, 300, 30)]),
        D("tie_below_51", "a largest-size tie below 51", [(0, 200, 30), (50, 300, 30), (100, 400, 20)]),
        # 6 + 6 dots: one group of 12 when the values are 9 apart, two groups of 6 when they are 10 apart - on i - j (the forward
        # segments) and on i + j (the anti segments, i + j = 1000 and 1009 / 1010)
        D("gap9", "gaps of 9 on each axis", [(0, 200, 6), (9, 300, 6)], [(400, 600, 6), (250, 759, 6)]),
        D("gap10", "gaps of 10 on each axis", [(0, 200, 6), (10, 300, 6)], [(400, 600, 6), (250, 760, 6)]),
        # the anti segment's i - j = 10, 8, ..., -12 lie in list 0 beside d = 0 x 40; its dot with i - j = 0 is in the winning sub-list
        D("anti_in_winner", "anti-diagonal segment inside the winning list", [(0, 200, 40), (500, 100, 11)], [(300, 310, 12)]),
        D("anti_outside", "anti-diagonal segment outside the winning list", [(0, 200, 40), (500, 100, 11)], [(300, 700, 12)]),
        D("anti_60", "an anti-diagonal segment of 60 beside a diagonal of 40 (C2's second step keeps it)", [(0, 200, 40)], [(500, 900, 60)]),
        D("dup_tuples", "duplicated tuples", [(0, 200, 20), (30, 300, 15)], dup=(0,)),
        # wide route only: the two count10 / j == 0 cases with a coordinate above 65 535
        D("c10_exact_wide", "25 |j - i| == 4 j hit exactly above 65 535 (j = 75 000, i - j = 12 000)", [(12000, 74990, 21)], wide_only=True),
        D("j0_i0_wide", "a kept dot with j == 0 and i == 0 beside i > 65 535", [(0, 0, 15), (70000, 100, 12)], wide_only=True),
    ]
    return out


NAMED = _named()
BY_NAME = {d.name: d for d in NAMED}


def random_designs(n=200, seed=2024, buildable=False):
    """Seeded random designs: 1-7 forward segments of 11-100 dots, sometimes anti segments and noise.  buildable: the segments'
    stretches of the read do not overlap (build_pair can spell them)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        fwd, anti, noise, used = [], [], [], []

        def free(a, b):
            return a >= 0 and all(b + 45 < x or a > y + 45 for x, y in used)
        for _ in range(int(rng.integers(1, 8))):
            ln = int(rng.integers(11, 101))
            j0 = int(rng.integers(0, 1500))
            d = int(rng.choice([rng.integers(-60, 61), rng.integers(-600, 601), rng.choice([-30, 0, 10, 20, 50])]))
            if free(j0 + d, j0 + d + ln):
                fwd.append((d, j0, ln))
                used.append((j0 + d, j0 + d + ln))
        if not fwd:
            continue
        if rng.random() < 0.4:
            ln = int(rng.integers(11, 70))
            j0, i0 = int(rng.integers(0, 1500)), int(rng.integers(100, 2100))
            if free(i0 - ln, i0):
                anti.append((j0, i0, ln))
                used.append((i0 - ln, i0))
        if rng.random() < 0.5 and not buildable:
            noise = [(int(a), int(b)) for a, b in rng.integers(0, 2200, size=(int(rng.integers(1, 12)), 2))]
        out.append(Design("rand%d_%d" % (seed, len(out)), "random", fwd, anti, noise))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the reference, and its mutants
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = ("far_ge", "x0_always_far", "x0_never_far", "median_lower", "l1_tie_first", "l2_tie_first", "edge_le", "max_in_list9",
           "skip_level2", "c10_le", "c10_no_j_filter", "abs_over_all")


def _number_cluster(values, edges, mutant):
    if mutant not in ("edge_le", "max_in_list9"):
        return oracle.number_cluster(values, edges)
    bins = [[] for _ in edges]
    a, b = 0, 1
    values.sort()
    while a < len(values) and b < len(edges):
        if (values[a] <= edges[b]) if mutant == "edge_le" else (values[a] < edges[b]):
            bins[b - 1].append(values[a])
            a += 1
        else:
            b += 1
    if a < len(values):
        bins[-2 if mutant == "max_in_list9" else -1] += values[a:]
    return bins


def _edges(v):
    lo, hi = min(v), max(v)
    return [lo + t * float(hi - lo) / 10.0 for t in range(11)]


def r4_lists(kept, mutant=None):
    """(c, number of longest sub-lists, those sub-lists): dis_to_diagnal_most_abundant_defined (SF:582-591) step by step."""
    d = [int(x[1]) - int(x[0]) for x in kept]
    kept1 = oracle.find_longest_list(_number_cluster(d, _edges(d), mutant))
    if mutant == "l1_tie_first":
        kept1 = kept1[:1]
    if mutant == "skip_level2":
        kept2 = kept1
    else:
        kept2 = []
        for km in kept1:
            kept2 += oracle.find_longest_list(_number_cluster(km, _edges(km), mutant))
    n_lists = len(kept2)
    if mutant == "l2_tie_first":
        kept2 = kept2[:1]
    if len(kept2) == 1:
        if mutant == "median_lower":
            return float(sorted(kept2[0])[(len(kept2[0]) - 1) // 2]), n_lists, kept2
        return np.median(kept2[0]), n_lists, kept2
    return 0, n_lists, kept2


def _rel(dot, mutant):
    if dot[0] == 0:
        if mutant == "x0_always_far":
            return 1.0
        if mutant == "x0_never_far":
            return 0.0
    return oracle.eu_dis_single_dot(dot)


def r4_words(kept, mutant=None):
    """Words 10-13 of the record for the C1-kept dots `kept` (a non-empty list of [j, i]): 2 c, the dots (j + c, i) that
    eu_dis_single_dot puts above 0.1, twice the sum of x - y over them, and the number of longest sub-lists."""
    c, n_lists, _lists = r4_lists(kept, mutant)
    moved = [[d[0] + c, d[1]] for d in kept]
    if mutant == "far_ge":
        far = [d for d in moved if _rel(d, mutant) >= 0.1]
    elif mutant in ("x0_always_far", "x0_never_far"):
        far = [d for d in moved if _rel(d, mutant) > 0.1]
    else:
        far = [d for d in moved if oracle.eu_dis_single_dot(d) > 0.1]
    return [int(round(2 * float(c))), len(far), int(round(2 * float(sum(d[0] - d[1] for d in far)))), n_lists]


class Reference:
    """Everything expected() needs of one dot list, computed once: the cleaners' flags and, per mutant, the fourteen words."""

    def __init__(self, hits):
        self.h = np.ascontiguousarray(hits, dtype=np.int32).reshape(-1, 2)
        self.k1 = oracle.clean_c1_flags(self.h)
        self.k2 = oracle.clean_c2_flags(self.h)
        self._words = {}

    def words(self, mutant=None):
        if mutant in self._words:
            return self._words[mutant]
        h = self.h
        w = [0] * 14
        w[0] = len(h)
        w[1] = w[2] = -1
        if len(h):
            L = h.tolist()
            kept1 = [L[t] for t in np.flatnonzero(self.k1)]
            kept2 = [L[t] for t in np.flatnonzero(self.k2)]
            w[1], w[2] = min(x[0] for x in L), max(x[0] for x in L)
            w[3] = len(kept1)
            w[4] = sum(abs(j - i) for j, i in (L if mutant == "abs_over_all" else kept1))
            w[5] = len(kept2)
            if mutant == "c10_le":
                w[6] = len([x for x in (abs(float(j - i) / float(j)) for j, i in kept2 if j > 0) if x <= 0.16])
            elif mutant == "c10_no_j_filter":       # (a j == 0 dot taken with eu_dis_single_dot's denominator, j + 1)
                w[6] = len([x for x in (abs(float(j - i) / float(j if j > 0 else 1)) for j, i in kept2) if x < 0.16])
            else:
                w[6] = oracle.eu_dis_dots_within_10perc(kept2)
            w[7] = sum(1 for j, i in L if j == i)
            w[8] = sum(1 for j, i in L if j > i)
            w[9] = int((self.k2 == 1).sum())
            if kept1:
                w[10:14] = r4_words(kept1, mutant)
        self._words[mutant] = w
        return w

    def flag_bytes(self, flags):
        f = np.zeros(len(self.h), dtype=np.uint8)
        if flags & 1:
            f |= (self.k1 > 0).astype(np.uint8)
        if flags & 2:
            f |= (self.k2 == 1).astype(np.uint8) * 2 + (self.k2 == 2).astype(np.uint8) * 4
        return f

    def expected(self, flags, mutant=None):
        w = list(self.words(mutant))
        if not flags & 1:                           # mask_flags of oracle/cpu_twin.cpp
            w[3] = w[4] = 0
        if not flags & 2:
            w[5] = w[6] = w[9] = 0
        if not (flags & 4 and flags & 1):
            w[10] = w[11] = w[12] = w[13] = 0
        return w, self.flag_bytes(flags)


def expected(hits, flags, mutant=None):
    """Words 0-13 of the record of one dot list under pair flags `flags`, and its per-dot flag bytes."""
    return Reference(hits).expected(flags, mutant)


def anti_runs(kept, values):
    """Over the anti-diagonal runs (j + t, i - t) of at least 2 dots among the dots `kept` (what the device holds as one reverse-complement record
    where a shared join cuts an inverted slice): (the most consecutive dots of one run whose i - j is in `values`, the longest run
    with no i - j in `values`)."""
    s = set(map(tuple, kept))
    inside = outside = 0
    for j, i in s:
        if (j - 1, i + 1) in s:
            continue
        n = 1
        while (j + n, i - n) in s:
            n += 1
        if n < 2:
            continue
        cur = best = 0
        for t in range(n):
            cur = cur + 1 if (i - t) - (j + t) in values else 0
            best = max(best, cur)
        inside = max(inside, best)
        if best == 0:
            outside = max(outside, n)
    return inside, outside


def killers(cases, mutants=MUTANTS, first_only=True):
    """{mutant: [names of the cases on which it differs from expected() in one of words 0-13]}; cases = [(name, Reference)]."""
    out = {}
    for m in mutants:
        out[m] = []
        for name, ref in cases:
            if ref.words(m) != ref.words(None):
                out[m].append(name)
                if first_only:
                    break
    return out


# ---------------------------------------------------------------------------------------------------------------------
# sequences from designs
# ---------------------------------------------------------------------------------------------------------------------
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def _rand_dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def _other(rng, *avoid):
    return str(rng.choice([c for c in "ACGT" if c not in avoid]))


def build_pair(rng, k, design, min_len=2000, max_len=4000):
    """(read, allele): the allele is random DNA; the read is the design's segments in read order - a forward segment (d, j0, n) the
    allele slice [j0, j0 + n + k - 1) at read position j0 + d, an anti segment (j0, i0, n) the reverse complement of that slice
    ending with its k-mer at i0 - with random filler between them whose first and last base differ from the base that would
    extend the neighbouring match, so that a segment gives exactly n dots.  ValueError when the read stretches touch."""
    assert not design.dup
    parts = []                                        # (read start, read end, j0, length, anti)
    for d, j0, n in design.fwd:
        parts.append((j0 + d, j0 + d + n + k - 1, j0, n + k - 1, False))
    for j0, i0, n in design.anti:
        parts.append((i0 - n + 1, i0 + k, j0, n + k - 1, True))
    for j, i in design.noise:
        parts.append((i, i + k, j, k, False))
    parts.sort()
    if not parts or parts[0][0] < 0 or any(b[0] - a[1] < 1 for a, b in zip(parts, parts[1:])):
        raise ValueError("design %s cannot be spelled as a read" % design.name)
    n_al = max(max(j0 + ln for _a, _b, j0, ln, _r in parts) + 1, int(rng.integers(min_len, max_len)))
    allele = _rand_dna(rng, n_al)

    def ext(part, left):
        """the read base that would extend the part's match on that side ('' when the allele ends there)"""
        _a, _b, j0, ln, anti = part
        if anti:
            p = j0 + ln if left else j0 - 1
            return _COMP[allele[p]] if 0 <= p < n_al else ""
        p = j0 - 1 if left else j0 + ln
        return allele[p] if 0 <= p < n_al else ""

    read, pos, prev = [], 0, None
    for part in parts + [None]:
        end = part[0] if part else max(pos + 1, int(rng.integers(min_len, max_len)))
        gap = end - pos
        if gap > 0:
            fill = list(_rand_dna(rng, gap))
            lo_avoid = ext(prev, False) if prev else ""
            hi_avoid = ext(part, True) if part else ""
            if gap == 1:
                fill[0] = _other(rng, lo_avoid, hi_avoid)
            else:
                fill[0] = _other(rng, lo_avoid)
                fill[-1] = _other(rng, hi_avoid)
            read.append("".join(fill))
        if part:
            _a, b, j0, ln, anti = part
            sl = allele[j0:j0 + ln]
            read.append(revcomp(sl) if anti else sl)
            pos, prev = b, part
    return "".join(read), allele


# ---------------------------------------------------------------------------------------------------------------------
# the four case sets (built once per process; a Reference is computed once per case and never changed)
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Case:
    """One dot list of a case set: name, dots, and its Reference (made at first use)."""

    def __init__(self, name, hits):
        self.name, self.hits = name, hits
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = Reference(self.hits)
        return self._ref


def _case(design):
    return _once(("case", design.name), lambda: Case(design.name, design.dots()))


def narrow_named():
    return [d for d in NAMED if not d.wide_only]


def rw_of(cases):
    """vapor_clean_hits' bitmap words for a batch: min(max over lists of (max i + max j + 4 + 31) / 32, 4096)."""
    return min(max((int(c.hits[:, 0].max()) + int(c.hits[:, 1].max()) + 35) // 32 for c in cases if len(c.hits)), 4096)


def small_cases(band=None, n_random=200):
    """Small lists (clean_kernel, one-dot records).  band None: the named and random designs; band 0 / 1 / 2: those plus the
    lists that put the batch's largest i + j into the band of clean_kernel<4> / <8> / <CLEAN_PER_MAX>.
    clean_plan::width picks the instantiation by per = ceil(rw / 256) (<= 4, <= 8, else), rw = rw_of(batch): max i + max j <= 32 764
    gives rw <= 1024, <= 65 532 gives rw <= 2048, and the corner 65 535 + 65 535 = 131 070 gives the cap, 4096."""
    base = [_case(d) for d in narrow_named()] + [_case(d) for d in random_designs(n_random)]
    if band is None:
        return base
    d = BY_NAME["far_exact"]
    mj, mi = d.extent()
    if band == 0:
        s = (32764 - mj - mi) // 2
        extra = [_case(OWN_3270), _case(d.shift(s, 32764 - mj - mi - s))]
    elif band == 1:
        s = (65532 - mj - mi) // 2
        extra = [_case(OWN_4096), _case(d.shift(s, 65532 - mj - mi - s))]
    else:
        c = BY_NAME["single_d0"]
        extra = [_case(OWN_4096), _case(c.shift(MAX_SEQ - 239, MAX_SEQ - 239)), _case(BY_NAME["x0_inside_even"].shift(65000, 0)),
                 _case(BY_NAME["tie_l2"].shift(0, 63000))]
    return base + extra


def big_cases():
    """Big lists (clean_big_kernel): the named designs scaled to more than 4 096 dots - vapor_clean_hits stages at most 4 096
    records - and three of more than 65 535 dots (the rule ndots > 65535u), all within coordinates 0 .. 65 535."""
    out = []
    for d in narrow_named():
        out.append(_case(d.scale(-(-4097 // (d.n_dots() - len(d.noise))))))
    for name, s in (("tie_l1", 1100), ("median_half", 1060), ("x0_inside_even", 940)):
        out.append(_case(BY_NAME[name].scale(s)))
    assert all(len(c.hits) > 4096 for c in out) and sum(len(c.hits) > 65535 for c in out) == 3
    return out


def stretched():
    """Named designs with every i - j multiplied until the plot reaches the wide limit; the two-sided ones get an i - j range
    above 2^24 / 10, where 10 * (v - lo) no longer fits the narrow route's float24 quotient and wide_bin needs 64 bits."""
    out = []
    for d in narrow_named():
        if d.name in ("own_3270", "own_4096"):
            continue
        lo, hi = d.d_range()
        m = max(abs(lo), abs(hi))
        if m == 0:
            continue
        mj, mi = d.extent()
        f = (MAX_WIDE - max(mj, mi) - 64) // m
        out.append(d.stretch(f))
    return out


def wide_cases(n_random=40):
    """Lists for vapor_clean_hits_wide with a coordinate above 65 535: named and random designs moved out on j, on i and on
    both, every big list moved the same three ways, stretched designs and the wide-only ones."""
    out = []
    named = narrow_named()
    for q, d in enumerate(named + random_designs(n_random)):
        out.append(_case(d.shift(70000 + 1000 * q, 0)))
        out.append(_case(d.shift(0, 70000 + 3000 * q)))
        out.append(_case(d.shift(900000 - 2000 * q, 900000 - 2000 * q)))
    for d in narrow_named():                          # the whole big set, the three lists above 65 535 dots included
        s = d.scale(-(-4097 // (d.n_dots() - len(d.noise))))
        out += [_case(s.shift(70000, 0)), _case(s.shift(0, 300000)), _case(s.shift(500000, 500000))]
    for name, f in (("tie_l1", 1100), ("median_half", 1060), ("x0_inside_even", 940)):
        s = BY_NAME[name].scale(f)
        out += [_case(s.shift(70000, 0)), _case(s.shift(0, 300000)), _case(s.shift(500000, 500000))]
    out += [_case(d) for d in stretched()] + [_case(d) for d in NAMED if d.wide_only]
    assert all(int(c.hits.max()) > MAX_SEQ and int(c.hits.max()) <= MAX_WIDE for c in out)
    return out


class SeqCase:
    """One (read, allele[off2:]) pair at window size k, with the oracle's dots and the Reference over them."""

    def __init__(self, name, k, read, allele, off2=0, design=None):
        self.name, self.k, self.read, self.allele, self.off2, self.design = name, k, read, allele, off2, design
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            st, h, _k1, _k2 = oracle.pair_stats(self.k, self.read, self.allele[self.off2:], want_hits=True)
            self._ref = Reference(h.copy())
            w = self._ref.words()
            assert w[:10] == st[:10].tolist(), (self.name, w[:10], st[:10].tolist())      # (the two statements of words 0-9 agree)
        return self._ref

    @property
    def hits(self):
        return self.ref.h


def sequence_cases(n_random=40):
    """Sequence-built designs for the plan route: every named design a read can spell, at k = 20, 30, 40 and 10 in turn (and a
    few more at k = 10, where random 10-mers add loose dots of their own), random designs, and one case with off2 > 0.
    The expectations come from the oracle on the real sequences; the construction only decides what the cases reach."""
    def make():
        out = []
        rng = np.random.default_rng(77)
        q = 0
        for d in narrow_named():
            if d.lists_only:
                continue
            k = (20, 30, 40, 10)[q % 4]
            q += 1
            rd, al = build_pair(rng, k, d)
            out.append(SeqCase("%s@k%d" % (d.name, k), k, rd, al, 0, d))
        for name in ("x0_inside_even", "median_half", "tie_l1"):            # (once more: at k = 10, or at 20 if that was its turn)
            k = 20 if any(c.name == name + "@k10" for c in out) else 10
            rd, al = build_pair(rng, k, BY_NAME[name])
            out.append(SeqCase("%s@k%d" % (name, k), k, rd, al, 0, BY_NAME[name]))
        rd, al = build_pair(rng, 20, BY_NAME["x0_inside_odd"])
        pre = _rand_dna(rng, 137)
        out.append(SeqCase("x0_inside_odd@k20+off2", 20, rd, pre + _other(rng, al[0]) + al, 138, BY_NAME["x0_inside_odd"]))
        for d in random_designs(n_random, seed=4048, buildable=True):
            k = int(rng.choice([10, 20, 30, 40]))
            rd, al = build_pair(rng, k, d)
            out.append(SeqCase("%s@k%d" % (d.name, k), k, rd, al, 0, d))
        return out
    return _once("seq", make)


def doubled_33kb_case():
    """An allele holding the same 32 750 bases twice and a read that is one copy and 60 bases more, at k = 20: 65 563 dots in
    run records of up to 32 - more than 65 535 dots, so the plan route cleans it in clean_big_kernel (both sequences stay
    within VAPOR_MAX_SEQ_LEN)."""
    def make():
        x = _rand_dna(np.random.default_rng(33), 32750)
        return SeqCase("doubled_33kb@k20", 20, x + x[:60], x + x)
    return _once("doubled", make)
