"""The finishing step stated once, in plain Python: from the integer statistics records to per-read scores and from a locus's
scores to VaPoR_QS / GS / GT / GQ.

A plain helper module (no pytest hooks).  No numpy in the arithmetic, no import of vapor_amd.finish, no kernel: Python floats
are IEEE doubles, and every operation below is the reference's own, in the reference's order (SF = vapor_vali/Simple_function.pyx
of the reference):
  * the three scorers' gates, SF:182-203 (abs_dis_m1b), SF:277-294 (within_10Perc_m1b), SF:241-257 (directed_dis ... redefine_diagnal);
  * the drivers' per-read rule, SF:1718-1726: a read is skipped when `0 in [a, b]`, its score is 1 - b / a, a deletion takes the
    smaller of the abs_dis and the within_10Perc score or the only valid one;
  * result_organize_ins, SF:1219-1231: GS = positives / scored, QS = np.mean of the positives (numpy's pairwise order, written
    out in qs_numpy);
  * gt_estimate_log_likelihood, SF:2054-2069, through a (k, l) -> (GT, GQ) table, l counted on the rounded scores.
A record is sixteen integers (include/vapor_hip.h); a record whose word 15 is not zero belongs to a pair that failed, and a
read that points at one scores nothing with it.

MUTANTS are the same statements with exactly one rule wrong; they exist to show that tests/finish_cases.py can tell each of
them from the right one (tests/test_finish_model_cpu.py)."""

N_HITS, FIRST_J, LAST_J, C1_KEPT, C1_SUM_ABS, C2_KEPT, C2_COUNT10, DIR_N, DIR_SUM2, STATUS = 0, 1, 2, 3, 4, 5, 6, 11, 12, 15
GT_TABLE_N = 65               # the table holds k, l in 0 .. 64
LOCUS_STRIDE = 8
CHUNK = 256                   # reads per chunk of the kernel's documented order
NAN = float("nan")

MUTANTS = (
    "hits_gate_ge",           # >= 0.1 for > 0.1
    "span06_ge",              # >= 0.6 for > 0.6
    "span07_ge",              # >= 0.7 for > 0.7
    "spans_swapped",          # S1 asks for 0.7, S3 for 0.6
    "s1_len_ref",             # len_ref for min(len_ref, len_alt) in S1
    "s2_min",                 # min for max in S2's gate
    "s2_ref_first",           # S2's outputs not swapped
    "hits_ge_2",              # n_hits >= 2 for > 2
    "kept_gates_dropped",     # C1_KEPT > 0 / C2_KEPT > 0 not asked (see _kept below for what of that can show)
    "dir_n0_dropped",         # DIR_N == 0 -> 0.0001 not applied
    "dir_no_abs",             # abs dropped from the directed value
    "del_max",                # kind 0 takes the larger score
    "del_s1_only",            # kind 0 takes S1's score whenever it is valid
    "nonpos_unrounded",       # `not s > 0` for `not round(s, 2) > 0`
    "table_le_65",            # n <= 65 for n < 65
    "table_lt_64",            # n < 64 for n < 65
    "gs_ge",                  # GS >= .15
    "sum_left_to_right",      # the positives added one by one
    "partials_left_to_right", # the eight partial sums combined as ((((((0+1)+2)+3)+4)+5)+6)+7
    "partials_by_slot",       # a positive goes to the partial sum of its read slot, not of its rank among the positives
    "failed_record_used",     # word 15 not looked at
)


class Model:
    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.m = mutant

    # -----------------------------------------------------------------------------------------------------------------
    # the scorers: [a, b] as the reference's functions return them
    # -----------------------------------------------------------------------------------------------------------------
    def _over(self, x, bound):
        ge = {0.1: "hits_gate_ge", 0.6: "span06_ge", 0.7: "span07_ge"}[bound]
        return x >= bound if self.m == ge else x > bound

    def _kept(self, n):
        # (dropped, the gate shows in S3 only: S1 then divides by zero - NaN on the device, a read that is skipped either
        # way - and S2 returns a count of 0, which `0 in [a, b]` skips as well)
        return True if self.m == "kept_gates_dropped" else n > 0

    def s1(self, r, a, len_ref, len_alt):
        """calcu_vapor_single_read_score_abs_dis_m1b, SF:182-203."""
        nr, na = int(r[N_HITS]), int(a[N_HITS])
        span = 0.7 if self.m == "spans_swapped" else 0.6
        if (nr >= 2 and na >= 2) if self.m == "hits_ge_2" else (nr > 2 and na > 2):
            shorter = float(len_ref) if self.m == "s1_len_ref" else min([float(len_ref), float(len_alt)])
            if self._over(float(nr) / shorter, 0.1):
                r_ok = self._over(float(int(r[LAST_J]) - int(r[FIRST_J])) / float(len_ref), span)
                a_ok = self._over(float(int(a[LAST_J]) - int(a[FIRST_J])) / float(len_alt), span)
                if r_ok and a_ok:
                    kr, ka = int(r[C1_KEPT]), int(a[C1_KEPT])
                    if self._kept(kr) and self._kept(ka):
                        if kr == 0 or ka == 0:
                            return [NAN, NAN]
                        return [float(int(r[C1_SUM_ABS])) / float(kr), float(int(a[C1_SUM_ABS])) / float(ka)]     # mean |j - i|
                    return [0, 0]
                if r_ok:
                    return [1.1, 2.1]
                if a_ok:
                    return [2.1, 1.1]
                return [0, 0]
            return [0, 0]
        return [0, 0]

    def s2(self, r, a, len_ref, len_alt):
        """calcu_vapor_single_read_score_within_10Perc_m1b, SF:277-294: the alt count first."""
        ratios = [float(int(r[N_HITS])) / float(len_ref), float(int(a[N_HITS])) / float(len_alt)]
        if self._over(min(ratios) if self.m == "s2_min" else max(ratios), 0.1):
            if self._kept(int(r[C2_KEPT])) and self._kept(int(a[C2_KEPT])):
                if self.m == "s2_ref_first":
                    return [int(r[C2_COUNT10]), int(a[C2_COUNT10])]
                return [int(a[C2_COUNT10]), int(r[C2_COUNT10])]
            return [0, 0]
        return [0, 0]

    def _directed(self, s):
        """eu_dis_dir_calcu over the moved dots (SF:718-722): 0.0001 for an empty list, else the mean of x - y; the record holds
        twice the sum (word 12) and the count (word 11)."""
        n = int(s[DIR_N])
        if n == 0 and self.m != "dir_n0_dropped":
            return 0.0001
        if n == 0:
            return NAN
        v = (float(int(s[DIR_SUM2])) * 0.5) / float(n)
        return v if self.m == "dir_no_abs" else abs(v)

    def s3(self, r, a, len_ref, len_alt):
        """calcu_vapor_single_read_score_directed_dis_m1b_redefine_diagnal, SF:241-257."""
        span = 0.6 if self.m == "spans_swapped" else 0.7
        if (self._over(float(int(r[N_HITS])) / float(len_ref), 0.1) and self._over(float(int(a[N_HITS])) / float(len_alt), 0.1)
                and self._over(float(int(r[LAST_J]) - int(r[FIRST_J])) / float(len_ref), span)
                and self._over(float(int(a[LAST_J]) - int(a[FIRST_J])) / float(len_alt), span)):
            if self._kept(int(r[C1_KEPT])) and self._kept(int(a[C1_KEPT])):
                return [self._directed(r), self._directed(a)]
            return [0, 0]
        return [0, 0]

    # -----------------------------------------------------------------------------------------------------------------
    # one read
    # -----------------------------------------------------------------------------------------------------------------
    def _one(self, fn, r, a, len_ref, len_alt):
        """The score of one scorer, or None: a failed pair scores nothing, `0 in [a, b]` skips the read (SF:1718)."""
        if self.m != "failed_record_used" and (int(r[STATUS]) != 0 or int(a[STATUS]) != 0):
            return None
        x = fn(r, a, len_ref, len_alt)
        if 0 in x:
            return None
        v = 1 - float(x[1]) / float(x[0])
        return None if v != v else v                      # (only the mutants that divide by zero get here with a NaN)

    def score(self, kind, st_ref_a, st_alt_a, st_ref_b, st_alt_b, len_ref, len_alt):
        """The score of one read, or None when it is skipped.  kind 1 / 2 / 3: S1 / S2 / S3 on the records `a`; kind 0 (a
        deletion, SF:1716-1726): S1 on the records `a`, S2 on the records `b`, the smaller of the two valid scores or the only
        valid one.  Lengths are at least 1."""
        assert len_ref >= 1 and len_alt >= 1
        if kind == 0:
            v1 = self._one(self.s1, st_ref_a, st_alt_a, len_ref, len_alt)
            v2 = self._one(self.s2, st_ref_b, st_alt_b, len_ref, len_alt)
            if v1 is not None and v2 is not None:
                if self.m == "del_s1_only":
                    return v1
                return max([v1, v2]) if self.m == "del_max" else min([v1, v2])
            return v1 if v1 is not None else v2
        fn = {1: self.s1, 2: self.s2, 3: self.s3}[kind]
        return self._one(fn, st_ref_a, st_alt_a, len_ref, len_alt)

    # -----------------------------------------------------------------------------------------------------------------
    # the mean of the positives, two orders
    # -----------------------------------------------------------------------------------------------------------------
    def _eight(self, a):
        """numpy's unrolled block: fewer than 8 values one by one from 0.0; otherwise eight strided partial sums over the first
        n - n % 8 values, combined as ((0+1)+(2+3))+((4+5)+(6+7)), then the last n % 8 values one by one."""
        n = len(a)
        if n < 8 or self.m == "sum_left_to_right":
            res = 0.0
            for v in a:
                res += v
            return res
        r = list(a[:8])
        full = n - n % 8
        for i in range(8, full, 8):
            for q in range(8):
                r[q] += a[i + q]
        if self.m == "partials_left_to_right":
            res = r[0]
            for q in range(1, 8):
                res += r[q]
        else:
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(full, n):
            res += a[i]
        return res

    def _pairwise(self, a):
        """numpy's pairwise_sum: the unrolled block up to 128 values, above that two halves, the first a multiple of 8."""
        n = len(a)
        if n <= 128:
            return self._eight(a)
        half = n // 2
        half -= half % 8
        return self._pairwise(a[:half]) + self._pairwise(a[half:])

    def _positives(self, slots):
        """The values the sums run over.  `slots`: one entry per read, None for a skipped one."""
        if self.m == "partials_by_slot":                  # (every slot takes part; what is not positive adds 0.0)
            return [s if s is not None and s > 0 else 0.0 for s in slots]
        return [s for s in slots if s is not None and s > 0]

    def qs_numpy(self, pos):
        """np.mean(pos) for a non-empty list of doubles: numpy's add.reduce order, then one division."""
        return self._pairwise(list(pos)) / float(len(pos))

    def qs_kernel(self, scores):
        """The order finish_kernel documents: the reads (None = skipped) in chunks of 256, the positives of a chunk summed with
        the eight-partial rule whatever their count, the chunk sums added left to right; 0.0 without a positive."""
        npos = len([s for s in scores if s is not None and s > 0])
        res = 0.0
        for base in range(0, len(scores), CHUNK):
            res += self._eight(self._positives(scores[base:base + CHUNK]))
        return res / float(npos) if npos > 0 else 0.0

    # -----------------------------------------------------------------------------------------------------------------
    # one locus
    # -----------------------------------------------------------------------------------------------------------------
    def locus(self, scores, gt_table, order="numpy"):
        """The eight doubles of one locus record [QS, GS, GT index, GQ, n scored, n positive, n rounding to <= 0, 0.0] from its
        reads' scores (None = skipped), or the NA row (NaN, word 4 = 0.0) when no read is scored.  gt_table[k][l] = (GT, GQ).
        order: "numpy" (np.mean, the reference's) or "kernel" (qs_kernel)."""
        scored = [s for s in scores if s is not None]
        if len(scored) == 0:
            return [NAN, NAN, NAN, NAN, 0.0, NAN, NAN, NAN]
        pos = [s for s in scored if float(s) > 0]
        gs = float(len(pos)) / float(len(scored))
        if order == "kernel":
            qs = self.qs_kernel(list(scores))
        elif not pos:
            qs = 0.0
        elif self.m == "partials_by_slot":
            qs = self._pairwise(self._positives(list(scores))) / float(len(pos))
        else:
            qs = self.qs_numpy(pos)
        k = len(scored)
        if self.m == "nonpos_unrounded":
            l = len([s for s in scored if not s > 0])
        else:
            l = len([s for s in scored if not round(float(s), 2) > 0])      # (the Rec string's values, SF:1229 / 2055-2057)
        bound = {"table_le_65": GT_TABLE_N + 1, "table_lt_64": GT_TABLE_N - 1}.get(self.m, GT_TABLE_N)
        gt, gq = 1, NAN
        if k < bound:
            if k < len(gt_table):
                gt, gq = int(gt_table[k][l][0]), float(gt_table[k][l][1])
            else:
                gt, gq = 0, -1.0                          # (table_le_65 reads behind the table: anything but (1, NaN))
        if gt == 0 and (gs >= .15 if self.m == "gs_ge" else gs > .15):
            gt = 1
        return [qs, gs, float(gt), gq, float(k), float(len(pos)), float(l), 0.0]


_RIGHT = Model()
score, locus, qs_numpy, qs_kernel = _RIGHT.score, _RIGHT.locus, _RIGHT.qs_numpy, _RIGHT.qs_kernel
s1, s2, s3 = _RIGHT.s1, _RIGHT.s2, _RIGHT.s3


def mutant(name):
    """The model with the one rule `name` wrong."""
    return Model(name)
