"""Designed pairs for the any-k route (vapor_anyk_batch, vapor_amd/csrc/vapor_anyk.h): the smallest shapes at which each of its
mechanisms is reached - the bitonic sort's sizes and its padding, every window size, the last symbol of a k-mer at every byte
alignment, the 64-lane rounds of the edit pass, its launch split, and the state a call carries from pair to pair.

A plain helper module (no pytest hooks).  It holds
  * Pair: (seq1, seq2, off2, k, forward) with a name, its group and the property it is built for; its expected dots come from
    anyk_model (the restatement of kmerhits' two match rules), its statistics words 0-13 from dot_designs.expected();
  * the groups: sort_sizes(), every_k(), last_symbol(), edit_rounds(), edit_split(), batch_state() - built once per process;
  * the numbers of the route that the designs are aimed at, restated: entries() / padded() (n and np of the sort), per_of() /
    launches() (dots_plan::edit_cut; tools/dots_plan_check.cpp holds vapor_dots_plan.h to the same numbers), comparator_key()
    (anyk_cmp's order);
  * MUTANTS and mutant_hits(): deliberately wrong variants of the statement, each one way the kernels can be wrong, used only
    to show that the designs can tell them from the right one.

Coordinates are the project's (j, i): j the position in the allele (seq2[off2:]), i in the read (seq1)."""
import numpy as np

import anyk_model as model
import dot_designs as dd

PF_FORWARD = 8                      # VAPOR_PF_FORWARD: kmerhits(..., inversions=False)
E_KEYERROR = -3                   # (the GPU test holds both against vapor_amd._lib)
TILE = 512                          # ANYK_TILE
EDIT_PAIRS_DEFAULT = 1 << 31        # ANYK_EDIT_PAIRS, the default of "anyk_edit_pairs"
WAVES = 4                           # ANYK_EDIT_WAVES
_COMP = str.maketrans("ACGTacgtNn", "TGCAtgcaNn")


def revcomp(s):
    return s[::-1].translate(_COMP)


def _rand(rng, n, letters="ACGT"):
    return np.frombuffer(letters.encode(), dtype=np.uint8)[rng.integers(0, len(letters), n)].tobytes().decode()


def _other(c, avoid=""):
    return [x for x in "ACGT" if x != c.upper() and x not in avoid][0]


def entries(len1, k, forward):
    """n: the read's lookup entries (one per k-mer, two with inversions)."""
    nk1 = max(0, len1 - k + 1)
    return nk1 if forward else 2 * nk1


def padded(n):
    """np: the sort's array, the smallest power of two >= max(n, TILE)."""
    p = TILE
    while p < n:
        p <<= 1
    return p


def per_of(n, edit_pairs=None):
    """Allele k-mers per launch of the edit pass (dots_plan::edit_cut)."""
    return max(WAVES, (edit_pairs or EDIT_PAIRS_DEFAULT) // max(n, 1) // WAVES * WAVES)


def launches(n, nk2, edit_pairs=None):
    return -(-nk2 // per_of(n, edit_pairs))


def comparator_key(kmer):
    """anyk_cmp's total order on k-byte strings: word by word, each word a little-endian integer."""
    b = kmer.encode("latin-1")
    return tuple(int.from_bytes(b[t:t + 4], "little") for t in range(0, len(b), 4))


class Pair:
    def __init__(self, name, group, s1, s2, k, forward, why, off2=0, flags=3, edit_pairs=None, planted=(), **info):
        self.name, self.group, self.s1, self.s2, self.k, self.forward, self.why = name, group, s1, s2, k, forward, why
        self.off2, self.flags, self.edit_pairs, self.planted, self.info = off2, flags, edit_pairs, list(planted), info
        self._hits = self._ref = self._keys = None

    @property
    def pair_flags(self):
        return self.flags | (PF_FORWARD if self.forward else 0)

    @property
    def allele(self):
        return self.s2[self.off2:]

    @property
    def n(self):
        return entries(len(self.s1), self.k, self.forward)

    @property
    def np(self):
        return padded(self.n)

    @property
    def nk2(self):
        return max(0, len(self.allele) - self.k + 1)

    @property
    def per(self):
        return per_of(self.n, self.edit_pairs)

    @property
    def n_launches(self):
        return launches(self.n, self.nk2, self.edit_pairs)

    def keys(self):
        """k > 40: (keys in first-insertion order, their lists, dist[rank, j])."""
        if self._keys is None:              # (pairs that differ in off2 alone have the same seq2[off2:]: one statement for them)
            self._keys = _once(("keys", self.s1, self.allele, self.k, self.forward),
                               lambda: model.key_distances(self.s1, self.allele, self.k, not self.forward))
        return self._keys

    @property
    def D(self):
        return len(self.keys()[0]) if self.k > 40 else len(model.lookup(self.s1, self.k, not self.forward))

    @property
    def refused(self):
        """The status of a pair the route refuses before any device work (a seq1 outside invert_base's alphabet)."""
        if not self.forward and self.n > 0:
            try:
                model.lookup(self.s1, self.k, True)
            except KeyError:
                return E_KEYERROR
        return 0

    def hits(self):
        if self._hits is None:
            if self.refused or self.n == 0:
                self._hits = np.zeros((0, 2), dtype=np.int32)
            elif self.k > 40:
                _names, lists, dist = self.keys()
                self._hits = model.dots_of(lists, dist <= self.k // 10)
            else:
                self._hits = model.kmerhits_array(self.s1, self.allele, self.k, not self.forward)
            self._hits.setflags(write=False)
        return self._hits

    def expected(self, flags=None):
        """Words 0-13 of the record under the pair's flags (dot_designs.expected) and word 15."""
        if self._ref is None:
            self._ref = dd.Reference(self.hits())
        w, _fl = self._ref.expected(self.flags if flags is None else flags)
        if self.refused:
            w = [0, -1, -1] + [0] * 11
        return w, self.refused


# ---------------------------------------------------------------------------------------------------------------------
# the groups (built once per process)
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


SORT_FWD_N = (1, 2, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
SORT_INV_N = (512, 1024, 1026, 2048)


def _planted_read(rng, length, piece):
    """A random read with the piece at six places (where it fits): repeated 33-mers between unique ones."""
    s = list(_rand(rng, length))
    if length >= 6 * (len(piece) + 8):
        for t in range(6):
            p = t * (length // 6) + 3
            s[p:p + len(piece)] = piece
    return "".join(s)


def sort_sizes():
    """n at, one below and one above every array size from the LDS tile to 4096 (and 1, 2): a small k over two letters, so that
    eight k-mers share all entries - the list order is the tie-break's, every run is long and crosses the tiles - and k = 33
    with a piece planted six times; a read already in the comparator's order and one in the reverse of it."""
    def make():
        rng = np.random.default_rng(101)
        out = []
        for forward, sizes in ((True, SORT_FWD_N), (False, SORT_INV_N)):
            tag = "fwd" if forward else "inv"
            for n in sizes:
                nk1 = n if forward else n // 2
                s1 = _rand(rng, nk1 + 2, "AC")
                s2 = "AAACACCCAA" + (_rand(rng, 14, "AC") if forward else "GGGTGTTTGG" + _rand(rng, 6, "ACGT"))     # every 3-mer of the read
                out.append(Pair("%s_n%d_k3" % (tag, n), "sort_sizes", s1, s2, 3, forward, "n = %d over eight 3-mers" % n, flags=7 if n == 1024 else 3))
                piece = _rand(rng, 40)
                s1 = _planted_read(rng, nk1 + 32, piece)
                s2 = _rand(rng, 7) + piece + _rand(rng, 5) + s1[:50] + s1[-45:] + ("" if forward else revcomp(piece))
                out.append(Pair("%s_n%d_k33" % (tag, n), "sort_sizes", s1, s2, 33, forward, "n = %d, planted repeats" % n))
        s1 = _rand(rng, 1025)
        out.append(Pair("fwd_n1024_k2_acgt", "sort_sizes", s1, _rand(rng, 40), 2, True, "n = np = 1024 over sixteen 2-mers"))
        up = "A" * 257 + "C" * 256 + "G" * 256 + "T" * 257
        out.append(Pair("fwd_ascending", "sort_sizes", up, "AAACCCGGGTTTAACCGGTT", 3, True, "already in the comparator's order, n = np = 1024"))
        out.append(Pair("fwd_descending", "sort_sizes", up[::-1], "TTTGGGCCCAAATTGGCCAA", 3, True, "in the reverse of it"))
        return out
    return _once("sort_sizes", make)


EVERY_OFF2 = (1, 8, 13)
EVERY_OFF2_K = (37, 38, 39, 40, 41, 42, 43, 44)        # every residue of k mod 4 on both sides of 40


def _every_read(al):
    r = list(al[40:440])
    for p in (17, 61, 97, 203, 277, 351, 389):
        r[p] = _other(r[p])
    s = "".join(r)
    s = s[:120] + s[122:]
    s = s[:250] + "GT" + s[250:]
    s = s[:150] + revcomp(s[150:210]) + s[210:]
    s = s[:230] + s[230:270].lower() + s[270:]
    s = s[:300] + "NNNNNN" + s[306:]
    return s[:330] + "R" + s[331:]


def every_k():
    """One read of 400 symbols - substitutions, a deletion and an insertion of two, a reverse-complemented stretch, a lower-case
    stretch, an N run, a folded IUPAC letter - against the allele of 500 it was cut from, at every k from 1 to 64 with and
    without inversions, and at off2 = 1, 8, 13 (odd, a whole word of the 4-bit plane, both) for the eight k around 40.  The
    forward pairs carry symbols outside the alphabet, on both sides."""
    def make():
        rng = np.random.default_rng(202)
        al = _rand(rng, 500)
        rd = _every_read(al)
        al_f = al[:110] + "XUX" + al[113:] + "RYU"
        rd_f = _every_read(al_f) + "UXZ"
        out = []
        for k in range(1, 65):
            fl = 7 if k % 3 == 0 else 3
            out.append(Pair("inv_k%d" % k, "every_k", rd, al, k, False, "k = %d with inversions" % k, flags=fl))
            out.append(Pair("fwd_k%d" % k, "every_k", rd_f, al_f, k, True, "k = %d forward" % k, flags=fl))
        for off in EVERY_OFF2:
            pre = _rand(rng, off)
            for k in EVERY_OFF2_K:
                out.append(Pair("inv_k%d_off%d" % (k, off), "every_k", rd, pre + al, k, False, "off2 = %d" % off, off2=off))
                out.append(Pair("fwd_k%d_off%d" % (k, off), "every_k", rd_f, pre + al_f, k, True, "off2 = %d" % off, off2=off))
        return out
    return _once("every_k", make)


LAST_K = (5, 6, 7, 8, 37, 38, 39, 40)


def _align(parts, a, rng):
    """lower-case filler (at least one symbol) so that the next part starts at a position that is a mod 4"""
    at = sum(len(x) for x in parts)
    parts.append(_rand(rng, 1 + (a - at - 1) % 4, "acgt"))


def last_symbol():
    """Per k: four k-mers K_a at the four byte alignments of the read, each followed by a known symbol, and a last one that ends
    the read; the allele holds, at each of its four alignments, every K_a with its last symbol changed (no dot) and every K_a
    followed by another symbol than in the read (a dot), and ends with the read's last k-mer (a dot between the two k-mers whose
    last word reaches into the buffers' padding).  planted: (j, i, dot or not)."""
    def make():
        rng = np.random.default_rng(303)
        out = []
        for k in LAST_K:
            K = [_rand(rng, k) for _ in range(5)]
            parts, pos = [], []
            for a in range(4):
                _align(parts, a, rng)
                pos.append(sum(len(x) for x in parts))
                parts += [K[a], "ACGT"[a]]
            _align(parts, (k + 1) % 4, rng)
            pos.append(sum(len(x) for x in parts))
            parts.append(K[4])
            s1 = "".join(parts)
            parts, planted = [], []
            for b in range(4):
                for a in range(4):
                    _align(parts, b, rng)
                    planted.append((sum(len(x) for x in parts), pos[a], False))
                    parts.append(K[a][:-1] + _other(K[a][-1]))
                    _align(parts, b, rng)
                    planted.append((sum(len(x) for x in parts), pos[a], True))
                    parts += [K[a], _other("ACGT"[a])]
            _align(parts, k % 4, rng)
            planted.append((sum(len(x) for x in parts), pos[4], False))
            parts.append(K[4][:-1] + _other(K[4][-1]))
            _align(parts, (k + 2) % 4, rng)
            planted.append((sum(len(x) for x in parts), pos[4], True))
            parts.append(K[4])
            s2 = "".join(parts)
            for forward in (False, True):
                out.append(Pair("%s_k%d" % ("fwd" if forward else "inv", k), "last_symbol", s1, s2, k, forward,
                                "symbol k - 1 and symbol k at every alignment, k = %d" % k, planted=planted))
        return out
    return _once("last_symbol", make)


ROUND_K = (41, 50, 64)
ROUND_D = (1, 63, 64, 65, 128, 129)
A_RUNS = (9, 11, 8, 13, 10, 12, 9, 14, 11, 8, 12, 10, 13, 9)      # lengths of the A runs between two C of the low-complexity read


def _edits(key, e):
    """key with e substitutions spread over it (to a symbol the key does not hold there)"""
    q = list(key)
    for t in range(e):
        p = (2 * t + 1) * len(key) // (2 * e)
        q[p] = _other(q[p])
    return "".join(q)


def edit_rounds():
    """k > 40, forward: a read of period D has exactly D distinct keys, key r the k-mer at r, and the first three are listed
    twice.  The allele holds the keys of rank 0, 63, 64 and D - 1 as they are, with k // 10 substitutions and with one more.
    planted: (j, rank, substitutions).  Then a read of A runs of different lengths between single C, of period 151, probed by
    all-A k-mers: most lanes of a round contribute, with lists of two and three; and a tandem read with inversions."""
    def make():
        rng = np.random.default_rng(404)
        out = []
        for k in ROUND_K:
            t = k // 10
            for D in ROUND_D:
                unit = "A" if D == 1 else _rand(rng, D)
                s1 = (unit * (2 + (k + 3) // D))[:D + k - 1 + 3]
                cyc = unit * (2 + k // D)
                parts, planted = [], []
                for r in sorted({0, 63, 64, D - 1}):
                    if r >= D:
                        continue
                    for e in (0, t, t + 1):
                        parts.append(_rand(rng, 9, "acgt"))
                        planted.append((sum(len(x) for x in parts), r, e))
                        parts.append(_edits(cyc[r:r + k], e))
                s2 = "".join(parts) + "ac"
                out.append(Pair("fwd_k%d_D%d" % (k, D), "edit_rounds", s1, s2, k, True, "exactly %d distinct keys" % D, planted=planted, keys=D))
        period = "".join("A" * a + "C" for a in A_RUNS)
        low = (period * 4)[:520]
        for k in ROUND_K:
            s2 = _rand(rng, 12, "cgt") + "A" * (k + 2) + _rand(rng, 7, "cgt") + low[30:30 + k + 4]
            out.append(Pair("fwd_k%d_lowcomplexity" % k, "edit_rounds", low, s2, k, True, "many lanes of a round, lists of different lengths",
                            query=12))
        unit = _rand(rng, 23)
        tandem = (unit * 20)[:450]
        for k in ROUND_K:
            s2 = _rand(rng, 15) + _edits((unit * 5)[:k + 20], 1) + _rand(rng, 11) + revcomp((unit * 5)[3:k + 9]) + _rand(rng, 6)
            out.append(Pair("inv_k%d_tandem" % k, "edit_rounds", tandem, s2, k, False, "inversions, lists longer than one", flags=7))
        return out
    return _once("edit_rounds", make)


def golden_rounds():
    """The eight pairs of at most 200 symbols that the reference itself states (tools/gen_anyk_golden.py --designs): the reads
    of D = 64 and 65 at k = 41 and 64, forward and with inversions (which doubles the keys), against an allele that holds the
    key of rank D - 1 as it is, the key of rank 63 with k // 10 substitutions and, where 200 symbols have room, key 0 with one
    more."""
    def make():
        rng = np.random.default_rng(414)
        by_name = {p.name: p for p in edit_rounds()}
        out = []
        for k in (41, 64):
            for D in (64, 65):
                s1 = by_name["fwd_k%d_D%d" % (k, D)].s1
                s2 = "".join(_rand(rng, 5, "acgt") + _edits(s1[r:r + k], e) for r, e in ((D - 1, 0), (63, k // 10), (0, k // 10 + 1)))[:200]
                for forward in (True, False):
                    out.append(Pair("rounds_k%d_D%d_%s" % (k, D, "fwd" if forward else "inv"), "golden_rounds", s1, s2, k, forward,
                                    "D = %d%s" % (D, "" if forward else " doubled")))
        return out
    return _once("golden_rounds", make)


SPLIT_PER = (4, 8, 64)
SPLIT_K = 50
BIG_UNIT, BIG_COPIES, BIG_ALLELE = 100, 2000, 12200


def edit_split():
    """k = 50.  Per launch size per in 4, 8, 64 ("anyk_edit_pairs" = 252 per, which gives per for n = 251 and n = 252): a forward
    pair of 300 x 400 symbols and one with inversions (a read of 175), the allele holding k + per + 2 symbols of the read from
    j = per - 1 on - dots at per - 1, per, 2 per - 1, 2 per - and a piece at j = 300; the same pairs at the default are their
    reference.  Last, at the default: a unit of 100 repeated 2000 times, with inversions - n = 399 902, per = 5368, 200 keys -
    against 12 200 random symbols with k + 20 symbols of the unit, one to three substitutions in any k of them, from j = per - 10 and 2 per - 10 on."""
    def make():
        rng = np.random.default_rng(505)
        out = []
        k = SPLIT_K
        for per in SPLIT_PER:
            for forward in (True, False):
                s1 = _rand(rng, 300 if forward else 175)
                al = list(_rand(rng, 400))
                p1 = s1[10:10 + k + per + 2] if forward else revcomp(s1[5:5 + k + per + 2])
                al[per - 1:per - 1 + len(p1)] = p1
                al[300:300 + k + 3] = _edits(s1[60:60 + k + 3], 2)
                out.append(Pair("%s_per%d" % ("fwd" if forward else "inv", per), "edit_split", s1, "".join(al), k, forward,
                                "dots on both sides of per and 2 per, per = %d" % per, edit_pairs=252 * per,
                                planted=[per - 1, per, 2 * per - 1, 2 * per]))
        unit = _rand(rng, BIG_UNIT)
        s1 = unit * BIG_COPIES
        per = per_of(entries(len(s1), k, False))
        al = list(_rand(rng, BIG_ALLELE))
        cyc = unit * 3
        for e, (at, ph) in enumerate(((per - 10, 17), (2 * per - 10, 61))):
            al[at:at + k + 20] = _edits(cyc[ph:ph + k + 20], 2 + e)
        out.append(Pair("inv_default_3launches", "edit_split", s1, "".join(al), k, False, "the shipped launch size: three launches",
                        planted=[per - 1, per, 2 * per - 1, 2 * per]))
        return out
    return _once("edit_split", make)


def batch_state():
    """One call: a large edit pair; a small one at the same k whose allele holds a stretch from beyond the small read's length
    of the large read (a key or a first-entry mark left over from the large pair would give dots); an exact pair; a forward
    pair; a pair without k-mers; a pair refused with a KeyError; an edit pair again."""
    def make():
        rng = np.random.default_rng(606)
        big = _rand(rng, 600)
        big_al = _rand(rng, 40) + big[100:500] + revcomp(big[500:600]) + _rand(rng, 60)
        small = _rand(rng, 120)
        small_al = _rand(rng, 20) + small[20:110] + _rand(rng, 10) + big[300:380] + revcomp(big[420:500])
        ex = _rand(rng, 300)
        ex_al = _rand(rng, 50) + _every_read(_rand(rng, 40) + ex + _rand(rng, 200))[:320]
        fw = _rand(rng, 100) + "XU" + _rand(rng, 100)
        fw_al = _rand(rng, 30) + fw[40:180] + "UX" + _rand(rng, 30)
        last = _rand(rng, 150)
        last_al = revcomp(last[10:140]) + last[:70]
        P = Pair
        return [P("edit_large", "batch_state", big, big_al, 50, False, "n = 1102"),
                P("edit_small", "batch_state", small, small_al, 50, False, "fewer entries, fewer keys, after the large pair"),
                P("exact", "batch_state", ex, ex_al, 15, False, "an exact pair after an edit pair", flags=7),
                P("forward", "batch_state", fw, fw_al, 45, True, "forward after inversions"),
                P("no_kmers", "batch_state", small[:30], small_al, 41, False, "len < k"),
                P("keyerror", "batch_state", fw, fw_al, 7, False, "refused: seq1 outside the alphabet"),
                P("edit_again", "batch_state", last, last_al, 41, False, "an edit pair after all of them")]
    return _once("batch_state", make)


GROUPS = {"sort_sizes": sort_sizes, "every_k": every_k, "last_symbol": last_symbol, "edit_rounds": edit_rounds,
          "edit_split": edit_split, "batch_state": batch_state}


def contributing(pair, j):
    """k > 40: per round of 64 keys, the list lengths of the lanes whose key is within the threshold of allele k-mer j."""
    _names, lists, dist = pair.keys()
    ok = dist[:, j] <= pair.k // 10
    return [[len(lists[r]) for r in range(r0, min(r0 + 64, len(lists))) if ok[r]] for r0 in range(0, len(lists), 64)]


# ---------------------------------------------------------------------------------------------------------------------
# mutants of the statement
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "cmp_k_minus_1": "k <= 40: k - 1 symbols compared (the last word's mask one byte short)",
    "cmp_round_up4": "k <= 40: compared up to the next multiple of four (the last word not masked; past a buffer's end its padding)",
    "no_tiebreak": "the entry tie-break dropped: a key's list not in insertion order (here: reversed)",
    "n1_empty": "a read of one lookup entry gives nothing (a sort or a search that needs a second element)",
    "rank_sorted": "k > 40: keys ranked by sorted order instead of first insertion",
    "thr_lt": "k > 40: distance < k // 10 instead of <=",
    "score_bit_k": "k > 40: the score bit at 1 << k instead of 1 << (k - 1) (none at k = 64)",
    "rounds_not_carried": "k > 40: within a round the lists in lane order, every round written from the start of j's slot",
    "one_lane_round": "k > 40: a last round of one lane is not run (D mod 64 == 1)",
    "restart_j0": "k > 40: every launch of the edit pass starts at allele k-mer 0 again",
    "stale_isfirst": "k > 40: first-entry marks of an earlier, larger pair of the call at the same k still count as keys",
    "off2_even": "off2 rounded down to even (the 4-bit plane read by bytes)",
}


def _exact_mutant(s1, s2, k, inversions, how):
    kk = -(-k // 4) * 4 if how == "cmp_round_up4" else k - 1 if how == "cmp_k_minus_1" else k
    b1, b2 = s1.translate(model._FOLD), s2.translate(model._FOLD)
    r1 = "".join(model._INV[c] for c in reversed(b1)) if inversions else ""

    def key(buf, pos, tag):
        t = buf[pos:pos + kk]
        return t + chr(tag) * (kk - len(t))
    table = {}
    for i in range(len(b1) - k + 1):
        table.setdefault(key(b1, i, 1), []).append(i)
        if inversions:
            table.setdefault(key(r1, len(b1) - k - i, 2), []).append(i)
    out = []
    for j in range(len(b2) - k + 1):
        lst = table.get(key(b2, j, 3), ())
        out += [(j, i) for i in (reversed(lst) if how == "no_tiebreak" else lst)]
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def _rounds_not_carried(lists, match):
    out = []
    for j in range(match.shape[1]):
        rs = np.flatnonzero(match[:, j])
        if not len(rs):
            continue
        slot = [(-1, -1)] * sum(len(lists[r]) for r in rs)
        for r0 in sorted({int(r) // 64 for r in rs}):
            at = 0
            for r in rs[(rs >= 64 * r0) & (rs < 64 * r0 + 64)]:
                for i in lists[r]:
                    slot[at] = (j, i)
                    at += 1
        out += slot
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def mutant_hits(pair, how, earlier=()):
    """The pair's dots under mutant `how`, or None where the mutant says what the right statement says by construction.
    earlier: the pairs before it in its call (stale_isfirst alone looks at them)."""
    if pair.refused or pair.n == 0:
        return None
    k, inv = pair.k, not pair.forward
    if how == "off2_even":
        if pair.off2 % 2 == 0:
            return None
        return model.kmerhits_array(pair.s1, pair.s2[pair.off2 - 1:], k, inv)
    if how == "n1_empty":
        return np.zeros((0, 2), dtype=np.int32) if pair.n == 1 else None
    if k <= 40:
        return _exact_mutant(pair.s1, pair.allele, k, inv, how) if how in ("cmp_k_minus_1", "cmp_round_up4", "no_tiebreak") else None
    names, lists, dist = pair.keys()
    t = k // 10
    match = dist <= t
    D = len(names)
    if how == "no_tiebreak":
        return model.dots_of([x[::-1] for x in lists], match)
    if how == "thr_lt":
        return model.dots_of(lists, dist < t)
    if how == "rank_sorted":
        order = sorted(range(D), key=lambda r: comparator_key(names[r]))
        return model.dots_of([lists[r] for r in order], match[order])
    if how == "score_bit_k":
        if pair.nk2 == 0:
            return None
        q = model._rows([pair.allele[j:j + k].translate(model._FOLD) for j in range(pair.nk2)], k)
        return model.dots_of(lists, model.lev_matrix(model._rows(names, k), q, bit=k) <= t)
    if how == "rounds_not_carried":
        return _rounds_not_carried(lists, match) if D > 64 else None
    if how == "one_lane_round":
        return model.dots_of(lists[:-1], match[:-1]) if D % 64 == 1 else None
    if how == "restart_j0":
        per = pair.per
        if pair.nk2 <= per:
            return None
        return np.concatenate([model.dots_of(lists, match[:, :min(per, pair.nk2 - j0)]) for j0 in range(0, pair.nk2, per)])
    if how == "stale_isfirst":
        prev = [p for p in earlier if p.k == k and p.k > 40 and not p.refused and p.n > pair.n and p.forward == pair.forward]
        if not prev or pair.nk2 == 0:
            return None
        p = prev[-1]
        stale = [(s, lst) for s, lst in zip(p.keys()[0], p.keys()[1]) if (lst[0] if p.forward else 2 * lst[0]) >= pair.n and s not in names]
        if not stale:
            return None
        q = model._rows([pair.allele[j:j + k].translate(model._FOLD) for j in range(pair.nk2)], k)
        extra = model.lev_matrix(model._rows([s for s, _l in stale], k), q)
        return model.dots_of(lists + [lst for _s, lst in stale], np.concatenate([match, extra <= t]))
    return None


def kills(group, how):
    """The first design of the group on which mutant `how` differs from the right statement, or None."""
    pairs = GROUPS[group]()
    for t, p in enumerate(pairs):
        got = mutant_hits(p, how, pairs[:t])
        if got is not None and not np.array_equal(got, p.hits()):
            return p.name
    return None
