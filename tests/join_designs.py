"""Designed pairs for the join (join_kernel / join_verify_t, vapor_amd/csrc/vapor_kernels.h): the smallest shapes at which each of
its data-dependent mechanisms is reached - the bucket-size classes of the packed prefix sums and the queue's fast path, the allele
tiles, the 1024-position read strips and their prefix over a task's reads, the ends of both sequences against the zero padding,
the run records, and k-mers that equal their own reverse complement.

A plain helper module (no pytest hooks).  It holds
  * Pair: (s1, s2, off2, k, flags) with a name, its group and the property it is built for; its expected dots come from anyk_model
    (kmerhits with inversions), its statistics words 0-13 from dot_designs.expected(), its record count from records();
  * the numbers of the kernel that the designs are aimed at, restated (the CPU test reads them out of the headers);
  * pair_mode() (vapor_planner.h, `pair_mode`), bucket() (canon_hash on the 2-bit planes), bucket_classes();
  * the groups buckets(), tiles(), strips() (+ strips_64(), strips_65(), strips_after()), ends(), runs(), strands();
  * MUTANTS and mutant(): deliberately wrong variants of the dots or of the record count, each one way the kernel can be wrong;
  * claims_hold(): whether a pair reaches what its `info` claims (a random pair of the same lengths does not), joined(): the
    planner's filter in front of the tasks, and diff(): the comparison of a device answer with a design, for the GPU test.

bucket() is a restatement that nothing on the device confirms: it only says which class a design reaches and is never compared
with device output.

Coordinates are the project's (j, i): j the position in the allele window (s2[off2:]), i in the read (s1); a = j + off2 is the
absolute allele position, which is what the tiles are cut on."""
from collections import Counter

import numpy as np

import anyk_designs as ad
import anyk_model as model

# ---- restated geometry (vapor_kernels.h: JoinBig, JCHUNK, VAPOR_JQ_FAST_SLACK, VREC_MAX_LEN; vapor_records.h: MAX_READS_PER_TASK)
TA2, TA4 = 24576, 21504
JCHUNK = 1024
QCAP = 256
JQ_FAST_SLACK = 128
MAX_READS_PER_TASK = 64
NB_LOG2 = 15
FILT_LOG2 = 17
VREC_MAX_LEN = 32
FAST_MAX = QCAP - JQ_FAST_SLACK             # the largest candidate total of a position that takes the fast path
KS = (10, 20, 30, 40)
E_KEYERROR = ad.E_KEYERROR

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_ALPHABET = set("ACGTNacgtn")
_rand, _other, revcomp = ad._rand, ad._other, ad.revcomp
_once = ad._once


def n_exc(s):
    """SeqDesc::n_exc: symbols outside upper-case ACGT."""
    return sum(1 for c in s if c not in "ACGT")


def n_invalid(s):
    """SeqDesc::n_invalid: symbols outside invert_base's alphabet after IUPAC folding."""
    return sum(1 for c in s.translate(model._FOLD) if c not in _ALPHABET)


def pair_mode(s1, s2):
    """vapor_planner.h, pair_mode(): 2 plain, 3 the allele has symbols outside upper-case ACGT, 5 the read has, 4 both (4-bit planes)."""
    e1, e2 = n_exc(s1) > 0, n_exc(s2) > 0
    return 4 if e1 and e2 else 3 if e2 else 5 if e1 else 2


class Pair(ad.Pair):
    """A designed pair of the plan route (always with inversions)."""

    def __init__(self, name, group, s1, s2, k, why, off2=0, flags=3, **info):
        ad.Pair.__init__(self, name, group, s1, s2, k, False, why, off2=off2, flags=flags, **info)

    @property
    def nk1(self):
        return max(0, len(self.s1) - self.k + 1)

    @property
    def nk2_all(self):
        """k-mers of the whole allele: what the tiles are cut from."""
        return max(0, len(self.s2) - self.k + 1)

    @property
    def mode(self):
        return pair_mode(self.s1, self.s2)

    @property
    def plane(self):
        return 4 if self.mode == 4 else 2

    @property
    def TA(self):
        return TA4 if self.plane == 4 else TA2

    @property
    def RB(self):
        """Read positions a run never crosses."""
        return 16 if self.plane == 4 and self.k in (30, 40) else VREC_MAX_LEN

    @property
    def forms_runs(self):
        return not (self.plane == 4 and n_invalid(self.s2) > 0)

    @property
    def route(self):
        return {2: "plain", 3: "aexc", 5: "rexc"}.get(self.mode) or ("x4" if self.forms_runs else "x4_noruns")

    def same_strand(self):
        """The same-strand dots (j, i), sorted."""
        if getattr(self, "_same", None) is None:
            if self.refused or self.n == 0:
                self._same = np.zeros((0, 2), dtype=np.int32)
            else:
                self._same = model.kmerhits_array(self.s1, self.allele, self.k, False)
        return self._same


def joined(pair):
    """Whether the pair enters a join task at all - plan_pairs (vapor_planner.h) puts a pair into the order the tasks are cut from
    only when it is not refused and both sequences (the WHOLE allele, not its window from off2 on) have a k-mer.  A read without
    a k-mer therefore never reaches join_kernel through a plan: its pair is answered on the host with zero dots."""
    return pair.refused == 0 and len(pair.s1) - pair.k + 1 > 0 and len(pair.s2) - pair.k + 1 > 0


def _keys(h):
    return h[:, 0].astype(np.int64) * 65536 + h[:, 1].astype(np.int64)


def heads(pair, rb=None, runs=None):
    """The same-strand dots that start a record, as a boolean array over pair.same_strand() - the rule of the kernel's comment
    "Dot records": a run never crosses a 32-aligned read position (RB) nor an allele tile, nor starts before the pair's window,
    so a dot is NOT a head only if i % RB != 0, a % TA != 0, a != off2 and the same-strand dot (a - 1, i - 1) exists."""
    h = pair.same_strand()
    if not (pair.forms_runs if runs is None else runs):
        return np.ones(len(h), dtype=bool)
    rb = rb or pair.RB
    a = h[:, 0].astype(np.int64) + pair.off2
    i = h[:, 1].astype(np.int64)
    pred = np.isin(_keys(h) - 65537, _keys(h))
    return ~((i % rb != 0) & (a % pair.TA != 0) & (a != pair.off2) & pred)


def records(pair, rb=None, runs=None):
    """Run records the join writes for the pair: every reverse-complement dot, and every same-strand dot that is a head."""
    n_rc = len(pair.hits()) - len(pair.same_strand())
    return int(n_rc + heads(pair, rb, runs).sum())


# ---------------------------------------------------------------------------------------------------------------------
# canon_hash, restated (2-bit planes)
# ---------------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def _key(s):
    v = 0
    for t, ch in enumerate(s):
        v |= _CODE[ch] << (2 * t)
    return v


def hash_of_key(c, k):
    """canon_hash of the canonical key c (symbol t in bits 2t .. 2t + 1; words of 32 bits, the lowest first)."""
    if k == 10:
        return (c * 0xC2B2AF) & M32                                  # __umul24: one word of at most 24 bits
    nw = (2 * k + 31) // 32
    x = ((c & M32) * 0x9E3779B1) & M32
    for t, mul in zip(range(1, nw), (0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F, 0x165667B1)):
        x ^= (((c >> (32 * t)) & M32) * mul) & M32
    x ^= x >> 15
    return (x * 0x2C1B3C6D) & M32


def hashes(seq, k):
    """canon_hash of every k-mer of an upper-case ACGT string (the key and its reverse complement slide by one symbol)."""
    out = []
    top = 2 * (k - 1)
    mask = (1 << (2 * k)) - 1
    f = r = 0
    for t, ch in enumerate(seq):
        c = _CODE[ch]
        f = (f >> 2) | (c << top)
        r = ((r << 2) & mask) | (c ^ 3)
        if t >= k - 1:
            out.append(hash_of_key(min(f, r), k))
    return out


def bucket(kmer):
    """join_kernel's bucket of a k-mer of 10, 20, 30 or 40 upper-case bases: the top NB_LOG2 bits of canon_hash."""
    k = len(kmer)
    assert k in KS
    return hash_of_key(min(_key(kmer), _key(revcomp(kmer))), k) >> (32 - NB_LOG2)


def _filter_bits(hx):
    fb = hx >> (32 - FILT_LOG2)
    return fb >> 5, (1 << (fb & 31)) | (1 << ((hx >> 10) & 31))                  # filt_mask()


def bucket_classes(pair):
    """Per allele tile, read strip and group of four positions (t = 4 g .. 4 g + 3 of every lane's sixteen): (tile start, strip
    start, g, the largest bucket size any lane meets in the group, the four candidate totals over the wave, the distinct sizes
    met).  A position counts when it lies inside the read and both of its filter bits are set.  Plain pairs only (mode 2)."""
    assert pair.mode == 2
    k = pair.k
    hr = hashes(pair.s1, k)
    ha = _once(("join_hashes", pair.s2, k), lambda: hashes(pair.s2, k))
    out = []
    for ts in range(0, len(ha), TA2):
        size = Counter()
        filt = {}
        for hx in ha[ts:ts + TA2]:
            size[hx >> (32 - NB_LOG2)] += 1
            w, m = _filter_bits(hx)
            filt[w] = filt.get(w, 0) | m
        for cb in range(0, len(hr), JCHUNK):
            for g in range(4):
                met, tots = set(), []
                for x in range(4):
                    tot = 0
                    for i in range(cb + 4 * g + x, min(cb + JCHUNK, len(hr)), 16):
                        w, m = _filter_bits(hr[i])
                        if filt.get(w, 0) & m == m:
                            c = size.get(hr[i] >> (32 - NB_LOG2), 0)
                            tot += c
                            met.add(c)
                    tots.append(tot)
                met.discard(0)
                out.append((ts, cb, g, max(met, default=0), tuple(tots), frozenset(met)))
    return out


def reaches(pair, sizes=(), totals=(), mixed=()):
    """Whether the pair reaches its bucket classes: the largest bucket any position meets is max(sizes) and every size of `sizes`
    is the largest of some group of four positions; the largest candidate total of a position is max(totals) and every total of
    `totals` occurs; one group of four positions meets all sizes of `mixed` and nothing larger."""
    cl = bucket_classes(pair)
    big = [c[3] for c in cl]
    tots = [t for c in cl for t in c[4]]
    return ((not sizes or (max(big) == max(sizes) and set(sizes) <= set(big))) and
            (not totals or (max(tots) == max(totals) and set(totals) <= set(tots))) and
            (not mixed or any(set(mixed) <= c[5] and c[3] == max(mixed) for c in cl)))


# ---------------------------------------------------------------------------------------------------------------------
# routes: the same two sequences on every plane and mode
# ---------------------------------------------------------------------------------------------------------------------
ROUTES = ("plain", "aexc", "rexc", "x4", "x4_noruns")
_TAIL1 = {"plain": "", "aexc": "", "rexc": "Gn", "x4": "Gn", "x4_noruns": "Gn"}
_TAIL2 = {"plain": "", "aexc": "Cacgtn", "rexc": "", "x4": "Cacgtn", "x4_noruns": "CaXgt"}
_HEAD1 = {"plain": "", "aexc": "", "rexc": "nC", "x4": "nC", "x4_noruns": "nC"}
_HEAD2 = {"plain": "", "aexc": "ntcaG", "rexc": "", "x4": "ntcaG", "x4_noruns": "tXaG"}


def on_route(route, s1, s2):
    """(s1, s2) with tails that put the pair on the route and leave every position as it was."""
    return s1 + _TAIL1[route], s2 + _TAIL2[route]


# ---------------------------------------------------------------------------------------------------------------------
# buckets
# ---------------------------------------------------------------------------------------------------------------------
BUCKET_M = (1, 2, 3, 4, 5, 127, 128, 129, 511, 512, 513)
BUCKET_N = (1, 32, 64)
THRESHOLD_M = (3, 4, 511, 512)
MAX_DOTS = 200000


def unit_kmers(m, n, k):
    """k-mers of the unit of multiplicity m that n lanes hold: 16 (k + 15 bases) up to m = 5, and for every m in one lane below
    k = 40; else one group of four positions (k + 3 bases) from 127 on - 513 units of 55 bases are more than a tile holds at
    k = 40, and in 32 or 64 lanes sixteen positions of 127 and more are half a million dots per design and k - and one position
    where 511 and more meet 32 or 64 lanes (tens of thousands of candidates at that one position as it is)."""
    if m <= 5 or (n == 1 and k < 40):
        return 16
    return 4 if m < 511 or n == 1 else 1


def _unit(rng, k, w):
    """(u, U): a period of 16 bases and the w k-mers of its cycle from rotation 0 on (k + w - 1 bases)."""
    while True:
        u = _rand(rng, 16)
        cyc = u * (2 + (k + 16) // 16)
        if len({cyc[t:t + k] for t in range(16)}) == 16 and len({bucket(cyc[t:t + k]) for t in range(16)}) == 16:
            return u, cyc[:k + w - 1], cyc


def _spacer(rng, cyc, U, n):
    """n random bases (n >= 2) that break the match on both sides of a unit: the first is not what follows U in the cycle, the last
    not what precedes it."""
    s = list(_rand(rng, n))
    s[0] = _other(cyc[len(U)])
    s[-1] = _other(cyc[15])
    return "".join(s)


def _unit_allele(rng, k, units):
    """units: (cyc, U, m).  m copies of every U between spacers."""
    parts = [_rand(rng, 20) + "G"]
    for cyc, U, m in units:
        gap = 2 if m >= 127 else 7            # (many copies: two fixed bases, so that the junctions are few distinct k-mers and no bucket mates)
        for _ in range(m):
            parts += [_spacer(rng, cyc, U, gap), U]
        parts.append(_spacer(rng, cyc, U, 7))
    return "".join(parts) + _rand(rng, 20)


def _lane_read(rng, k, lanes):
    """A read of one strip (1024 + k - 1 bases): lanes = [(first lane, number of lanes, u)] holds the period u over those lanes'
    positions (and the k - 1 bases after them), random bases elsewhere."""
    s = list(_rand(rng, JCHUNK + k - 1))
    for b0, n, u in lanes:
        fill = (u * (n + 1 + k // 16))[:16 * n + k - 1]
        s[16 * b0:16 * b0 + len(fill)] = fill
        if b0:
            s[16 * b0 - 1] = _other(u[15], _other(u[15]))         # (not the base the allele's spacers end with)
        e = 16 * b0 + len(fill)
        if e < len(s):
            s[e] = _other(fill[len(fill) - 16], _other(fill[len(fill) - 16]))
    return "".join(s)


def _both_cases(name, group, s1, s2, k, why, **kw):
    """The pair, and the same sequences in lower case on both sides (the 4-bit planes; no bucket class is claimed there)."""
    info = dict(kw)
    low = {x: v for x, v in info.items() if x in ("off2", "flags", "m", "lanes")}
    return [Pair(name, group, s1, s2, k, why, **info), Pair(name + "_x4", group, s1.lower(), s2.lower(), k, why + " (4-bit planes)", **low)]


def buckets():
    """Every k-mer of a unit U has multiplicity m in the allele (m copies of U between spacers that break any longer match) and
    the read holds U's period in n whole lanes of one strip, so that at U's positions every one of those lanes meets a bucket of
    m entries and the wave's candidate total is n m.  U has 16 k-mers (k + 15 bases) where that fits a tile and keeps the design
    small, else 4 or 1 (unit_kmers).  k = 10 and 40 in full,
    k = 20 and 30 at m = 3, 4, 511, 512.  Then one read that meets sizes 3, 4 and 512 in the same group of four positions, and
    one whose totals are 128 in its first strip and 129 in its second, with sizes 4 and 5."""
    def make():
        rng = np.random.default_rng(7001)
        out = []

        def settled(name, k, why, build, **claims):
            """The first draw of the random bases around the units at which the pair reaches exactly what it claims (a chance
            bucket mate of a unit's k-mer, or a random read k-mer that passes the filter, would add to a size or a total)."""
            for _ in range(200):
                s1, s2 = build()
                if len(s2) - k + 1 <= TA2 and reaches(Pair(name, "buckets", s1, s2, k, why), **claims):
                    return s1, s2
            raise AssertionError("no draw of %s reaches %s" % (name, claims))

        for k in KS:
            for m in (BUCKET_M if k in (10, 40) else THRESHOLD_M):
                for n in (BUCKET_N if k in (10, 40) else (1,)):
                    w = unit_kmers(m, n, k)
                    assert n * w * m < MAX_DOTS
                    fixed = {"tries": 0}
                    name, why = "k%d_m%d_n%d" % (k, m, n), "buckets of %d in %d lanes" % (m, n)

                    def build():
                        if fixed["tries"] % 8 == 0:                      # (a new unit and allele now and then: a chance bucket mate stays)
                            fixed["unit"] = _unit(rng, k, w)
                            fixed["s2"] = _unit_allele(rng, k, [(fixed["unit"][2], fixed["unit"][1], m)])
                        fixed["tries"] += 1
                        return _lane_read(rng, k, [((64 - n) // 2, n, fixed["unit"][0])]), fixed["s2"]
                    s1, s2 = settled(name, k, why, build, sizes=[m], totals=[n * m])
                    out += _both_cases(name, "buckets", s1, s2, k, why, m=m, lanes=n, sizes=[m], totals=[n * m], flags=7 if m <= 2 else 3)
            if k in (10, 40):
                def mixed():
                    us = [_unit(rng, k, 4) for _ in range(3)]
                    return (_lane_read(rng, k, [(5, 2, us[0][0]), (20, 3, us[1][0]), (40, 1, us[2][0])]),
                            _unit_allele(rng, k, [(c, U, m) for (u, U, c), m in zip(us, (3, 4, 512))]))
                name, why = "k%d_mixed_3_4_512" % k, "sizes 3, 4 and 512 in one group of four positions"
                claims = dict(mixed=(3, 4, 512), sizes=[512], totals=[2 * 3 + 3 * 4 + 512])
                s1, s2 = settled(name, k, why, mixed, **claims)
                out += _both_cases(name, "buckets", s1, s2, k, why, **claims)

                def two_strips():
                    u4, u5 = _unit(rng, k, 16), _unit(rng, k, 16)
                    a = _lane_read(rng, k, [(16, 32, u4[0])])
                    b = _lane_read(rng, k, [(3, 31, u4[0]), (40, 1, u5[0])])
                    return a[:JCHUNK - 1] + _other(a[JCHUNK - 1], b[0]) + b, _unit_allele(rng, k, [(u4[2], u4[1], 4), (u5[2], u5[1], 5)])
                name, why = "k%d_total_128_129" % k, "totals of 128 and of 129 from sizes 4 and 5"
                claims = dict(sizes=[5], totals=[FAST_MAX, FAST_MAX + 1])
                s1, s2 = settled(name, k, why, two_strips, **claims)
                out += _both_cases(name, "buckets", s1, s2, k, why, **claims)
        return out
    return _once("join_buckets", make)


# ---------------------------------------------------------------------------------------------------------------------
# tiles
# ---------------------------------------------------------------------------------------------------------------------
def _soft(s, a, n):
    return s[:a] + s[a:a + n].lower() + s[a + n:]


def tiles():
    """Per plane (TA = TA2 or TA4): alleles of exactly TA, TA + 1 and 2 TA + 1 k-mers; reads that are copies of
    allele[TA - 200 : TA + 200 + k] and of the allele's last 300 bases; off2 = 0, TA - 1, TA, TA + 1, 2 TA and one that leaves
    fewer than k bases.  k = 10 in full (and 30 on the 4-bit planes, where runs are cut at 16); the other k at 2 TA + 1 k-mers
    with off2 = 0 and TA.  The 4-bit alleles carry a lower-case stretch across the tile edge, and so do the reads cut from it.
    Last: an allele that is poly-A over a whole tile against a read with 12 A between other bases - one bucket of 24 576
    entries."""
    def make():
        rng = np.random.default_rng(7002)
        out = []
        for plane, TA in ((2, TA2), (4, TA4)):
            base = _rand(rng, 2 * TA + 1 + 39)
            if plane == 4:
                base = _soft(_soft(base, TA - 60, 100), 2 * TA - 30, 69)
            for k in KS:
                full = k == 10 or (plane == 4 and k == 30)
                for nk2, tag in ((TA, "TA"), (TA + 1, "TA+1"), (2 * TA + 1, "2TA+1")):
                    if not full and nk2 != 2 * TA + 1:
                        continue
                    s2 = base[:nk2 + k - 1]
                    edge = base[TA - 200:TA + 200 + k]
                    last = s2[-300:]
                    offs = (0, TA - 1, TA, TA + 1, 2 * TA, len(s2) - k + 1) if full else (0, TA)
                    for off2 in offs:
                        if off2 > len(s2):
                            continue
                        for rname, s1 in (("edge", edge), ("last", last)):
                            dots_a = [a for a in ((TA - 1, TA) if rname == "edge" else (nk2 - 1,)) if off2 <= a < nk2]
                            out.append(Pair("p%d_k%d_%s_off%d_%s" % (plane, k, tag, off2, rname), "tiles", s1, s2, k,
                                            "%d k-mers, off2 = %d" % (nk2, off2), off2=off2, nk2_all=nk2, plane=plane, dots_a=dots_a,
                                            flags=7 if off2 == 0 else 3))
        k = 10
        s2 = _rand(rng, 30) + "C" + "A" * (TA2 + k - 1) + "G" + _rand(rng, 200)
        s1 = _rand(rng, 150) + "C" + "A" * 12 + "G" + _rand(rng, 150)
        out.append(Pair("polyA_tile", "tiles", s1, s2[31:], k, "one bucket of a whole tile", nk2_all=len(s2) - 31 - k + 1, plane=2,
                        sizes=[TA2], dots_a=[0, TA2 - 1], n_dots_min=3 * TA2))
        return out
    return _once("join_tiles", make)


# ---------------------------------------------------------------------------------------------------------------------
# strips
# ---------------------------------------------------------------------------------------------------------------------
STRIP_NK1 = (0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 2049)
STRIP_K = (10, 40)


def _strip_reads(allele, k):
    """(nk1 or -1 for the single base, read): the zero-strip reads first, in the middle and last."""
    def cut(nk1, at):
        return nk1, allele[at:at + nk1 + k - 1]
    return [cut(0, 11), cut(1, 40), cut(2, 77), cut(15, 130), (-1, allele[5]), cut(16, 300), cut(17, 411), cut(0, 500), cut(1023, 600),
            cut(1024, 701), cut(1025, 802), cut(2049, 903), cut(0, 2000)]


def _strip_pairs(group, allele, k, n, tag="", in_task=None):
    """n reads of the cycle; or, with in_task, as many as it takes for in_task of them to have a k-mer (the planner drops the
    others before it cuts tasks: joined()), and one more without."""
    reads = _strip_reads(allele, k)
    out = []
    t = have = 0
    while (t < n) if in_task is None else (have < in_task):
        nk1, s1 = reads[t % len(reads)]
        out.append(Pair("%sk%d_r%d_nk%d" % (tag, k, t, nk1), group, s1, allele, k, "nk1 = %d" % max(nk1, 0), nk1=max(nk1, 0),
                        flags=7 if t % 5 == 0 else 3))
        have += nk1 > 0
        t += 1
    if in_task is not None:
        out.append(Pair("%sk%d_r%d_nk0" % (tag, k, t), group, reads[0][1], allele, k, "nk1 = 0", nk1=0))
    return out


def _strip_alleles():
    def make():
        rng = np.random.default_rng(7003)
        return _rand(rng, 3000), _rand(rng, 2600)
    return _once("join_strip_alleles", make)


def strips():
    """Reads of 0, 1, 2, 15, 16, 17, 1023, 1024, 1025 and 2049 k-mers (the read without a k-mer with k - 1 bases and with one),
    every one an exact substring of one allele of 3000 bases.  With join_tasks = 1 the nine reads that have a k-mer are one task;
    the four without never enter it (joined()): they hold the host's answer for such a pair - status 0, no dots, no records -
    among pairs that are joined, not the kernel's `strips = 0` branch, which no plan reaches."""
    return _once("join_strips", lambda: [p for k in STRIP_K for p in _strip_pairs("strips", _strip_alleles()[0], k, 13)])


def strips_64():
    """Exactly MAX_READS_PER_TASK reads with a k-mer against one allele at one k (and the reads without one among them): a full task."""
    return _once("join_strips64", lambda: _strip_pairs("strips_64", _strip_alleles()[0], 10, 0, "n64_", in_task=MAX_READS_PER_TASK))


def strips_65():
    """One more: the allele's reads are split over two tasks."""
    return _once("join_strips65", lambda: _strip_pairs("strips_65", _strip_alleles()[0], 10, 0, "n65_", in_task=MAX_READS_PER_TASK + 1))


def strips_after():
    """The same reads after another allele's reads in the same task (join_tasks = 1: two of the other allele's three reads and
    nine of these have a k-mer): the table is rebuilt inside the task and the strip prefix starts again."""
    def make():
        first, other = _strip_alleles()
        pre = [Pair("other_r%d" % t, "strips_after", other[a:a + n], other, 10, "another allele's read", nk1=n - 9)
               for t, (a, n) in enumerate(((100, 9), (200, 1500), (50, 30)))]
        return pre + _strip_pairs("strips_after", first, 10, 13, "after_")
    return _once("join_strips_after", make)


# ---------------------------------------------------------------------------------------------------------------------
# ends
# ---------------------------------------------------------------------------------------------------------------------
END_CASES = ("together", "read_first", "allele_first")


def _end_pair(rng, route, k, case, base):
    """Both sequences end in a run of `base` (plane padding is zero, which reads as A; T is its reverse complement): together,
    the read 28 symbols before the allele, or the allele before the read.  The route's exception symbols stand at the start."""
    core = _rand(rng, 160 + k) + "G"
    t1 = base * (40 if case == "allele_first" else 12)
    t2 = base * (40 if case == "read_first" else 12)
    s1 = _HEAD1[route] + core[60:] + t1
    s2 = _HEAD2[route] + core + t2
    return s1, s2


def ends():
    """For every route and k: read and allele end together in a run of A; the read ends in 12 A where the allele goes on with
    40; the allele ends in 12 A where the read goes on with 40; the same with T.  At k = 40: an N (read) or a lower-case base
    (allele) as the very first and the very last symbol; a read N exactly k, k + 1 and k + 31 symbols after a 32-aligned dot.  And
    an exception symbol on the last position of a strip and on the first of the next."""
    def make():
        rng = np.random.default_rng(7004)
        out = []
        for route in ROUTES:
            for k in KS:
                for case in END_CASES:
                    for base in "AT":
                        s1, s2 = _end_pair(rng, route, k, case, base)
                        out.append(Pair("%s_k%d_%s_%s" % (route, k, case, base), "ends", s1, s2, k, "%s, ends in %s" % (case, base),
                                        route=route, case=case, flags=7 if case == "together" else 3))
        k = 40
        al = _rand(rng, 700)
        seg = al[100:600]
        out.append(Pair("k40_read_N_first_last", "ends", "N" + seg[1:-1] + "N", al, k, "N first and last in the read", route="rexc"))
        out.append(Pair("k40_allele_lower_first_last", "ends", seg, al[0].lower() + al[1:-1] + al[-1].lower(), k,
                        "lower case first and last in the allele", route="aexc"))
        out.append(Pair("k40_allele_ends_lower", "ends", al[-200:], al[:-1] + al[-1].lower(), k, "the allele's last symbol under a read's",
                        route="aexc"))
        r = list(seg)
        spots = (64 + k, 160 + k + 1, 256 + k + 31)
        for q in spots:
            r[q] = "N"
        out.append(Pair("k40_N_after_a_dot", "ends", "".join(r), al, k, "N k, k + 1, k + 31 symbols after a 32-aligned dot", route="rexc",
                        heads_at=[64, 160, 256], dead=[(q - k + 1, q) for q in spots]))
        out.append(Pair("k40_read_refused", "ends", seg[:90] + "X" + seg[91:200], al, k, "a read symbol outside the alphabet: KeyError", route="rexc"))
        out.append(Pair("k40_short_read_with_X", "ends", seg[:20] + "X" + seg[21:39], al, k, "the same without a k-mer: no dots, no error",
                        route="rexc"))
        al = _rand(rng, 2400)
        for k in (10, 40):
            r = list(al[50:50 + 1300])
            r[JCHUNK - 1] = r[JCHUNK] = "N"
            out.append(Pair("k%d_N_across_strips" % k, "ends", "".join(r), al, k, "exception bits on position 1023 and 1024", route="rexc",
                            dead=[(JCHUNK - k, JCHUNK)]))
            a2 = list(al)
            a2[50 + JCHUNK - 1] = a2[50 + JCHUNK - 1].lower()
            a2[50 + JCHUNK] = a2[50 + JCHUNK].lower()
            out.append(Pair("k%d_lower_across_strips" % k, "ends", al[50:50 + 1300], "".join(a2), k, "allele exceptions under a strip edge",
                            route="aexc"))
        return out
    return _once("join_ends", make)


# ---------------------------------------------------------------------------------------------------------------------
# runs
# ---------------------------------------------------------------------------------------------------------------------
def _tile_base(plane):
    def make():
        TA = TA2 if plane == 2 else TA4
        return _rand(np.random.default_rng(7100 + plane), TA + 400)
    return _once(("join_tile_base", plane), make)


def _diag(rng, al, k, at, n_dots, start):
    """A read with `start` foreign bases, then the n_dots k-mers of al from `at` on, then foreign bases again."""
    seg = al[at:at + n_dots + k - 1]
    pre = _rand(rng, start)
    if start:
        pre = pre[:-1] + _other(al[at - 1])
    return pre + seg + _other(al[at + len(seg)]) + _rand(rng, 12)


def runs():
    """Once per route, at k = 10 and 30 (runs of 16 on the 4-bit planes there): one exact diagonal of 100 dots that starts at
    read position 0, 1, RB - 1, RB, RB + 1; diagonals of RB - 1, RB, RB + 1, 2 RB and 2 RB + 1 dots; a diagonal that a tile edge
    cuts; one that off2 cuts; an inverted segment, whose reverse-complement dots stay single records."""
    def make():
        rng = np.random.default_rng(7005)
        out = []
        for route in ROUTES:
            plane = 4 if route.startswith("x4") else 2
            TA = TA4 if plane == 4 else TA2
            for k in (10, 30):
                RB = 16 if plane == 4 and k == 30 else 32
                al = _rand(rng, 600)

                def add(name, s1, s2, why, **kw):
                    a, b = on_route(route, s1, s2)
                    out.append(Pair("%s_k%d_%s" % (route, k, name), "runs", a, b, k, why, route=route, rb=RB, **kw))
                for start in (0, 1, RB - 1, RB, RB + 1):
                    n_heads = 1 + (start + 99) // RB - start // RB
                    add("start%d" % start, _diag(rng, al, k, 200, 100, start), al, "100 dots from read position %d" % start,
                        diag=(200, start, 100), diag_heads=n_heads, flags=7)
                for n in (RB - 1, RB, RB + 1, 2 * RB, 2 * RB + 1):
                    add("len%d" % n, _diag(rng, al, k, 150, n, 5), al, "a diagonal of %d dots" % n, diag=(150, 5, n),
                        diag_heads=1 + (5 + n - 1) // RB)
                big = _tile_base(plane)
                add("tile_edge", _diag(rng, big, k, TA - 20, 50, 3), big, "a diagonal across the tile edge", diag=(TA - 20, 3, 50),
                    diag_heads=2 + (3 + 49) // RB - (1 if (3 + 20) % RB == 0 else 0))
                out.append(Pair("%s_k%d_off2_cut" % (route, k), "runs", *on_route(route, _diag(rng, al, k, 200, 60, 2), al), k=k,
                                why="a diagonal that off2 cuts", off2=225, route=route, rb=RB, diag=(225, 27, 35),
                                diag_heads=1 + (27 + 34) // RB - 27 // RB))
                inv = al[100:160] + revcomp(al[250:310]) + al[400:460]
                add("inverted", inv, al, "an inverted segment", rc_min=60 - k + 1, flags=7)
        return out
    return _once("join_runs", make)


# ---------------------------------------------------------------------------------------------------------------------
# strands
# ---------------------------------------------------------------------------------------------------------------------
def strands():
    """Per k, plain and on the 4-bit planes: a k-mer equal to its own reverse complement (w + revcomp(w)), present once and
    three times in the allele - every such dot comes twice; an allele that holds a read k-mer and its reverse complement five
    bases apart; and a read k-mer that differs from an allele k-mer in exactly one symbol - symbol 0, 15, 16, 31, 32, k - 1 -
    which gives no dot."""
    def make():
        rng = np.random.default_rng(7006)
        out = []
        for k in KS:
            w = _rand(rng, k // 2 - 1) + "G"
            pal = w + revcomp(w)
            assert pal == revcomp(pal)
            rd = _rand(rng, 70) + "A" + pal + "A" + _rand(rng, 70)
            km = rd[20:20 + k]
            variants = []
            for sym in sorted({s for s in (0, 15, 16, 31, 32, k - 1) if s < k}):
                q = rd[120:120 + k] if sym % 2 else rd[3:3 + k]
                variants.append((sym, 120 if sym % 2 else 3, q[:sym] + _other(q[sym]) + q[sym + 1:]))
            for copies in (1, 3):
                parts, at = [_rand(rng, 33)], []
                for _ in range(copies):
                    at.append(sum(len(x) for x in parts) + 1)
                    parts += ["C", pal, "C", _rand(rng, 21)]
                km_at = sum(len(x) for x in parts) + 1
                parts += ["T", km, "GCATG"[:5], revcomp(km), "T", _rand(rng, 17)]
                no = []
                for sym, i, v in variants:
                    no.append((sum(len(x) for x in parts) + 1, i))
                    parts += ["T" if v[0] != "T" else "G", v, _rand(rng, 9)]
                s2 = "".join(parts)
                for x4 in (False, True):
                    a, b = (rd.lower(), s2.lower()) if x4 else (rd, s2)
                    out.append(Pair("k%d_selfrc_x%d%s" % (k, copies, "_x4" if x4 else ""), "strands", a, b, k,
                                    "a self-complementary k-mer %d times" % copies, dup=[(j, 71) for j in at],
                                    both=[(km_at, 20), (km_at + k + 5, 20)], no_dots=no, flags=7))
        return out
    return _once("join_strands", make)


GROUPS = {"buckets": buckets, "tiles": tiles, "strips": strips, "strips_64": strips_64, "strips_65": strips_65,
          "strips_after": strips_after, "ends": ends, "runs": runs, "strands": strands}


# ---------------------------------------------------------------------------------------------------------------------
# mutants: wrong variants of the dots ("hits") or of the record count ("records")
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "pad_dots": ("ends", "hits", "read positions >= nk1 are looked up against the zero padding (vmask not cut at the read's end)"),
    "run_past_end": ("ends", "hits", "a run is not cut at nk1 or tn: it goes on over the padding, or into the symbols after the allele's last k-mer"),
    "pre_off2_later_tile": ("tiles", "hits", "emin taken as off2 instead of off2 - ts: dots with a < off2 kept in a later tile"),
    "tile_tail_lost": ("tiles", "hits", "the last k - 1 positions of a tile lost (the tile copied without its k - 1 symbols of lookahead)"),
    "selfrc_once": ("strands", "hits", "a self-complementary k-mer counted once (same strand and reverse complement not both reported)"),
    "fourth_lost": ("buckets", "hits", "a bucket's entries from the fourth on lost (the loop after the three unconditional stores)"),
    "beyond_128_lost": ("buckets", "hits", "candidates beyond 128 of a position lost (the fast path taken above its slack)"),
    "zero_strip_shift": ("strips", "hits", "a read without a k-mer shifts the pairs after it by one: their dots land on the neighbouring pair "
                         "(the planner drops such a read before the tasks are cut, so on the device this is the host's pair bookkeeping, "
                         "not the kernel's strip prefix, whose zero-strip branch no plan reaches)"),
    "run_through_exception": ("ends", "hits", "a run continued through an exception symbol (the exception bits not consulted for its length)"),
    "partial_lane_lost": ("strips", "hits", "the last partial lane of a strip lost (vmask zero unless all sixteen positions are inside)"),
    "no_head_at_32": ("runs", "records", "no head at a 32-aligned read position (16-aligned on the 4-bit planes at k = 30, 40)"),
    "runs_on_noruns": ("runs", "records", "runs formed on the no-runs mode (merge not switched off for an allele with invalid symbols)"),
}


def _arr(rows):
    a = np.asarray(sorted(rows), dtype=np.int64).reshape(-1, 2)
    return a


def _with_same(pair, same_rows):
    """The pair's reverse-complement dots with another list of same-strand dots."""
    rc = Counter(map(tuple, pair.hits().tolist())) - Counter(map(tuple, pair.same_strand().tolist()))
    return _arr(list(rc.elements()) + [tuple(x) for x in same_rows])


def _continued(pair, s1x, s2x):
    """The same-strand dots when every run goes on as long as the sequences s1x / s2x (what the planes hold beyond the end or
    under an exception symbol) agree, up to the next 32-aligned read position."""
    k = pair.k
    true = set(map(tuple, pair.same_strand().tolist()))
    ext = set(map(tuple, model.kmerhits_array(s1x, s2x[pair.off2:], k, False).tolist()))
    kept = set(true)
    for j, i in sorted(ext):
        if (j, i) not in kept and (j - 1, i - 1) in kept and i % pair.RB != 0:
            kept.add((j, i))
    return kept


def _plane2(s):
    """What the 2-bit plane holds for a sequence: upper case, anything else as A (code 0)."""
    return "".join(c if c in "ACGT" else "A" for c in s.upper())


def mutant(pair, how, group=(), index=0):
    """(kind, value) of the pair under mutant `how` - ("hits", sorted (j, i) rows) or ("records", count) - or None where the
    mutant says what the right statement says by construction."""
    if pair.refused:
        return None
    k = pair.k
    if how == "zero_strip_shift":
        zero = [t for t, p in enumerate(group) if p.nk1 == 0 and p.s2 == pair.s2 and t < index]
        if not zero or index + 1 >= len(group) or pair.nk1 == 0:
            return None
        return "hits", _arr(map(tuple, group[index + 1].hits().tolist()))
    if pair.n == 0 or pair.nk2 == 0:
        return None
    same = pair.same_strand()
    if how == "pad_dots":
        ext = model.kmerhits_array(_plane2(pair.s1) + "A" * (k - 1), _plane2(pair.allele), k, False) if pair.plane == 2 else None
        if ext is None:
            return None
        extra = [tuple(x) for x in ext.tolist() if x[1] >= pair.nk1]
        return "hits", _with_same(pair, [tuple(x) for x in same.tolist()] + extra)
    if how == "run_past_end":
        if not pair.forms_runs or pair.plane != 2:
            return None
        return "hits", _with_same(pair, _continued(pair, pair.s1 + "A" * 31, pair.s2 + "A" * 31))
    if how == "run_through_exception":
        if pair.mode not in (3, 5):
            return None
        return "hits", _with_same(pair, _continued(pair, _plane2(pair.s1), _plane2(pair.s2)))
    if how == "pre_off2_later_tile":
        if pair.off2 <= pair.TA:
            return None
        whole = model.kmerhits_array(pair.s1, pair.s2, k, False)
        extra = [(int(a) - pair.off2, int(i)) for a, i in whole.tolist() if pair.TA <= a < pair.off2 and a // pair.TA == pair.off2 // pair.TA]
        return "hits", _with_same(pair, [tuple(x) for x in same.tolist()] + extra)
    if how == "tile_tail_lost":
        h = pair.hits()
        a = h[:, 0].astype(np.int64) + pair.off2
        return "hits", _arr(map(tuple, h[a % pair.TA <= pair.TA - k].tolist()))
    if how == "selfrc_once":
        return "hits", _arr(set(map(tuple, pair.hits().tolist())))
    if how == "fourth_lost":
        seen = Counter()
        rows = []
        for j, i in same.tolist():
            seen[i] += 1
            if seen[i] <= 3:
                rows.append((j, i))
        return "hits", _with_same(pair, rows)
    if how == "beyond_128_lost":
        seen = Counter()
        rows = []
        for j, i in sorted(same.tolist(), key=lambda x: (x[1], x[0])):
            slot = (i // JCHUNK, i % 16)
            seen[slot] += 1
            if seen[slot] <= FAST_MAX:
                rows.append((j, i))
        return "hits", _with_same(pair, rows)
    if how == "partial_lane_lost":
        h = pair.hits()
        return "hits", _arr(map(tuple, h[h[:, 1] < pair.nk1 // 16 * 16].tolist()))
    if how == "no_head_at_32":
        return ("records", records(pair, rb=1 << 20)) if pair.forms_runs else None
    if how == "runs_on_noruns":
        return ("records", records(pair, runs=True)) if not pair.forms_runs else None
    raise KeyError(how)


def right(pair, kind):
    return _arr(map(tuple, pair.hits().tolist())) if kind == "hits" else records(pair)


def kills(group, how):
    """The first design of the group on which mutant `how` differs from the right answer, or None."""
    pairs = GROUPS[group]()
    for t, p in enumerate(pairs):
        got = mutant(p, how, pairs, t)
        if got is None:
            continue
        kind, value = got
        want = right(p, kind)
        if (not np.array_equal(value, want)) if kind == "hits" else value != want:
            return p.name
    return None


# ---------------------------------------------------------------------------------------------------------------------
# what a design claims, and the comparison with a device answer
# ---------------------------------------------------------------------------------------------------------------------
def claims_hold(pair):
    """Whether the pair has what its info names: route and plane, the k-mer counts, the bucket classes, the planted dots, heads
    and gaps.  Every design must; a random pair of the same lengths does not."""
    f = pair.info
    same = pair.same_strand()
    dots = Counter(map(tuple, pair.hits().tolist()))
    sset = set(map(tuple, same.tolist()))
    on = set(same[:, 1].tolist())
    ok = [f.get("route", pair.route) == pair.route, f.get("plane", pair.plane) == pair.plane, f.get("rb", pair.RB) == pair.RB,
          f.get("nk1", pair.nk1) == pair.nk1, f.get("nk2_all", pair.nk2_all) == pair.nk2_all, len(dots) > 0 or not joined(pair) or pair.nk2 <= 1]
    if pair.group.startswith("strips"):
        ok.append(pair.s1 in pair.s2 and on == set(range(pair.nk1)))
    if pair.mode == 2 and ("sizes" in f or "totals" in f or "mixed" in f):
        ok.append(reaches(pair, f.get("sizes", ()), f.get("totals", ()), f.get("mixed", ())))
    if "m" in f:
        n, w = f["lanes"], unit_kmers(f["m"], f["lanes"], pair.k)
        per_i = np.bincount(same[:, 1], minlength=JCHUNK) if len(same) else np.zeros(JCHUNK, dtype=np.int64)
        ok.append(all(per_i[16 * b + t] == f["m"] for b in range((64 - n) // 2, (64 - n) // 2 + n) for t in range(w)))
    if "dots_a" in f:
        ok.append(set(f["dots_a"]) <= set((same[:, 0].astype(np.int64) + pair.off2).tolist()))
    ok.append(sum(dots.values()) >= f.get("n_dots_min", 0))
    if "case" in f:
        j_end, i_end = pair.nk2 - 1, pair.nk1 - 1
        ok.append({"together": (j_end, i_end), "read_first": (j_end - 28, i_end), "allele_first": (j_end, i_end - 28)}[f["case"]] in sset)
    if "heads_at" in f:
        ok.append(all(h in on and not (set(range(lo, hi + 1)) & on) for h, (lo, hi) in zip(f["heads_at"], f["dead"])))
    elif "dead" in f:
        ok.append(all(lo - 1 in on and hi + 1 in on and not (set(range(lo, hi + 1)) & on) for lo, hi in f["dead"]))
    if "diag" in f:
        a0, i0, n = f["diag"]
        d = (same[:, 0] + pair.off2 - same[:, 1] == a0 - i0) & (same[:, 1] >= i0) & (same[:, 1] < i0 + n)
        ok.append(d.sum() == n and not ({(a0 - pair.off2 - 1, i0 - 1), (a0 - pair.off2 + n, i0 + n)} & sset) and
                  heads(pair)[d].sum() == (f["diag_heads"] if pair.forms_runs else n))
    if "rc_min" in f:
        ok.append(sum(dots.values()) - len(same) >= f["rc_min"])
    if "dup" in f:
        ok.append(all(dots[d] == 2 for d in f["dup"]) and all(dots[d] == 1 for d in f["both"]) and
                  all(dots[(j, i)] == 0 and sum(x != y for x, y in zip(pair.allele[j:j + pair.k], pair.s1[i:i + pair.k])) == 1
                      for j, i in f["no_dots"]))
    return all(bool(x) for x in ok)


def diff(pairs, st, hits, rec=None):
    """The differences between a device answer - statistics rows, dots per pair sorted by (j, i), record counts or None - and
    the designs, one line each."""
    errs = []
    for t, p in enumerate(pairs):
        want, code = p.expected()
        exp = p.hits()
        if not np.array_equal(hits[t], exp):
            m = min(len(exp), len(hits[t]))
            bad = next((q for q in range(m) if tuple(hits[t][q]) != tuple(exp[q])), m)
            errs.append("%s/%s: %d dots for %d, first difference at %d" % (p.group, p.name, len(hits[t]), len(exp), bad))
        if st[t, :14].tolist() != want:
            errs.append("%s/%s: words 0-13 %s for %s" % (p.group, p.name, st[t, :14].tolist(), want))
        if st[t, 15] != code:
            errs.append("%s/%s: status %d for %d" % (p.group, p.name, st[t, 15], code))
        if rec is not None and rec[t] != records(p):
            errs.append("%s/%s (%s): %d records for %d, %d dots" % (p.group, p.name, p.route, rec[t], records(p), len(exp)))
    return errs
