"""The rule of `--realign-revote`, stated in plain Python integers.  TEST INFRASTRUCTURE: no numpy, nothing of
vapor_amd and no kernel; the polish is polish_model's (4.25), the distances realign_model's (4.23), the spelling, the mapping of a
read's start, the second vote and its gate are written from the rule's text.

    spell(codes, calls, sites, ins)          (spelt codes, own): own[q] the polished position of column q's own symbol, own[len] = plen
    revote(votes, allele, band, pol)         (lout, vout, spelt, own) of a locus whose polish `pol` is polish_model.polish's five
    eight(d_ref, d_alt, d_pol)               the eight VaPoR_RA2_* columns of a locus from its reads' three distances

`votes` is a list of (read, off2).  `mutant` changes one rule each (MUTANTS): the first six the spelling and the mapping, which
designed_loci() tells from the rule; the last three the columns, which COLUMN_CASES tell.  tests/test_revote_cpu.py shows that
every mutant is told at least three times; tests/test_gpu_revote.py holds vapor_realign_revote to designed_loci() exactly."""
import random

import polish_model as pm
import realign_model as rm

MARGIN, MIN_COV, RMAX, MAX_SITES = rm.MARGIN, pm.MIN_COV, pm.RMAX, pm.MAX_SITES
KEEP, DELETE, SITE_BIT = pm.KEEP, pm.DELETE, pm.SITE_BIT
MAX_SEQ_LEN = 65535
E_ARG = -4
SPELL_MUTANTS = ("text_behind_own", "keep_upper", "delete_emits", "off2_start", "off2_unmapped", "text_by_column")
COLUMN_MUTANTS = ("gain_all_reads", "vote_strict", "no_pn_gate")
MUTANTS = SPELL_MUTANTS + COLUMN_MUTANTS

_BYTE_OF_CODE = b"ACGTacgtNn?????*"


def bytes_of(codes):
    """Bytes whose plane codes (realign_model.code) are `codes`."""
    return bytes(_BYTE_OF_CODE[c] for c in codes)


def spell(codes, calls, sites, ins, mutant=None):
    out, own, k = [], [], 0
    for q, a in enumerate(codes):
        call = calls[q]
        text = []
        if call & SITE_BIT:
            slot = q % len(sites) if mutant == "text_by_column" else k
            text = [b"ACGT".index(v) for v in ins[slot][:sites[slot][1]]]
            k += 1
        call &= 7
        if call == KEEP:
            mine = [a & 3 if mutant == "keep_upper" and 4 <= a < 8 else 8 if mutant == "keep_upper" and a == 9 else a]
        elif call < 4:
            mine = [call]
        else:
            mine = [a] if mutant == "delete_emits" else []
        if mutant == "text_behind_own":
            own.append(len(out))
            out += mine + text
        else:
            out += text
            own.append(len(out))
            out += mine
    own.append(len(out))
    return out, own


_dists = {}


def _distance(read, allele, off2, band):
    key = (bytes(read), bytes(allele), off2, band)
    if key not in _dists:
        _dists[key] = rm.distance(read, allele, off2, band)
    return _dists[key]


def revote(votes, allele, band, pol, mutant=None, want_d=True):
    """pol = (counts, calls, sites, ins, stats) of the locus, status 0.  Without want_d the distances are left out (None): the
    spelling mutants are told by what is spelt and where a read starts."""
    _counts, calls, sites, ins, _stats = pol
    codes = [rm.code(v) for v in bytes(allele)]
    spelt, own = spell(codes, calls, sites, ins, mutant)
    plen = len(spelt)
    if plen > MAX_SEQ_LEN:
        return [E_ARG, plen, 0, 0], [[-1, E_ARG, 0, 0] for _ in votes], spelt, own
    text = bytes_of(spelt)
    vout = []
    for read, off2 in votes:
        if not 0 <= off2 <= len(codes):
            vout.append([-1, E_ARG, 0, 0])
            continue
        if mutant == "off2_unmapped":
            at = min(off2, plen)
        elif mutant == "off2_start":                # (the symbols emitted before the column's inserted text)
            k = sum(1 for q in range(off2) if calls[q] & SITE_BIT)
            at = own[off2] - (sites[k][1] if off2 < len(codes) and calls[off2] & SITE_BIT else 0)
        else:
            at = own[off2]
        vout.append([_distance(read, text, at, band) if want_d else None, 0, at, plen - at])
    return [0, plen, 0, 0], vout, spelt, own


def eight(d_ref, d_alt, d_pol, pn=None, mutant=None):
    """The eight columns of a locus whose every gate but VaPoR_RA_PN >= MIN_COV holds; pn: the reads piled, by default the
    round-1 ALT voters."""
    diff = [r - a for r, a in zip(d_ref, d_alt)]
    piled = [k for k, v in enumerate(diff) if v >= MARGIN]
    if pn is None:
        pn = len(piled)
    if pn < MIN_COV and mutant != "no_pn_gate":
        return ["."] * 8
    diff2 = [r - p for r, p in zip(d_ref, d_pol)]
    gain = sum(d_alt[k] - d_pol[k] for k in (range(len(diff)) if mutant == "gain_all_reads" else piled))
    return rm.columns(diff2, "vote_strict" if mutant == "vote_strict" else None) + [str(gain)]


# (d_ref, d_alt, d_pol) of designed loci for the columns: a polish that lifts a read over the margin, one that lands exactly on it,
# one that costs edits, REF readers the polish moves, fewer than three voters, and nothing at all
COLUMN_CASES = (
    ([40, 41, 39, 12, 0, 1], [25, 26, 24, 5, 30, 29], [20, 21, 19, 2, 32, 29]),
    ([30, 30, 30, 19], [15, 16, 17, 10], [10, 10, 10, 9]),
    ([30, 30, 30, 19], [15, 16, 17, 12], [12, 18, 17, 9]),
    ([50, 50, 50, 50, 3, 4], [10, 10, 10, 45, 30, 30], [10, 10, 10, 40, 20, 14]),
    ([22, 23, 5, 5], [10, 10, 5, 9], [8, 8, 4, 2]),
    ([22, 5, 5], [10, 5, 9], [8, 4, 2]),
    ([21, 22], [5, 5], [4, 4]),
    ([15, 15, 15], [5, 5, 5], [5, 5, 6]),
    ([12, 12, 12, 9], [1, 1, 1, 0], [2, 2, 2, 0]),
    ([], [], []),
)


def _reads_at(rng, truth, own, cols, n_col):
    """Vote reads that start at the allele columns `cols`: 45 symbols of the polished text `truth` from own[q] on, one of them
    substituted - the read a molecule that starts at column q carries."""
    out = []
    for q in cols:
        if 0 <= q <= n_col:
            piece = bytearray(truth[own[q]:own[q] + 45])
            if len(piece) > 6:
                piece[5] = rm._other(rng, piece[5]) if piece[5] in b"ACGT" else piece[5]
            out.append((bytes(piece), q))
    return out


_loci = None


def designed_loci():
    """[(name, pairs, votes, allele, band)]: pairs the piled reads of polish_model's shape, votes the reads of the second
    alignment - the piled reads themselves, and reads that start at column 0, at the first flagged column, at the first deleted
    column and the one behind it, and at len."""
    global _loci
    if _loci is not None:
        return _loci
    rng = random.Random(20270)
    base_loci = [(n, p, a, b) for n, p, a, b in pm.designed_loci() if len(a) <= 300]
    extra = []
    # the polished length at nibble, word and chunk edges: an allele of plen + 1 columns whose reads lack one
    for plen in (7, 8, 9, 31, 32, 33, 63, 64, 65):
        al = rm._dna(rng, plen + 1)
        cut = next(q for q in range(1 + plen // 2, 0, -1) if al[q] != al[q - 1] and (q + 1 > plen or al[q] != al[q + 1]))
        extra.append(("plen %d" % plen, [(al[:cut] + al[cut + 1:], 0)] * 3, al, 31))
        extra.append(("plen %d, nothing called" % plen, [(al[:plen], 0)] * 3, al[:plen], 100))
    # flagged columns at 255, 256 and 257: the rank and the carry cross a round of 256 columns; texts of three lengths
    al = bytes(rng.choice(b"ACG") for _ in range(300))
    for cols in ((255, 256, 257), (256,), (40, 255), (100, 257, 290)):
        rd = bytearray()
        for q, ch in enumerate(al):
            if q in cols:
                rd += b"T" * (1 + cols.index(q))
            rd.append(ch)
        extra.append(("sites before %s" % (cols,), [(bytes(rd), 0)] * 3 + [(al, 0)], al, 100))
    # two and three sites whose texts differ, and a deletion between them
    al = bytes(rng.choice(b"ACG") for _ in range(150))
    for a, b, c in ((40, 90, 120), (21, 64, 65), (10, 128, 140)):
        rd = al[:a] + b"T" + al[a:b - 10] + al[b - 9:b] + b"TTT" + al[b:c] + b"TT" + al[c:]
        extra.append(("sites before %d, %d and %d" % (a, b, c), [(rd, 0)] * 3, al, 100))
        extra.append(("sites before %d, %d and %d, reads behind off2 7" % (a, b, c), [(rd[7:], 7)] * 4, al, 31))
    # every kind of symbol under KEEP: lower case, N, lower-case IUPAC, a byte outside the alphabet
    mixed = bytearray(rm._dna(rng, 120))
    mixed[10:20] = bytes(mixed[10:20]).lower()
    mixed[30], mixed[31], mixed[32], mixed[33] = ord("N"), ord("r"), ord("*"), ord("n")
    planted = pm._plant(rng, bytes(mixed), sub=50, dele=70, ins=(90, b"GAT"))
    for k in (3, 4):
        extra.append(("every kind of symbol, %d reads" % k, [(planted, 0)] * k, bytes(mixed), 100))
    # bands 1, 2, 32 and 33: every compiled width of the re-vote's kernel
    al = rm._dna(rng, 65)
    rd = pm._plant(rng, al, sub=20, dele=40)
    for band in (1, 2, 32, 33):
        extra.append(("B=%d, allele of 65" % band, [(rd, 0)] * 3 + [(al, 0)], al, band))
        extra.append(("B=%d, three clean reads behind off2 3" % band, [(al[3:], 3)] * 3, al, band))
    # fewer than three voters: nothing is called, the allele is spelt as it is
    extra.append(("two voters", [(rd, 0)] * 2, al, 100))
    extra.append(("no voter", [], al, 100))
    out = []
    for name, pairs, allele, band in base_loci + extra:
        _counts, calls, sites, ins, _stats = pol = pm.polish(pairs, allele, band)
        codes = [rm.code(v) for v in bytes(allele)]
        spelt, own = spell(codes, calls, sites, ins)
        truth = bytes_of(spelt)
        n_col = len(allele)
        flagged = [q for q in range(n_col) if calls[q] & SITE_BIT]
        deleted = [q for q in range(n_col) if calls[q] & 7 == DELETE]
        at = [0, n_col] + flagged[:1] + flagged[-1:] + deleted[:1] + [q + 1 for q in deleted[:1]]
        seen, votes = set(), []
        for v in list(pairs) + _reads_at(rng, truth, own, sorted(set(at)), n_col):
            if v not in seen:
                seen.add(v)
                votes.append(v)
        out.append((name, pairs, votes, allele, band))
    # the 1 200-column allele with more than 256 sites: short vote reads, at the start, across round edges and at len
    name, pairs, allele, band = pm.designed_loci()[-1]
    pol = pm.polish(pairs, allele, band)
    spelt, own = spell([rm.code(v) for v in allele], pol[1], pol[2], pol[3])
    out.append((name, pairs, _reads_at(rng, bytes_of(spelt), own, (0, 254, 510, 514, 1026, 1100, 1199, 1200), len(allele)), allele, band))
    _loci = out
    return out


_polished = {}


def polish_of(locus):
    name, pairs, _votes, allele, band = locus
    key = (name, allele, band, len(pairs))
    if key not in _polished:
        _polished[key] = pm.polish(pairs, allele, band)
    return _polished[key]


_expected = None


def designed_expected():
    """[(lout, vout, spelt, own)] of designed_loci(), computed once per process."""
    global _expected
    if _expected is None:
        _expected = [revote(l[2], l[3], l[4], polish_of(l)) for l in designed_loci()]
    return _expected


def _shape(got):
    """What tells a spelling mutant: the locus record, every read's start and length, the spelt codes and own[]."""
    lout, vout, spelt, own = got
    return lout, [v[1:] for v in vout], spelt, own


def told_apart(mutant):
    """In how many designed loci (spelling mutants) or column cases (column mutants) the mutant differs from the rule."""
    if mutant in COLUMN_MUTANTS:
        return sum(1 for c in COLUMN_CASES if eight(*c, mutant=mutant) != eight(*c))
    return sum(1 for l, e in zip(designed_loci(), designed_expected())
               if _shape(revote(l[2], l[3], l[4], polish_of(l), mutant, want_d=False)) != _shape(e))


def fuzz_loci(seed=31, count=40):
    """polish_model's seeded loci, every piled read a vote pair, and three more that start at columns drawn at random."""
    rng = random.Random(seed + 1000)
    out = []
    for name, pairs, allele, band in pm.fuzz_loci(seed, count):
        more = [(rm._with_subs(rng, allele[q:q + 50], 2), q) for q in (rng.randrange(len(allele) + 1) for _ in range(3))]
        out.append((name, pairs, list(dict.fromkeys(list(pairs) + more)), allele, band))
    return out
