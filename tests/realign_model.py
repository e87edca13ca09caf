"""The rule of `--realign`, stated once more in plain Python integers.  TEST INFRASTRUCTURE: no numpy, nothing of
vapor_amd.realign and no kernel; written from the rule's text, so that what the kernel and the Python statement compute can be
compared with something that is neither.

    distance(read, allele, off2, band)   the full matrix D, the band as an existence test on every cell
    vote(diff)                           'ALT', 'REF' or None
    genotype(alt, ref)                   (GT, GQ) of two counts, the (alt, ref) rule written out

`mutant` changes one rule each (MUTANTS); tests/test_realign_cpu.py shows that the designed cases below tell every one of them
from the rule.  The designed cases are what tests/test_gpu_realign.py holds vapor_realign_batch to."""
import math
import random

MARGIN = 10
ERR = 0.05
MUTANTS = ("band_strict", "n_matches_n", "case_sensitive", "end_corner", "end_last_row", "off2_ignored", "vote_strict")
BANDS = (1, 2, 31, 32, 33, 100, 256, 512)
LENGTHS = (0, 1, 2, 63, 64, 65, 300)
OFFSETS = (0, 1, 7, 8, 9, 31, 32, 33)
IUPAC = "NRYSWKMBDHV"


def code(byte):
    """The symbol code of a byte as the 4-bit plane holds it: ACGT 0..3, acgt 4..7, N and IUPAC 8, their lower case 9, else 15."""
    ch = chr(byte)
    if ch in "ACGT":
        return "ACGT".index(ch)
    if ch in "acgt":
        return 4 + "acgt".index(ch)
    if ch in IUPAC:
        return 8
    if ch in IUPAC.lower():
        return 9
    return 15


def matches(x, y, mutant=None):
    if mutant == "n_matches_n" and x in (8, 9) and y in (8, 9):
        return True
    if x >= 8 or y >= 8:
        return False
    if mutant == "case_sensitive":
        return x == y
    return (x & 3) == (y & 3)


def distance(read, allele, off2, band, mutant=None):
    a = [code(v) for v in bytes(read)]
    b = [code(v) for v in bytes(allele)[0 if mutant == "off2_ignored" else off2:]]
    n, m = len(a), len(b)

    def exists(i, j):
        if not (0 <= i <= n and 0 <= j <= m):
            return False
        return abs(i - j) < band if mutant == "band_strict" else abs(i - j) <= band
    D = [[None] * (m + 1) for _ in range(n + 1)]              # None: the cell does not exist
    D[0][0] = 0
    for i in range(0, n + 1):
        for j in range(0, m + 1):
            if (i, j) == (0, 0) or not exists(i, j):
                continue
            best = None
            if i > 0 and j > 0 and D[i - 1][j - 1] is not None:
                best = D[i - 1][j - 1] + (0 if matches(a[i - 1], b[j - 1], mutant) else 1)
            if i > 0 and D[i - 1][j] is not None and (best is None or D[i - 1][j] + 1 < best):
                best = D[i - 1][j] + 1
            if j > 0 and D[i][j - 1] is not None and (best is None or D[i][j - 1] + 1 < best):
                best = D[i][j - 1] + 1
            D[i][j] = best
    row = [v for v in D[n] if v is not None]
    col = [D[i][m] for i in range(n + 1) if D[i][m] is not None]
    if mutant == "end_corner":
        ends = [D[n][m]] if D[n][m] is not None else []
    elif mutant == "end_last_row":
        ends = row
    else:
        ends = row + col
    return min(ends) if ends else None


def vote(diff, mutant=None):
    if mutant == "vote_strict":
        return "ALT" if diff > MARGIN else "REF" if diff < -MARGIN else None
    return "ALT" if diff >= MARGIN else "REF" if diff <= -MARGIN else None


def genotype(alt, ref):
    """The likeliest of 0/0, 0/1 and 1/1 for `alt` reads of the alt allele and `ref` of the reference at an error rate of 0.05,
    ties to fewer alt alleles, and ten times the log10 ratio to the second, floored, at most 99; (None, None) without a read."""
    if alt + ref == 0:
        return None, None
    ls = [alt * math.log10(ERR) + ref * math.log10(1 - ERR), (alt + ref) * math.log10(0.5), alt * math.log10(1 - ERR) + ref * math.log10(ERR)]
    best = 0
    for g in (1, 2):
        if ls[g] > ls[best]:
            best = g
    second = max(ls[g] for g in range(3) if g != best)
    return ("0/0", "0/1", "1/1")[best], min(99, int(math.floor(10 * (ls[best] - second))))


def columns(diffs, mutant=None):
    """The seven VaPoR_RA_* columns of a locus whose reads have these diffs."""
    vs = [vote(d, mutant) for d in diffs]
    alt, ref = vs.count("ALT"), vs.count("REF")
    gt, gq = genotype(alt, ref)
    return [str(alt), str(ref), str(len(vs) - alt - ref), "%.3f" % (alt / (alt + ref)) if alt + ref else ".", gt or ".",
            "." if gq is None else str(gq), ",".join(str(d) for d in diffs) if diffs else "."]


VOTE_CASES = (MARGIN, -MARGIN, MARGIN - 1, 1 - MARGIN, MARGIN + 1, -MARGIN - 1, 0)


def _dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _other(rng, base):
    return rng.choice([v for v in b"ACGT" if v != base])


def _with_subs(rng, seq, k):
    s = bytearray(seq)
    for p in rng.sample(range(len(s)), min(k, len(s))):
        s[p] = _other(rng, s[p])
    return bytes(s)


_cases = None


def designed_cases():
    """[(name, read, allele, off2, band)]: the designed pairs of the issue, from fixed seeds."""
    global _cases
    if _cases is not None:
        return _cases
    rng = random.Random(20230)
    out = []
    base = _dna(rng, 400)
    # lengths crossed with bands: lane-ownership edges (2B + 1 = 63, 65, 67), one lane, every lane, 17 slots a lane
    for n in LENGTHS:
        for m in LENGTHS:
            for band in BANDS:
                out.append(("len n=%d m=%d B=%d" % (n, m, band), _with_subs(rng, base[:n], 3), base[:m], 0, band))
    # off2 at nibble, word and chunk edges of the 4-bit plane, off2 == len(seq2) among them
    for off2 in OFFSETS:
        for band in (2, 33, 256):
            allele = _dna(rng, off2) + base[:70]
            out.append(("off2=%d B=%d" % (off2, band), _with_subs(rng, base[:70], 2), allele, off2, band))
        out.append(("off2=%d == len(seq2)" % off2, base[:9], _dna(rng, off2), off2, 32))
    # identical sequences; one substitution at the first and at the last symbol
    for band in (1, 32, 100):
        s = base[:130]
        out.append(("identical B=%d" % band, s, s, 0, band))
        out.append(("first symbol B=%d" % band, bytes([_other(rng, s[0])]) + s[1:], s, 0, band))
        out.append(("last symbol B=%d" % band, s[:-1] + bytes([_other(rng, s[-1])]), s, 0, band))
    # one insertion or deletion of exactly B (bridged at cost B) and of B + 1 (not bridged)
    # (the event is a run of T between flanks without a T, the right flank longer than the event: ending early in the run
    # costs a mismatch a symbol, so crossing the run - B steps along the band's edge - is the cheapest path while it exists)
    for band in BANDS:
        left, right = bytes(rng.choice(b"ACG") for _ in range(8)), bytes(rng.choice(b"ACG") for _ in range(band + 20))
        for extra in (band, band + 1):
            mid = b"T" * extra
            out.append(("insertion of %d B=%d" % (extra, band), left + mid + right, left + right, 0, band))
            out.append(("deletion of %d B=%d" % (extra, band), left + right, left + mid + right, 0, band))
    # |n - m| > B both ways: the end lies on the last column only, or on the last row only
    for band in (1, 31, 100):
        s = _dna(rng, 2 * band + 150)
        out.append(("n - m > B, B=%d" % band, s, _with_subs(rng, s[:40], 1), 0, band))
        out.append(("m - n > B, B=%d" % band, _with_subs(rng, s[:40], 1), s, 0, band))
    # symbols: N against N, IUPAC codes, lower against upper case, a byte outside the alphabet
    out.append(("N against N", b"ACGTNNNNACGTACGT", b"ACGTNNNNACGTACGT", 0, 32))
    out.append(("IUPAC", b"ACGTRYSWKMBDHVACGT", b"ACGTRYSWKMBDHVACGT", 0, 32))
    out.append(("lower IUPAC and n", b"ACGTrynACGT", b"ACGTrynACGT", 0, 2))
    out.append(("lower against upper", b"acgtacgtACGTacgt", b"ACGTACGTacgtACGT", 0, 32))
    out.append(("mixed case with substitutions", base[:90].lower(), _with_subs(rng, base[:90], 4), 0, 33))
    out.append(("a byte outside the alphabet", b"ACGTAC*TACGT-ACGT", b"ACGTAC*TACGT-ACGT", 0, 32))
    out.append(("X against X", b"XXXXXXXX", b"XXXXXXXX", 0, 2))
    _cases = out
    return out


_expected = None


def designed_expected():
    """distance() of every designed case, computed once per process."""
    global _expected
    if _expected is None:
        _expected = [distance(r, a, o, b) for _name, r, a, o, b in designed_cases()]
    return _expected


# the bands on both sides of every step of the compiled lane widths 1, 2, 3, 5, 9, 17: ceil((2 B + 1) / 64) slots a lane
EDGE_BANDS = (31, 32, 63, 64, 95, 96, 159, 160, 287, 288, 512)
EDGE_WIDTHS = (1, 2, 2, 3, 3, 5, 5, 9, 9, 17, 17)


def edge_band_cases():
    """[(name, read, allele, off2, band)] at every EDGE_BANDS: the insertion and the deletion of B and of B + 1 of designed_cases()
    (every slot of the band carries a live cell), and one pair with a few substitutions behind off2 = 5."""
    rng = random.Random(20231)
    out = []
    for band in EDGE_BANDS:
        left, right = bytes(rng.choice(b"ACG") for _ in range(8)), bytes(rng.choice(b"ACG") for _ in range(band + 20))
        for extra in (band, band + 1):
            mid = b"T" * extra
            out.append(("insertion of %d B=%d" % (extra, band), left + mid + right, left + right, 0, band))
            out.append(("deletion of %d B=%d" % (extra, band), left + right, left + mid + right, 0, band))
        s = _dna(rng, band + 40)
        out.append(("substitutions off2=5 B=%d" % band, _with_subs(rng, s, 4), _dna(rng, 5) + s, 5, band))
    return out


def planted(rng, n, subs, indels, max_indel=6):
    """(read, allele): an allele of n random bases and a read made of it with planted substitutions and short indels."""
    allele = _dna(rng, n)
    read = bytearray(_with_subs(rng, allele, subs))
    for _ in range(indels):
        p = rng.randrange(len(read) + 1)
        k = rng.randint(1, max_indel)
        if rng.random() < 0.5:
            read[p:p] = _dna(rng, k)
        else:
            del read[p:p + k]
    return bytes(read), allele


def fuzz_cases(seed=77, count=60, max_len=300):
    rng = random.Random(seed)
    out = []
    for t in range(count):
        n = rng.randint(1, max_len - 20)
        read, allele = planted(rng, n, rng.randint(0, 8), rng.randint(0, 4))
        off2 = rng.choice((0, 0, 3, 8, 17))
        allele = _dna(rng, off2) + allele
        out.append(("fuzz %d" % t, read[:max_len], allele[:max_len], off2, rng.choice(BANDS)))
    return out
