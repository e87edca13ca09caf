"""The rule of `--realign-junction`, stated once more in plain Python integers.  TEST INFRASTRUCTURE: no numpy,
nothing of vapor_amd.junction and no kernel; written from the rule's text, so that what the kernels and the Python statement
compute can be compared with something that is neither.

    row_table(s, l, band)          [(f, jf)] of rows 0 .. ns: the full matrix D, the band as an existence test on every cell
    junction(s, l, band)           ((cost, i, j1, j2, f_F(i), f_R(ns - i)), rows)
    lens(allele, window, band)     (cost, left, right, glen, type)
    locus(called, polished, window, band)   the six columns, or None where cost0 != 0

`mutant` changes one rule each (MUTANTS); tests/test_junction_cpu.py shows that the designed cases below tell every one of them
from the rule at least three times.  The designed pairs are what tests/test_gpu_junction.py holds vapor_realign_junction to."""
import random

from realign_model import code

MUTANTS = ("largest_j", "rightmost_row", "validity_dropped", "r_read_at_i", "backward_run_forward", "band_strict", "n_matches_n",
           "equal_lengths_other_way", "gate_dropped")
BANDS = (1, 2, 31, 32, 33, 100, 256, 512)
LENGTHS = (0, 1, 2, 63, 64, 65, 300)
TYPES = ("NONE", "DEL", "INS")


def matches(x, y, mutant=None):
    if mutant == "n_matches_n" and x in (8, 9) and y in (8, 9):
        return True
    if x >= 8 or y >= 8:
        return False
    return (x & 3) == (y & 3)


def row_table(s, l, band, mutant=None):
    """[(f(i), jf(i))] for i = 0 .. ns.  D is held row by row over every column 0 .. nl; None is a cell that does not exist."""
    a, b = [code(v) for v in bytes(s)], [code(v) for v in bytes(l)]
    ns, nl = len(a), len(b)
    assert ns <= nl

    def exists(i, j):
        return abs(i - j) < band if mutant == "band_strict" else abs(i - j) <= band
    out = []
    above = None
    for i in range(ns + 1):
        row = [None] * (nl + 1)
        for j in range(max(0, i - band), min(nl, i + band) + 1):        # (no cell outside these columns exists under either test)
            if not exists(i, j):
                continue
            if i == 0 and j == 0:
                row[0] = 0
                continue
            best = None
            if i > 0 and j > 0 and above[j - 1] is not None:
                best = above[j - 1] + (0 if matches(a[i - 1], b[j - 1], mutant) else 1)
            if i > 0 and above[j] is not None and (best is None or above[j] + 1 < best):
                best = above[j] + 1
            if j > 0 and row[j - 1] is not None and (best is None or row[j - 1] + 1 < best):
                best = row[j - 1] + 1
            row[j] = best
        cells = [(v, j) for j, v in enumerate(row) if v is not None]
        f = min(v for v, _j in cells)
        js = [j for v, j in cells if v == f]
        out.append((f, max(js) if mutant == "largest_j" else min(js)))
        above = row
    return out


def junction(s, l, band, mutant=None):
    """((cost, i, j1, j2, f_F(i), f_R(ns - i)), rows): rows[i] = (f_F(i), jf_F(i), f_R(i), jf_R(i)), each pass by its own row."""
    s, l = bytes(s), bytes(l)
    ns, nl = len(s), len(l)
    F = row_table(s, l, band, mutant)
    R = F if mutant == "backward_run_forward" else row_table(s[::-1], l[::-1], band, mutant)
    best = None
    for i in range(ns + 1):
        r = R[i] if mutant == "r_read_at_i" else R[ns - i]
        j1, j2, cost = F[i][1], nl - r[1], F[i][0] + r[0]
        if j2 < j1 and mutant != "validity_dropped":
            continue
        if best is None or cost < best[0] or (mutant == "rightmost_row" and cost == best[0]):
            best = (cost, i, j1, j2, F[i][0], r[0])
    return best, [F[i] + R[i] for i in range(ns + 1)]


def lens(allele, window, band, mutant=None):
    """(cost, left, right, glen, type): left and right in window coordinates."""
    a, w = bytes(allele), bytes(window)
    deletion = len(a) < len(w) if mutant == "equal_lengths_other_way" else len(a) <= len(w)
    if deletion:
        (cost, _i, j1, j2, _f, _r), _rows = junction(a, w, band, mutant)
        return cost, j1, j2, j2 - j1, "DEL" if j2 > j1 else "NONE"
    (cost, i, j1, j2, _f, _r), _rows = junction(w, a, band, mutant)
    return cost, i, i, j2 - j1, "INS" if j2 > j1 else "NONE"


def locus(called, polished, window, band, mutant=None):
    """The six columns JT, JLEN, JLEN0, JDL, JDR, JCOST of a locus whose polish applies, as text; None where the call's own
    allele is not exactly one jump of its window."""
    cost0, left0, right0, glen0, _t0 = lens(called, window, band, mutant)
    if cost0 != 0 and mutant != "gate_dropped":
        return None
    cost, left, right, glen, kind = lens(polished, window, band, mutant)
    return [kind, str(glen), str(glen0), str(left - left0), str(right - right0), str(cost)]


# ------------------------------------------------------------------------------------------------------------------------------
# the designed cases
# ------------------------------------------------------------------------------------------------------------------------------
def _dna(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(letters) for _ in range(n))


def _other(rng, base):
    return rng.choice([v for v in b"ACGT" if v != base])


def _with_subs(rng, seq, k):
    s = bytearray(seq)
    for p in rng.sample(range(len(s)), min(k, len(s))):
        s[p] = _other(rng, s[p])
    return bytes(s)


_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _rc(seq):
    return bytes(seq).translate(_RC)[::-1]


def _validity_pairs(want=8):
    """Short pairs over two letters on which the validity test decides: the junction with the test dropped is another one.
    Found by a seeded search over pairs of up to 14 symbols at band 3, the smallest first."""
    rng = random.Random(5)
    found, seen = [], set()
    while len(found) < want:
        nl = rng.randint(2, 14)
        ns = rng.randint(1, nl)
        s, l = _dna(rng, ns, b"AC"), _dna(rng, nl, b"AC")
        if (s, l) in seen:
            continue
        seen.add((s, l))
        if junction(s, l, 3)[0] != junction(s, l, 3, "validity_dropped")[0]:
            found.append((s, l))
    return found


_pairs = None


def designed_pairs():
    """[(name, s, l, band)] with len(s) <= len(l): the designed pairs of the issue, from fixed seeds.  tests/test_gpu_junction.py
    runs every one of them at every band of BANDS as well; `band` is the one the case was designed at."""
    global _pairs
    if _pairs is not None:
        return _pairs
    rng = random.Random(4260)
    out = []
    base = _dna(rng, 400)
    # ns of 0, 1, 2, 63, 64, 65 and 300 against a longer sequence with a planted jump, and against itself (ns == nl)
    for ns in LENGTHS:
        s = base[:ns]
        cut = ns // 3
        out.append(("ns=%d, 7 planted" % ns, s, s[:cut] + _dna(rng, 7) + s[cut:], 32))
        out.append(("ns=%d == nl, identical" % ns, s, s, 33))
        if ns:
            out.append(("ns=%d == nl, substitutions" % ns, _with_subs(rng, s, 2), s, 2))
    # a planted jump of 1, B, B + 1, 2B, 2B + 1 and 1 000 symbols: the two passes' bands overlap iff the jump is at most 2B
    # (the insertion form of the same event is the same pair: `lens` orders it; the locus cases below take both forms)
    for band in (1, 2, 31, 32, 33, 100):
        left, right = _dna(rng, 23), _dna(rng, 29)
        for jump in (1, band, band + 1, 2 * band, 2 * band + 1, 1000):
            out.append(("jump of %d B=%d" % (jump, band), left + right, left + _dna(rng, jump) + right, band))
    for band, jump in ((256, 256), (256, 513), (512, 1024), (512, 1025)):
        left, right = _dna(rng, 40), _dna(rng, 37)
        out.append(("jump of %d B=%d" % (jump, band), left + right, left + _dna(rng, jump) + right, band))
    # microhomology of 0, 1 and 5 at the jump: the jump's first h symbols repeat behind it, so h + 1 rows cost the same
    for h in (0, 1, 5):
        left, right = b"ACCA" * 5, b"GTTG" * 6
        hom = b"TAGCA"[:h]
        mid = hom + b"CC" + _dna(rng, 9) + b"GG"
        out.append(("microhomology of %d" % h, left + hom + right, left + mid + hom + right, 32))
        out.append(("microhomology of %d B=2" % h, left + hom + right, left + mid + hom + right, 2))
    # a jump at row 0 and at row ns
    s = base[100:160]
    out.append(("jump at row 0", s, _dna(rng, 12) + s, 32))
    out.append(("jump at row ns", s, s + _dna(rng, 12), 32))
    out.append(("jump at row 0 beyond 2B", s, _dna(rng, 80) + s, 31))
    out.append(("jump at row ns beyond 2B", s, s + _dna(rng, 80), 31))
    # a residual substitution, insertion or deletion beside the jump
    left, right, mid = base[200:240], base[240:290], _dna(rng, 30)
    l = left + mid + right
    out.append(("substitution left of the jump", _with_subs(rng, left, 1) + right, l, 32))
    out.append(("substitution right of the jump", left + _with_subs(rng, right, 1), l, 32))
    out.append(("insertion beside the jump", left[:20] + b"T" + left[20:] + right, l, 32))
    out.append(("deletion beside the jump", left + right[:25] + right[26:], l, 32))
    out.append(("two edits on either side", _with_subs(rng, left, 2) + _with_subs(rng, right, 2), l, 2))
    # N and lower-case symbols: N matches nothing, not even itself; case never matters
    out.append(("N on both sides of the jump", b"ACGTNACGTTGCA", b"ACGTNACGT" + b"GGGGG" + b"TGCA", 32))
    out.append(("N in both, no jump", b"ACNNGTAC", b"ACNNGTAC", 2))
    out.append(("N run at the jump", b"ACGTACNNNNGTCAGT", b"ACGTACNN" + b"CCCCCC" + b"NNGTCAGT", 32))
    out.append(("IUPAC and n", b"ACGTRYnACGTAA", b"ACGTRYn" + b"TTTT" + b"ACGTAA", 33))
    out.append(("lower against upper", left.lower() + right, left + mid.lower() + right.lower(), 32))
    # an inverted segment: no one-jump reading, the cost stays
    seg = base[300:340]
    out.append(("inverted segment", base[290:300] + _rc(seg) + base[340:352], base[290:352], 32))
    out.append(("inverted segment of 12", base[290:300] + _rc(seg[:12]) + base[312:340], base[290:340], 2))
    # short two-letter pairs on which the validity test decides
    for k, (s, l) in enumerate(_validity_pairs()):
        out.append(("validity pair %d" % k, s, l, 3))
    _pairs = out
    return out


_loci = None


def designed_loci():
    """[(name, called, polished, window, band)]: loci whose polish applies, for `lens` and the gate."""
    global _loci
    if _loci is not None:
        return _loci
    rng = random.Random(4261)
    w = _dna(rng, 180)
    ins = _dna(rng, 40)
    out = []
    # exact calls: the polished allele is the called one
    dele = w[:60] + w[110:]
    out.append(("exact DEL", dele, dele, w, 32))
    insa = w[:90] + ins + w[90:]
    out.append(("exact INS", insa, insa, w, 32))
    dup = w[:120] + w[70:120] + w[120:]
    out.append(("exact TANDUP", dup, dup, w, 32))
    # calls that end 5 bases late, start 3 bases early; an insertion 4 bases short
    out.append(("DEL called 5 late", w[:60] + w[115:], dele, w, 32))
    out.append(("DEL called 3 early", w[:57] + w[110:], dele, w, 32))
    out.append(("INS called 4 short", w[:90] + ins[:36] + w[90:], insa, w, 32))
    out.append(("DEL with a residual edit", dele, _with_subs(rng, dele, 1), w, 32))
    # the polished allele as long as the window: a deletion of one base and an insertion of one elsewhere (ns == nl in `lens`)
    for k, (p, q) in enumerate(((20, 100), (75, 30), (140, 141))):
        same = bytearray(w)
        del same[p]
        same.insert(q, _other(rng, same[q]) if same[q] != same[q - 1] else ord("N"))
        out.append(("polished as long as the window %d" % k, w[:p] + w[p + 3:], bytes(same), w, 32))
    # the polished allele turns a called DEL into an insertion-form reading
    out.append(("DEL polished past the window", w[:60] + w[62:], w[:60] + ins + w[60:], w, 33))
    # an INV call, and a window with N outside the jump: the call's own allele is no single jump, the gate says '.'
    for k, (a, b) in enumerate(((50, 90), (20, 150), (100, 112))):
        inv = w[:a] + _rc(w[a:b]) + w[b:]
        out.append(("INV %d" % k, inv, inv, w, 32))
    wn = w[:30] + b"N" + w[31:]
    out.append(("window with N outside the jump", wn[:60] + wn[110:], wn[:60] + wn[110:], wn, 32))
    wj = w[:70] + b"NN" + w[72:]
    out.append(("window with N inside the jump", wj[:60] + wj[110:], wj[:60] + wj[110:], wj, 32))
    _loci = out
    return out


_expected = {}


def expected_pairs(band=None):
    """junction() of every designed pair, at its own band or at `band`; computed once per process and band."""
    if band not in _expected:
        _expected[band] = [junction(s, l, b if band is None else band) for _name, s, l, b in designed_pairs()]
    return _expected[band]


def fuzz_pairs(seed=78, count=60, max_len=260):
    """[(name, s, l, band)]: seeded pairs, l made of s by a planted jump, a few substitutions and short indels."""
    rng = random.Random(seed)
    out = []
    for t in range(count):
        ns = rng.randint(1, max_len)
        s = _dna(rng, ns, b"ACGT" if t % 3 else b"AC")
        l = bytearray(_with_subs(rng, s, rng.randint(0, 4)))
        for _ in range(rng.randint(0, 2)):
            p = rng.randrange(len(l) + 1)
            l[p:p] = _dna(rng, rng.randint(1, 4))
        p = rng.randrange(len(l) + 1)
        l[p:p] = _dna(rng, rng.choice((0, 1, 9, 40, 70, 300)))
        while len(l) < ns:
            l.append(rng.choice(b"ACGT"))
        out.append(("fuzz %d" % t, s, bytes(l), rng.choice(BANDS)))
    return out


def told_apart(mutant):
    """The designed cases on which `mutant` answers differently from the rule: pairs by their junction and rows, loci by columns."""
    n = 0
    for (_name, s, l, band), want in zip(designed_pairs(), expected_pairs()):
        n += junction(s, l, band, mutant) != want
    for _name, called, polished, window, band in designed_loci():
        n += locus(called, polished, window, band, mutant) != locus(called, polished, window, band)
    return n
