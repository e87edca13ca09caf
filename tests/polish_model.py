"""The rule of `--realign-polish`, stated in plain Python integers.  TEST INFRASTRUCTURE: no numpy, nothing of
vapor_amd and no kernel; the traces are trace_model's (4.24), the pile, the calls, the sites and the inserted text are written
from the rule's text.

    polish(pairs, allele, band)   (counts, calls, sites, ins, stats): counts a list of [A, C, G, T, O, Dl, bcov, ins] per
                                  column; calls a list of call bytes; sites the kept sites as [column, bases]; ins their texts
                                  as bytes; stats [0, pairs, PCOV, PSUB, PDEL, sites kept, PINS, sites dropped]
    text(allele, calls, sites, ins)   the polished allele

`pairs` is a list of (read, off2).  `mutant` changes one rule each (MUTANTS); tests/test_polish_cpu.py shows that the designed
loci tell every one of them from the rule at least three times.  tests/test_gpu_polish.py holds vapor_realign_polish to
designed_loci() counter for counter and byte for byte."""
import random

import realign_model as rm
import trace_model as tm

MIN_COV, RMAX, MAX_SITES = 3, 64, 256
KEEP, DELETE, SITE_BIT = 4, 5, 8
MUTANTS = ("majority_ge", "lead_counted", "site_vs_cov", "edge_ins", "same_base_sub", "min_cov_2", "ins_past_gap", "ins_tie_largest",
           "off2_ignored")

_traces = {}


def trace_of(read, allele, off2, band):
    key = (bytes(read), bytes(allele), off2, band)
    if key not in _traces:
        _traces[key] = tm.trace(read, allele, off2, band)
    return _traces[key]


def polish(pairs, allele, band, mutant=None):
    allele = bytes(allele)
    n_col = len(allele)
    counts = [[0] * 8 for _ in range(n_col)]
    min_cov = 2 if mutant == "min_cov_2" else MIN_COV
    inserted = []                                   # (column, the read codes of the run) of every I run that counts
    for read, off2 in pairs:
        _d, _i_end, j_end, runs, _cigar = trace_of(read, allele, off2, band)
        a = [rm.code(v) for v in bytes(read)]
        shift = 0 if mutant == "off2_ignored" else off2
        lead = runs[0][0] if runs and runs[0][1] == "D" else 0
        if mutant == "lead_counted":
            lead = 0
        first_col, end_col = shift + lead, shift + j_end
        i = j = 0
        for r, (k, op) in enumerate(runs):
            if op == "I":
                q = shift + j
                inside = first_col <= q <= end_col if mutant == "edge_ins" else first_col < q < end_col
                if inside and q < n_col:
                    counts[q][7] += 1
                    inserted.append((q, a[i:i + k]))
                i += k
            elif op == "D" and r == 0 and mutant != "lead_counted":
                j += k
            else:
                for s in range(k):
                    col = shift + j + s
                    if col >= n_col:                # (only a mutant's columns leave the allele)
                        continue
                    if op == "D":
                        counts[col][5] += 1
                    else:
                        c = a[i + s]
                        counts[col][c & 3 if c < 8 else 4] += 1
                    if col != first_col:
                        counts[col][6] += 1
                j += k
                if op != "D":
                    i += k
    b = [rm.code(v) for v in allele]
    calls, sites, stats = [KEEP] * n_col, [], [0, len(pairs), 0, 0, 0, 0, 0, 0]
    for q in range(n_col):
        A, C, G, T, O, Dl, bcov, ins = counts[q]
        cov = A + C + G + T + O + Dl
        if cov >= min_cov:
            stats[2] += 1
            cand = [A, C, G, T, Dl]
            best = max(cand)
            if 2 * best > cov or (mutant == "majority_ge" and 2 * best >= cov):
                w = cand.index(best)
                own = b[q] & 3 if b[q] < 8 else None
                if w == 4:
                    calls[q] = DELETE
                    stats[4] += 1
                elif w != own or mutant == "same_base_sub":
                    calls[q] = w
                    stats[3] += 1
        judge = cov if mutant == "site_vs_cov" else bcov
        if q >= 1 and judge >= min_cov and 2 * ins > judge:
            if len(sites) < MAX_SITES:
                sites.append([q, 0])
                calls[q] |= SITE_BIT
            else:
                stats[7] += 1
    stats[5] = len(sites)
    texts = []
    for site in sites:
        q = site[0]
        bcov = counts[q][6]
        out = bytearray()
        for r in range(RMAX):
            n4 = [0, 0, 0, 0]
            for col, codes in inserted:
                if col == q and r < len(codes) and codes[r] < 8:
                    n4[codes[r] & 3] += 1
            if not 2 * sum(n4) > bcov:
                if mutant == "ins_past_gap":
                    continue
                break
            top = max(n4)
            w = max(k for k in range(4) if n4[k] == top) if mutant == "ins_tie_largest" else n4.index(top)
            out.append(b"ACGT"[w])
        site[1] = len(out)
        stats[6] += len(out)
        texts.append(bytes(out))
    return counts, calls, sites, texts, stats


def text(allele, calls, sites, ins):
    out, slot = bytearray(), 0
    for q, ch in enumerate(bytes(allele)):
        if calls[q] & SITE_BIT:
            out += ins[slot]
            slot += 1
        call = calls[q] & 7
        if call == KEEP:
            out.append(ch)
        elif call < 4:
            out.append(b"ACGT"[call])
    return bytes(out)


def _plant(rng, allele, sub=None, dele=None, ins=None):
    """A read of `allele` with a substitution at `sub`, the symbol at `dele` left out and `ins` = (column, bases) put in."""
    out = bytearray()
    for q, ch in enumerate(bytes(allele)):
        if ins is not None and q == ins[0]:
            out += ins[1]
        if q == dele:
            continue
        out.append(rm._other(rng, ch) if q == sub else ch)
    return bytes(out)


_loci = None


def designed_loci():
    """[(name, pairs, allele, band)], pairs a list of (read, off2)."""
    global _loci
    if _loci is not None:
        return _loci
    rng = random.Random(20250)
    out = []
    base = rm._dna(rng, 150)
    planted = _plant(rng, base, sub=30, dele=70, ins=(110, b"GAT"))
    # k identical reads: MIN_COV
    for k in range(6):
        out.append(("%d identical planted reads" % k, [(planted, 0)] * k, base, 100))
    # the strict majority: k planted among clean ones
    for k, tot in ((2, 4), (3, 5), (1, 3), (2, 3), (2, 5), (3, 6), (4, 6)):
        out.append(("%d planted of %d" % (k, tot), [(planted, 0)] * k + [(base, 0)] * (tot - k), base, 100))
    # different off2: lead, bcov and the coverage edges differ per pair
    shifted = [(planted[12:], 10), (planted[25:140], 20), (planted[5:], 0), (planted, 0), (planted[40:120], 37)]
    out.append(("reads with different off2", shifted, base, 100))
    out.append(("reads with different off2, band 31", shifted, base, 31))
    for lead in (1, 7, 29):
        out.append(("three reads that start %d behind the start" % lead, [(planted[lead:], 0)] * 3 + [(planted, 0)], base, 100))
        out.append(("off2 %d and a lead" % lead, [(planted[lead + 3:], lead)] * 4, base, 31))
    # an insertion at a read's first covered column and at its end
    head = b"TTG" + base[20:120]
    tail = base[50:] + b"CCA"                    # (behind the allele's end: the end cell leaves such symbols to the clip)
    out.append(("insertion before the first covered column", [(head, 20)] * 4, base, 31))
    out.append(("insertion behind the last covered column", [(tail, 50)] * 4, base, 31))
    out.append(("insertions at both edges among inner ones", [(head, 20)] * 3 + [(tail, 50)] * 3 + [(planted, 0)] * 3, base, 100))
    # an allele N under a base majority, a read N under an allele base, lower case kept
    with_n = bytearray(base)
    with_n[40], with_n[41], with_n[90] = ord("N"), ord("r"), ord("n")
    lower = bytes(with_n[:50]) + bytes(with_n[50:100]).lower() + bytes(with_n[100:])
    read_n = bytearray(base)
    read_n[60] = ord("N")
    for k in (2, 3, 4):
        out.append(("allele N, %d reads" % k, [(base, 0)] * k, bytes(with_n), 100))
        out.append(("read N, %d reads of 5" % k, [(bytes(read_n), 0)] * k + [(base, 0)] * (5 - k), base, 100))
        out.append(("lower-case allele, %d planted reads" % k, [(planted, 0)] * k, lower, 100))
    # planted insertions of 1, 63, 64 and 65 bases
    wide = rm._dna(rng, 300)                     # (enough allele behind the stretch that inserting it is the cheapest path)
    for n_ins in (1, 63, 64, 65):
        stretch = rm._dna(rng, n_ins)
        long_read = _plant(rng, wide, ins=(75, stretch))
        for band in (100, 256):
            out.append(("insertion of %d B=%d" % (n_ins, band), [(long_read, 0)] * 3 + [(wide, 0)], wide, band))
    # the tie and the majority at once: two reads insert A, two insert C, one inserts nothing
    at = next(q for q in range(40, 100) if base[q - 1] in b"GT" and base[q] in b"GT")      # (no neighbour an inserted A or C could slide along)
    ra, rc = _plant(rng, base, ins=(at, b"A")), _plant(rng, base, ins=(at, b"C"))
    out.append(("two A and two C of five", [(ra, 0)] * 2 + [(rc, 0)] * 2 + [(base, 0)], base, 100))
    out.append(("two C and two A of five", [(rc, 0)] * 2 + [(ra, 0)] * 2 + [(base, 0)], base, 100))
    rt, rg = _plant(rng, base, ins=(50, b"TG")), _plant(rng, base, ins=(50, b"GG"))
    out.append(("two TG and two GG of four", [(rt, 0)] * 2 + [(rg, 0)] * 2, base, 100))
    out.append(("two TG, one GG and one A of five", [(rt, 0)] * 2 + [(rg, 0), (ra, 0), (base, 0)], base, 100))
    # an inserted stretch that half of the reads carry on with: the text stops where no majority inserts
    r5, r2 = _plant(rng, base, ins=(50, b"ACGTA")), _plant(rng, base, ins=(50, b"AC"))
    out.append(("a stretch of 5 in two of four, of 2 in the others", [(r5, 0)] * 2 + [(r2, 0)] * 2, base, 100))
    rn = _plant(rng, base, ins=(50, b"ANGT"))
    out.append(("an N inside the inserted stretch", [(rn, 0)] * 3 + [(r5, 0)], base, 100))
    out.append(("an N inside two of four stretches", [(rn, 0)] * 2 + [(_plant(rng, base, ins=(50, b"ACGT")), 0)] * 2, base, 100))
    for seq in (b"ANGT", b"ANNGT", b"CNT"):
        rs = _plant(rng, base, ins=(90, seq))
        out.append(("every read inserts %s" % seq.decode(), [(rs, 0)] * (3 + len(seq) % 3), base, 100))
    for col in (20, 45, 100, 130):
        rs, rw = _plant(rng, base, ins=(col, b"ANGT")), _plant(rng, base, ins=(col, b"CTNNA"))
        out.append(("ANGT before column %d" % col, [(rs, 0)] * 3, base, 100))
        out.append(("CTNNA before column %d, and a clean read" % col, [(rw, 0)] * 3 + [(base, 0)], base, 31))
    for x, y, tot in ((b"G", b"T", 4), (b"T", b"G", 5), (b"CA", b"CC", 4), (b"C", b"A", 4)):
        rx, ry = _plant(rng, base, ins=(33, x)), _plant(rng, base, ins=(33, y))
        out.append(("two %s and two %s of %d" % (x.decode(), y.decode(), tot), [(rx, 0)] * 2 + [(ry, 0)] * 2 + [(base, 0)] * (tot - 4), base, 31))
    # the strict majority once more, in a narrow band
    for k, tot in ((2, 4), (3, 6), (4, 8)):
        out.append(("%d planted of %d B=31" % (k, tot), [(planted, 0)] * k + [(base, 0)] * (tot - k), base, 31))
    # a site is judged against bcov, not cov: reads whose first covered column is the site's add to cov alone
    for n_ins, n_full, n_start in ((3, 0, 3), (2, 1, 1), (2, 0, 1), (2, 0, 2), (3, 1, 2)):
        pile = [(ra, 0)] * n_ins + [(base, 0)] * n_full + [(base[at:], at)] * n_start
        out.append(("%d insert, %d pass, %d start at the site" % (n_ins, n_full, n_start), pile, base, 100))
    # an insertion at the edge of the coverage is no insertion, whatever the band and the pile
    for band in (100, 256):
        out.append(("edge insertions B=%d" % band, [(head, 20)] * 3 + [(tail, 50)] * 2, base, band))
        out.append(("edge insertions among clean reads B=%d" % band, [(head, 20)] * 4 + [(base, 0)] * 2 + [(tail, 50)] * 3, base, band))
    # edges of the 64-column step: alleles of 1, 63, 64, 65 and 300 columns, '=' runs of exactly 64 and 65
    for n_col in (1, 63, 64, 65, 300):
        al = rm._dna(rng, n_col)
        out.append(("allele of %d, three clean reads" % n_col, [(al, 0)] * 3, al, 31))
        if n_col > 1:
            rd = _plant(rng, al, sub=n_col - 1, dele=n_col // 2)
            out.append(("allele of %d, a substitution in the last column" % n_col, [(rd, 0)] * 3 + [(al, 0)], al, 100))
    al = rm._dna(rng, 200)
    for run in (64, 65):
        rd = _plant(rng, al, sub=run)
        out.append(("an = run of %d" % run, [(rd, 0)] * 3, al, 100))
        out.append(("an = run of %d behind off2 3" % run, [(rd[3:], 3)] * 3, al, 100))
    # more than MAX_SITES sites: a T planted every fourth column between symbols that are no T
    wide = bytes(rng.choice(b"ACG") for _ in range(1200))
    many = bytearray()
    for q, ch in enumerate(wide):
        if q % 4 == 2 and 8 <= q:
            many += b"T"
        many.append(ch)
    out.append(("more than 256 sites", [(bytes(many), 0)] * 3, wide, 512))
    _loci = out
    return out


_results = None


def _all():
    global _results
    if _results is None:
        _results = {k: [polish(p, a, band, k) for _name, p, a, band in designed_loci()] for k in (None,) + MUTANTS}
    return _results


def designed_expected():
    return _all()[None]


def told_apart(mutant):
    return sum(1 for got, want in zip(_all()[mutant], _all()[None]) if got != want)


def fuzz_loci(seed=31, count=40):
    """Seeded loci of 3 to 8 noisy reads each, with their own off2."""
    rng = random.Random(seed)
    out = []
    for t in range(count):
        n_col = rng.randint(40, 220)
        allele = rm._dna(rng, n_col)
        truth = _plant(rng, allele, sub=rng.randrange(n_col), dele=rng.randrange(n_col),
                       ins=(rng.randrange(1, n_col), rm._dna(rng, rng.randint(1, 9))))
        pairs = []
        for _ in range(rng.randint(3, 8)):
            off2 = rng.choice((0, 0, 3, 8, 17))
            src = truth if rng.random() < 0.7 else allele
            lo = min(len(src) - 1, off2 + rng.choice((0, 0, 2, 5)))
            hi = rng.randint(max(lo + 1, len(src) - 30), len(src))
            noisy = bytearray(rm._with_subs(rng, src[lo:hi], rng.randint(0, 3)))
            if rng.random() < 0.4 and len(noisy) > 4:
                del noisy[rng.randrange(len(noisy))]
            if rng.random() < 0.4:
                noisy.insert(rng.randrange(len(noisy) + 1), rng.choice(b"ACGTN"))
            pairs.append((bytes(noisy), off2))
        out.append(("fuzz %d" % t, pairs, allele, rng.choice((31, 100, 256))))
    return out
