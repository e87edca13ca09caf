"""The rule of `--realign-out`, stated in plain Python integers.  TEST INFRASTRUCTURE: no numpy, nothing of
vapor_amd and no kernel; the full matrix D of 4.23 (realign_model's symbols and matches), every cell's existence tested, and the
walk from the end cell back to (0, 0) written from the rule's text.

    trace(read, allele, off2, band)   (d, i_end, j_end, runs, cigar): runs a list of (length, op) in path order, op one of
                                      '=', 'X', 'I', 'D'; cigar the runs as text with the soft clip of n - i_end behind them

`mutant` changes one rule each (MUTANTS); tests/test_trace_cpu.py shows that the designed cases tell every one of them from the
rule at least three times.  designed_cases() is realign_model's list and the pairs below it; tests/test_gpu_trace.py holds
vapor_realign_trace to them run for run."""
import random

import realign_model as rm

MUTANTS = ("end_smallest", "vertical_first", "horizontal_before_vertical", "eq_is_x", "clip_dropped")
OPS = "=XID"


def matrix(a, b, band):
    """D of 4.23 over the symbol codes a and b: None where the cell does not exist."""
    n, m = len(a), len(b)
    D = [[None] * (m + 1) for _ in range(n + 1)]
    D[0][0] = 0
    for i in range(n + 1):
        for j in range(m + 1):
            if (i, j) == (0, 0) or abs(i - j) > band:
                continue
            best = None
            if i > 0 and j > 0 and D[i - 1][j - 1] is not None:
                best = D[i - 1][j - 1] + (0 if rm.matches(a[i - 1], b[j - 1]) else 1)
            if i > 0 and D[i - 1][j] is not None and (best is None or D[i - 1][j] + 1 < best):
                best = D[i - 1][j] + 1
            if j > 0 and D[i][j - 1] is not None and (best is None or D[i][j - 1] + 1 < best):
                best = D[i][j - 1] + 1
            D[i][j] = best
    return D


def trace(read, allele, off2, band, mutant=None, D=None):
    """(`D`: the pair's matrix where the caller has it already - every mutant walks the same one)"""
    a = [rm.code(v) for v in bytes(read)]
    b = [rm.code(v) for v in bytes(allele)[off2:]]
    n, m = len(a), len(b)
    if D is None:
        D = matrix(a, b, band)
    ends = [(n, j) for j in range(m + 1) if D[n][j] is not None] + [(i, m) for i in range(n + 1) if D[i][m] is not None]
    d = min(D[i][j] for i, j in ends)
    ends = [e for e in ends if D[e[0]][e[1]] == d]
    i_end, j_end = min(ends) if mutant == "end_smallest" else max(ends)           # the largest i, among those the largest j
    i, j, path = i_end, j_end, []
    while (i, j) != (0, 0):
        here = D[i][j]
        diag = i > 0 and j > 0 and D[i - 1][j - 1] is not None
        same = diag and rm.matches(a[i - 1], b[j - 1])
        diag = diag and D[i - 1][j - 1] + (0 if same else 1) == here
        vert = i > 0 and D[i - 1][j] is not None and D[i - 1][j] + 1 == here
        hori = j > 0 and D[i][j - 1] is not None and D[i][j - 1] + 1 == here
        if mutant == "vertical_first":
            move = "I" if vert else "d" if diag else "D"
        elif mutant == "horizontal_before_vertical":
            move = "d" if diag else "D" if hori else "I"
        else:
            move = "d" if diag else "I" if vert else "D"
        if move == "d":
            path.append("=" if same or mutant == "eq_is_x" else "X")
            i, j = i - 1, j - 1
        elif move == "I":
            assert vert
            path.append("I")
            i -= 1
        else:
            assert hori
            path.append("D")
            j -= 1
    path.reverse()
    runs = []
    for op in path:
        if runs and runs[-1][1] == op:
            runs[-1] = (runs[-1][0] + 1, op)
        else:
            runs.append((1, op))
    clip = 0 if mutant == "clip_dropped" else n - i_end
    cigar = "".join("%d%s" % r for r in runs) + ("%dS" % clip if clip else "")
    return d, i_end, j_end, runs, cigar or "*"


_own = None


def own_cases():
    """[(name, read, allele, off2, band)]: the pairs 4.24 adds to realign_model.designed_cases()."""
    global _own
    if _own is not None:
        return _own
    rng = random.Random(20240)
    base = rm._dna(rng, 300)
    out = []
    # a read that starts behind the allele's start: a leading D run
    for lead, band in ((1, 1), (5, 32), (12, 33), (30, 32), (20, 256)):
        out.append(("leading D of %d B=%d" % (lead, band), rm._with_subs(rng, base[lead:lead + 200], 2), base, 0, band))
    out.append(("leading D behind off2", base[10:170], rm._dna(rng, 9) + base, 9, 100))
    # nothing to align: n = 0, m = 0 (off2 == len(seq2)), both
    for band in (1, 32, 512):
        out.append(("n = 0 B=%d" % band, b"", base[:50], 0, band))
        out.append(("m = 0 B=%d" % band, base[:50], b"", 0, band))
        out.append(("off2 == len(seq2) B=%d" % band, base[:20], base[:33], 33, band))
    out.append(("n = m = 0", b"", b"", 0, 2))
    # the end on the last column with a long clip: the allele ends far above the read's end, inside and outside the band
    for m, band in ((40, 2), (40, 100), (64, 33), (100, 512)):
        out.append(("long clip m=%d B=%d" % (m, band), rm._with_subs(rng, base[:280], 3), base[:m], 0, band))
    # ties among end cells: on the row (the allele goes on, every further column costs one more ... or nothing more: a read
    # that ends in a symbol the allele repeats), on the column (the read goes on past the allele's end)
    out.append(("row tie, repeated tail", b"ACGTACGTAA", b"ACGTACGTAAAAAAAA", 0, 8))
    out.append(("row tie, substituted tail", b"ACGTACGTAC", b"ACGTACGTAGC", 0, 4))
    out.append(("column tie, repeated tail", b"ACGTACGTAAAAAAAA", b"ACGTACGTAA", 0, 8))
    out.append(("column tie, substituted tail", b"ACGTACGTAGC", b"ACGTACGTAC", 0, 4))
    out.append(("row and column tie at the corner", b"ACGTTGCA", b"ACGTTGCA", 0, 3))
    out.append(("all N: every end cell ties", b"NNNNNN", b"NNNNNN", 0, 3))
    out.append(("all N, read longer", b"NNNNNNNNN", b"NNNN", 0, 6))
    out.append(("all N, allele longer", b"NNNN", b"NNNNNNNNN", 0, 6))
    # only the vertical and the horizontal predecessors tie (the diagonal one is dearer): two symbols swapped, so that the
    # cell behind the swap is reached at the same cost by skipping either one
    for left, band in ((b"", 2), (b"ACCA", 3), (base[:70], 32), (base[:130], 100)):
        out.append(("swap behind %d B=%d" % (len(left), band), left + b"GT" + b"CCAACC", left + b"TG" + b"CCAACC", 0, band))
        out.append(("swap at the end behind %d B=%d" % (len(left), band), left + b"GT", left + b"TG", 0, band))
    out.append(("two swaps", b"AAGTCCCCTGAA", b"AATGCCCCGTAA", 0, 5))
    # ... where the diagonal predecessor ties too, so these tell vertical-first but not horizontal-before-vertical.  Pairs in
    # which a cell of the path has ONLY the vertical and the horizontal predecessor at its cost (found by a search over short
    # strings, kept here as found, and once more behind a common prefix and in wider bands)
    vh = ((b"AGAC", b"GAGCAAG", 2), (b"CACGC", b"ACAGCA", 3), (b"ACAAG", b"CACCGCA", 4), (b"AGAGCGG", b"GAGGC", 2),
          (b"AAGACGC", b"ACACAG", 2), (b"GCGACG", b"CGCCCGA", 2), (b"GCAGCCA", b"AGCCCAG", 3), (b"GCCGCAC", b"CGGCCAC", 4))
    for k, (r, a, band) in enumerate(vh):
        out.append(("vertical and horizontal tie %d" % k, r, a, 0, band))
    for k, (r, a, _band) in enumerate(vh[:4]):
        pre = base[:(3, 64, 129, 200)[k]]
        out.append(("vertical and horizontal tie %d behind %d" % (k, len(pre)), pre + r, pre + a, 0, (33, 100, 256, 512)[k]))
    _own = out
    return out


_cases = None


def designed_cases():
    global _cases
    if _cases is None:
        _cases = list(rm.designed_cases()) + own_cases()
    return _cases


_results = None


def _all():
    """trace() of every designed case under the rule (key None) and under every mutant, one matrix a case, once per process."""
    global _results
    if _results is None:
        _results = {k: [] for k in (None,) + MUTANTS}
        for _name, r, a, o, band in designed_cases():
            D = matrix([rm.code(v) for v in bytes(r)], [rm.code(v) for v in bytes(a)[o:]], band)
            for k in _results:
                _results[k].append(trace(r, a, o, band, k, D))
    return _results


def designed_expected():
    return _all()[None]


def told_apart(mutant):
    """How many designed cases tell `mutant` from the rule."""
    return sum(1 for got, want in zip(_all()[mutant], _all()[None]) if got != want)
