"""A test-local restatement of kmerhits' two match rules (SF:951-983), in numpy, for the any-k tests.

k <= 40: the lookup dict of key_modify'd k-mers (with inversions each followed by its reverse complement), probed by every
allele k-mer in order.  k > 40: every distinct key in first-insertion order whose Levenshtein distance to the allele k-mer is
below k // 10 + 1; the distances come from a bit-parallel recurrence (Myers / Hyyro, global boundary) over all keys at once,
which check_lev_model() holds against the plain dynamic programme."""
import hashlib

import numpy as np

_FOLD = str.maketrans("RrYySsWwKkMmBbDdHhVv", "NnNnNnNnNnNnNnNnNnNn")
_INV = {"A": "T", "T": "A", "C": "G", "G": "C", "N": "N", "a": "t", "t": "a", "c": "g", "g": "c", "n": "n"}
M64 = (1 << 64) - 1


def lookup(seq1, k, inversions):
    table = {}
    for i in range(len(seq1) - k + 1):
        key = seq1[i:i + k].translate(_FOLD)
        table.setdefault(key, []).append(i)
        if inversions:
            table.setdefault("".join(_INV[c] for c in reversed(key)), []).append(i)     # KeyError as the reference
    return table


def lev_dp(a, b):
    prev = list(range(len(b) + 1))
    for x in range(1, len(a) + 1):
        cur = [x] + [0] * len(b)
        for y in range(1, len(b) + 1):
            cur[y] = min(prev[y] + 1, cur[y - 1] + 1, prev[y - 1] + (a[x - 1] != b[y - 1]))
        prev = cur
    return prev[-1]


def lev_many(q, keys):
    """Levenshtein distances of the k-byte query q to each row of keys (uint8, (n, k)), k <= 64."""
    k = len(q)
    n = keys.shape[0]
    peq = np.zeros(256, dtype=np.uint64)
    for p, c in enumerate(q):
        peq[c] |= np.uint64(1 << p)
    pv = np.full(n, M64, dtype=np.uint64)
    mv = np.zeros(n, dtype=np.uint64)
    score = np.full(n, k, dtype=np.int64)
    hb = np.uint64(1 << (k - 1))
    one = np.uint64(1)
    for c in range(k):
        eq = peq[keys[:, c]]
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | ~(xh | pv)
        mh = pv & xh
        score += (ph & hb != 0).astype(np.int64) - (mh & hb != 0).astype(np.int64)
        ph = (ph << one) | one
        mh = mh << one
        pv = mh | ~(xv | ph)
        mv = ph & xv
    return score


def kmerhits(seq1, seq2, k, inversions):
    table = lookup(seq1, k, inversions)
    out = []
    if len(seq2) < k:
        return out
    if k <= 40:
        for j in range(len(seq2) - k + 1):
            for i in table.get(seq2[j:j + k].translate(_FOLD), ()):
                out.append((j, i))
        return out
    names = list(table)
    if not names:
        return out
    keys = np.frombuffer("".join(names).encode("latin-1"), dtype=np.uint8).reshape(len(names), k)
    lists = [table[s] for s in names]
    t = k // 10
    for j in range(len(seq2) - k + 1):
        q = seq2[j:j + k].translate(_FOLD).encode("latin-1")
        for r in np.flatnonzero(lev_many(q, keys) <= t):
            out.extend((j, i) for i in lists[r])
    return out


def digest(hits):
    return hashlib.sha256(np.asarray(hits, dtype=np.int32).reshape(-1, 2).tobytes()).hexdigest()


def matches(entry, hits):
    """Whether hits equal a golden {"n", "sha", ["hits"]} entry."""
    if len(hits) != entry["n"]:
        return False
    if "hits" in entry:
        return [list(h) for h in hits] == entry["hits"]
    return digest(hits) == entry["sha"]
