"""A test-local restatement of kmerhits' two match rules (SF:951-983), in numpy, for the any-k tests.

k <= 40: the lookup dict of key_modify'd k-mers (with inversions each followed by its reverse complement), probed by every
allele k-mer in order.  k > 40: every distinct key in first-insertion order whose Levenshtein distance to the allele k-mer is
below k // 10 + 1; the distances come from a bit-parallel recurrence (Myers / Hyyro, global boundary) over all keys at once,
which check_lev_model() holds against the plain dynamic programme.  key_distances() / kmerhits_array() state the k > 40 rule
key-major (the distance is symmetric), which is cheap for a pair of few distinct keys and many allele k-mers."""
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


def _rows(kmers, k):
    return np.frombuffer("".join(kmers).encode("latin-1"), dtype=np.uint8).reshape(len(kmers), k)


def key_distances(seq1, seq2, k, inversions):
    """(keys in first-insertion order, their lists, dist) with dist[r, j] the Levenshtein distance of key r to allele k-mer j:
    key-major - lev_many(key r, all allele k-mers), the distance being symmetric - so that a pair of few distinct keys and
    many allele k-mers costs one recurrence per key."""
    table = lookup(seq1, k, inversions)
    names = list(table)
    nk2 = max(0, len(seq2) - k + 1)
    dist = np.zeros((len(names), nk2), dtype=np.int64)
    if names and nk2:
        q = _rows([seq2[j:j + k].translate(_FOLD) for j in range(nk2)], k)
        if len(names) <= 16:
            for r, name in enumerate(names):
                dist[r] = lev_many(name.encode("latin-1"), q)
        else:
            dist = lev_matrix(_rows(names, k), q)
    return names, [table[s] for s in names], dist


def lev_matrix(keys, queries, bit=None):
    """lev_many for every key at once: dist[r, j] of keys (uint8, (D, k)) to queries (uint8, (Q, k)), the same recurrence with
    the match masks taken from the key (row r of the result is lev_many(keys[r], queries)).  bit: where the score is read, k - 1
    unless a mutant of the statement says otherwise (anyk_designs)."""
    D, k = keys.shape
    Q = queries.shape[0]
    step = max(1, (1 << 15) // max(Q, 1))              # (blocks of keys whose rows stay in the cache)
    if D > step:
        return np.concatenate([lev_matrix(keys[a:a + step], queries, bit) for a in range(0, D, step)])
    peq = np.zeros((D, 256), dtype=np.uint64)
    rows = np.arange(D)
    for p in range(k):
        peq[rows, keys[:, p]] |= np.uint64(1 << p)
    pv = np.full((D, Q), M64, dtype=np.uint64)
    mv = np.zeros((D, Q), dtype=np.uint64)
    up = np.zeros((D, Q), dtype=np.uint64)             # how often the score went up, and down
    down = np.zeros((D, Q), dtype=np.uint64)
    b = k - 1 if bit is None else bit
    hb = np.uint64((1 << b) & M64)
    sh = np.uint64(min(b, 63))
    one = np.uint64(1)
    for c in range(k):
        eq = peq[:, queries[:, c]]
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | ~(xh | pv)
        mh = pv & xh
        up += (ph & hb) >> sh
        down += (mh & hb) >> sh
        ph = (ph << one) | one
        mh = mh << one
        pv = mh | ~(xv | ph)
        mv = ph & xv
    return k + up.astype(np.int64) - down.astype(np.int64)


def kmerhits_array(seq1, seq2, k, inversions):
    """kmerhits as an (n, 2) int32 array of (j, i) rows; at k > 40 from key_distances (j, then key rank, then list position)."""
    if k <= 40:
        return np.asarray(kmerhits(seq1, seq2, k, inversions), dtype=np.int32).reshape(-1, 2)
    _names, lists, dist = key_distances(seq1, seq2, k, inversions)
    return dots_of(lists, dist <= k // 10)


def dots_of(lists, match):
    """The dots of the k > 40 rule from match[r, j] (key r is within the threshold of allele k-mer j)."""
    js, rs = np.nonzero(match.T)                       # (row-major over the transpose: j, then rank)
    if not len(js):
        return np.zeros((0, 2), dtype=np.int32)
    arrs = [np.asarray(x, dtype=np.int32) for x in lists]
    lens = np.asarray([len(x) for x in lists], dtype=np.int64)
    out = np.empty((int(lens[rs].sum()), 2), dtype=np.int32)
    out[:, 0] = np.repeat(js, lens[rs])
    out[:, 1] = np.concatenate([arrs[r] for r in rs])
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
