"""Executors for the driver generators (vapor_amd.drivers): turn their Window / Score requests
into batches for the HIP library and feed the results back.

`run_sync`  - one locus at a time (what the reference does);
`run_batch` - many loci in lockstep: all pending requests of a round become ONE sequence set
              and ONE plan on the device (reads that share an allele window share its hash table).
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from . import repeat_qc
from .drivers import Figure, Realign, Score, ScoreGrid, Window

import threading

_engine = None
_engine_lock = threading.RLock()      # made at import: the chunk threads of cli.score_jobs reach engine_slot() together


def get_engine():
    """Process-wide default engine on the current device (LOCAL_RANK or 0)."""
    global _engine
    with _engine_lock:
        if _engine is None:
            from .dist import _device_ordinal
            from .engine import Engine
            _engine = Engine(_device_ordinal())
        return _engine


def set_engine(e) -> None:
    global _engine, _more_engines
    _engine = e
    _more_engines = []


_more_engines: list = []


def get_engines(n: int) -> list:
    """`n` engines on the current device, the default one first: one per thread that scores chunks (a library context serves
    one host thread).  An engine that is not this package's own (the tests' stand-in) is shared: it has no such rule."""
    first = get_engine()
    from .engine import Engine
    if not isinstance(first, Engine):
        return [first] * n
    from .dist import _device_ordinal
    while len(_more_engines) < n - 1:
        _more_engines.append(Engine(_device_ordinal()))
    return [first] + _more_engines[:n - 1]


def engine_slot(k: int):
    """The engine of the k-th thread that scores chunks, made on that thread's first call (the second context of a run comes
    up while the first chunk is already being prepared on the first): get_engines(k + 1)[k]."""
    first = get_engine()
    from .engine import Engine
    if k == 0 or not isinstance(first, Engine):
        return first
    with _engine_lock:
        if len(_more_engines) >= k:
            return _more_engines[k - 1]
    from .dist import _device_ordinal
    made = Engine(_device_ordinal())                   # (outside the lock: the other threads' first calls go on)
    with _engine_lock:
        while len(_more_engines) < k - 1:              # (slots are taken in order; a gap is filled by whoever comes)
            _more_engines.append(Engine(_device_ordinal()))
        if len(_more_engines) >= k:                    # another thread was faster
            made.close()
            return _more_engines[k - 1]
        _more_engines.append(made)
        return made


class _SeqTable:
    """Deduplicating builder of the sequence list of one device batch."""

    def __init__(self):
        self.seqs: List[str] = []
        self.upper: List[bool] = []
        self._idx: Dict[Tuple[str, bool], int] = {}

    def add(self, s: str, upper: bool = False) -> int:
        key = (s, upper)
        i = self._idx.get(key)
        if i is None:
            i = len(self.seqs)
            self._idx[key] = i
            self.seqs.append(s)
            self.upper.append(upper)
        return i


def _raise_for_status(st_row) -> None:
    code = int(st_row[L.ST_STATUS])
    if code == 0:
        return
    if code == L.E_KEYERROR:
        raise KeyError("invert_base")      # what SF:1421 raises on a base outside ATCGN/atcgn
    if code == L.E_ARG:
        raise ValueError("sequence longer than %d bases or unsupported window size" % L.MAX_SEQ_LEN)
    raise RuntimeError("libvapor_hip pair status %d" % code)


# ------------------------------------------------------------------------------------------
# window_size_refine for many sequences at once
# ------------------------------------------------------------------------------------------

# Windows that met the X-means branch of the repeat check since the process started (SF:1165-1167), by outcome: `one_cluster`
# - BIC keeps one cluster, the reference's answer whatever its unseeded draws; `split` - more than one cluster: seed-dependent
# in the reference (and on current SciPy it raises there, SF:878); `sizes_decide` - of either kind, the windows whose diagonal
# share is at most 0.4, i.e. the only ones where the cluster sizes can change the window size at all (SF:2038).
qc_counts = {"band": 0, "one_cluster": 0, "split": 0, "sizes_decide": 0, "raised": 0}
_qc_lock = threading.Lock()


def refine_windows(engine, seqs: Sequence[str], region_QC_Cff: float = 0.4) -> List[list]:
    """window_size_refine (SF:2030-2046) for every sequence; returns [[w, qc] | ['Error','Error']].
    Exceptions the reference would raise for one sequence are returned in its slot.

    All self dot plots of a round (one window size) are one plan; the statistics are read as arrays, and only a
    plot whose lower-triangle share falls into (0.1, 0.5) (SF:1165) is fetched dot by dot for the clustering."""
    n = len(seqs)
    out: List[Optional[object]] = [None] * n
    work = []                     # (slot, seq2)
    for t, s in enumerate(seqs):
        s2 = s.replace("X", "") if "X" in s else s   # ''.join([i for i in seq2 if not i == 'X']), SF:2031
        if s2.count("N") + s2.count("n") > 100:
            out[t] = ["Error", "Error"]
        else:
            work.append((t, s2))
    k = 10
    while work:
        idx_of: Dict[str, int] = {}
        useqs: List[str] = []
        which = np.empty(len(work), dtype=np.int64)
        for w, (_t, s2) in enumerate(work):
            q = idx_of.get(s2)
            if q is None:
                q = idx_of[s2] = len(useqs)
                useqs.append(s2)
            which[w] = q
        pairs = np.zeros(len(useqs), dtype=L.PAIR_DTYPE)
        pairs["seq1"] = pairs["seq2"] = np.arange(len(useqs))
        pairs["k"] = k
        ss = engine.seqset(useqs)
        plan = engine.plan(ss, pairs)
        st_all = plan.run()
        # self plots of sequences longer than the plan's limit (the plan refuses them): the wide route, dots included
        wide_hits: Dict[int, np.ndarray] = {}
        longq = [q for q, s2 in enumerate(useqs) if len(s2) > L.MAX_SEQ_LEN] if has_wide(engine) else []
        if longq:
            st_w, h_w = engine.score_wide(ss, pairs[longq], want_hits=True)
            st_all = st_all.copy()
            st_all[longq] = st_w
            wide_hits = dict(zip(longq, h_w))
        st = st_all[which]
        code = st[:, L.ST_STATUS]
        nh, nd, nl = st[:, L.ST_N_HITS], st[:, L.ST_N_DIAG], st[:, L.ST_N_LOWER]
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = nl.astype(np.float64) / nh.astype(np.float64)
            diag = nd.astype(np.float64) / nh.astype(np.float64)
        band = (code == 0) & (nh > 0) & (frac > 0.1) & (frac < 0.5)
        pts = {}
        need = np.asarray([w for w in np.flatnonzero(band) if int(which[w]) not in wide_hits], dtype=np.int64)
        for w in np.flatnonzero(band):
            if int(which[w]) in wide_hits:
                h = wide_hits[int(which[w])]
                pts[int(w)] = h[h[:, 0] > h[:, 1]]
        if len(need):
            hits, _f, off = plan.fetch_hits(which[need].tolist(), want_flags=False)
            for q, w in enumerate(need):
                h = hits[off[q]:off[q + 1]]
                h = h[h[:, 0] > h[:, 1]]
                pts[int(w)] = h[np.lexsort((h[:, 1], h[:, 0]))]
        plan.close()
        ss.close()
        # the clustering of the windows in the band (sklearn / scipy, ~1 ms each, unseeded as in the reference) goes to the
        # host worker processes when there are enough of them to pay for the pickling
        sizes_of: Dict[int, object] = {}
        if len(pts) >= 8:
            from . import hostpool
            hp = hostpool.get()
            if hp is not None:
                futs = {w: hp.submit("vapor_amd.repeat_qc", "cluster_sizes_of_points", p) for w, p in pts.items()}
                for w, f in futs.items():
                    try:
                        sizes_of[w] = f.result()
                    except hostpool.WorkerLost:
                        pass                    # (clustered below, by this process)
                    except Exception as e:      # noqa: BLE001 - e.g. the clustering libraries' own errors
                        sizes_of[w] = e
        nxt = []
        for w, (t, s2) in enumerate(work):
            if code[w] != 0:
                try:
                    _raise_for_status(st[w])
                except Exception as e:      # noqa: BLE001
                    out[t] = e
                continue
            if nh[w] == 0:
                # SF:2035, 2045 at the first size; later an empty plot divides by zero in SF:1171
                out[t] = ["Error", "Error"] if k == 10 else ZeroDivisionError("float division by zero")
                continue
            if band[w]:
                try:
                    got = sizes_of[w] if w in sizes_of else repeat_qc.cluster_sizes(pts[w][:, 0].tolist(), pts[w][:, 1].tolist())
                    if isinstance(got, BaseException):
                        raise got
                    qc = [float(diag[w]), got]
                    with _qc_lock:
                        qc_counts["band"] += 1
                        qc_counts["one_cluster" if len(got) == 1 else "split"] += 1
                        qc_counts["sizes_decide"] += int(not qc[0] > region_QC_Cff)
                except Exception as e:          # noqa: BLE001 - e.g. the clustering libraries' own errors
                    with _qc_lock:
                        qc_counts["band"] += 1
                        qc_counts["raised"] += 1
                    out[t] = e
                    continue
            else:
                qc = [float(diag[w]), [0]]
            if k > 30 or qc[0] > region_QC_Cff or sum(qc[1]) / float(len(s2)) < 0.3:
                out[t] = [k, qc]
            else:
                nxt.append((t, s2))
        work = nxt
        k += 10
    return out  # type: ignore[return-value]


# ------------------------------------------------------------------------------------------
# scorer requests
# ------------------------------------------------------------------------------------------
_FLAGS = {"s1": L.PF_C1, "s2": L.PF_C2, "s3": L.PF_C1 | L.PF_DIR}
_KIND = {"del": 0, "s1": 1, "s2": 2, "s3": 3}


def _has_route(engine, route: str) -> bool:
    """A score_<route> method, and - for an engine that can say so (Engine.<route>_available) - a library that has the route."""
    if not callable(getattr(engine, "score_" + route, None)):
        return False
    avail = getattr(engine, route + "_available", None)
    return bool(avail()) if callable(avail) else True


def has_wide(engine) -> bool:
    """Whether `engine` has the wide route (sequences longer than MAX_SEQ_LEN, up to MAX_WIDE_SEQ_LEN)."""
    return _has_route(engine, "wide")


def has_anyk(engine) -> bool:
    """Whether `engine` has the any-k route (window sizes 1 .. MAX_ANY_K, the reference's kmerhits at every k)."""
    return _has_route(engine, "anyk")


def check_any_k(k) -> int:
    """The window size as an int, or the ValueError that names the any-k route's limit."""
    k = int(k)
    if not 1 <= k <= L.MAX_ANY_K:
        raise ValueError("window size %d outside 1 .. %d (VAPOR_MAX_ANY_K)" % (k, L.MAX_ANY_K))
    return k


def score_requests(engine, reqs: Sequence[Score]) -> List[object]:
    """Evaluates every Score request (_score_requests_narrow); the requests that route refuses for a window, allele or read
    longer than MAX_SEQ_LEN are scored again on the wide route (score_requests_wide) when the engine has one, in place, and
    those with a window size other than 10/20/30/40 on the any-k route when the engine has that."""
    out = _score_requests_narrow(engine, reqs)
    if has_wide(engine):
        redo = [t for t, v in enumerate(out) if isinstance(v, ValueError) and not k_unsupported(reqs[t].k)]
        if redo:
            for t, v in zip(redo, score_requests_wide(engine, [reqs[t] for t in redo])):
                out[t] = v
    if has_anyk(engine):
        redo = [t for t, v in enumerate(out) if isinstance(v, ValueError) and k_unsupported(reqs[t].k)
                and 1 <= int(reqs[t].k) <= L.MAX_ANY_K]
        if redo:
            for t, v in zip(redo, score_requests_wide(engine, [reqs[t] for t in redo], anyk=True)):
                out[t] = v
    return out


def score_requests_wide(engine, reqs: Sequence[Score], anyk: bool = False) -> List[object]:
    """score_requests on the wide route: the pairs' statistics from engine.score_wide, the per-read scores and the deletion
    rule (SF:1718-1726) on the host in float64 (vapor_amd.finish), as the device's finish kernel computes them.  anyk: the
    statistics from engine.score_anyk instead (any window size from 1 to MAX_ANY_K)."""
    from . import finish
    seqs: List[str] = []
    upper: List[bool] = []
    rows = []                         # (seq1, seq2, off2, k, flags)
    per_req = []                      # per request: [(kind, ref pair, alt pair)], one entry per scorer, per read
    for r in reqs:
        base = len(seqs)
        seqs += [str(r.ref_seq), str(r.alt_seq)]
        upper += [False, False]
        iu = (base, base + 1)
        if r.kind in ("del", "s1") and not (_is_upper(r.ref_seq) and _is_upper(r.alt_seq)):
            seqs += [str(r.ref_seq), str(r.alt_seq)]
            upper += [True, True]
            iu = (base + 2, base + 3)
        reads = []
        for x in r.reads:
            q = len(seqs)
            seqs.append(str(x[0]))
            upper.append(False)
            miss = int(x[1])
            sc = []
            plan_of = {"s1": [(1, iu, L.PF_C1)], "s2": [(2, (base, base + 1), L.PF_C2)],
                       "s3": [(3, (base, base + 1), L.PF_C1 | L.PF_DIR)],
                       "del": [(1, iu, L.PF_C1), (2, (base, base + 1), L.PF_C2)]}[r.kind]
            for kind, (a_ref, a_alt), fl in plan_of:
                sc.append((kind, len(rows), len(rows) + 1))
                rows += [(q, a_ref, miss, int(r.k), fl), (q, a_alt, miss, int(r.k), fl)]
            reads.append(sc)
        per_req.append(reads)
    ss = engine.seqset(seqs, upper)
    try:
        st = (engine.score_anyk if anyk else engine.score_wide)(ss, engine.make_pairs(rows))
    finally:
        ss.close()
    out: List[object] = []
    for r, reads in zip(reqs, per_req):
        idx = [p for sc in reads for (_k, a, b) in sc for p in (a, b)]
        codes = st[idx, L.ST_STATUS] if idx else np.zeros(0, dtype=np.int64)
        if (codes == L.E_ARG).any():
            out.append(ValueError("sequence longer than %d bases or unsupported window size" % L.MAX_WIDE_SEQ_LEN))
            continue
        if (codes == L.E_KEYERROR).any():
            out.append(KeyError("invert_base"))              # what SF:1421 raises on a base outside ATCGN/atcgn
            continue
        if (codes != 0).any():
            out.append(RuntimeError("libvapor_hip pair status %d" % int(codes[codes != 0][0])))
            continue
        lr, la = len(r.ref_seq), len(r.alt_seq)
        vals: List[object] = []
        for sc in reads:
            ss_ = []
            for kind, a, b in sc:
                av, bv, valid = finish.batch_scores(np.asarray([kind]), st[[a]], st[[b]], np.asarray([lr]), np.asarray([la]))
                ss_.append(float(finish.read_scores(av, bv)[0]) if bool(valid[0]) else None)
            if len(ss_) == 2:                                 # a deletion read: the smaller of the two scores wins
                s1, s2 = ss_
                v = (s2 if s2 < s1 else s1) if (s1 is not None and s2 is not None) else (s1 if s1 is not None else s2)
            else:
                v = ss_[0]
            vals.append(v)
        out.append(vals)
    return out


class _SetBuilder:
    """The sequences of one device batch: `seqs` travel as bytes (windows, insertion payloads, reads), `derived` are described
    instead (drivers.Allele.segs; the str.upper() twins of abs_dis_m1b) as (segments, upper)."""

    def __init__(self):
        self.seqs: List[str] = []
        self.derived: List[tuple] = []
        self.lit_of: Dict[int, int] = {}       # id(string) -> its index among the literals (a window is uploaded once per batch)
        self.nocomp_of: Dict[int, bool] = {}
        self.derived_of: Dict[tuple, int] = {}  # (id(string), upper) -> its derived index: requests that share a window share its twins too

    def lit(self, sq: str) -> int:
        q = self.lit_of.get(id(sq))
        if q is None:
            q = self.lit_of[id(sq)] = len(self.seqs)
            self.seqs.append(sq)
        return q

    def describe(self, sq, up: bool) -> int:
        got = self.derived_of.get((id(sq), up))
        if got is not None:
            return got
        got = self.derived_of[(id(sq), up)] = self._describe(sq, up)
        return got

    def _describe(self, sq, up: bool) -> int:
        """Index of `sq` (upper-cased when `up`) in the set: a literal, or - (d + 1) for derived sequence d (their place behind
        the literals is known when all literals are)."""
        derived, lit = self.derived, self.lit
        segs = getattr(sq, "segs", None)
        if segs is not None and len(segs) > L.MAX_SEGMENTS:
            segs = None               # (more blocks than a descriptor holds, include/vapor_hip.h: this allele travels as bytes)
        if segs is not None and segs:
            # (a reversed slice needs a parent complementary() keeps whole, SF:471-478: the library checks the same)
            for par, _o, _n, rc in segs:
                if rc:
                    bad = self.nocomp_of.get(id(par))
                    if bad is None:
                        bad = self.nocomp_of[id(par)] = _NOCOMP.search(par) is not None
                    if bad:
                        segs = None
                        break
        if segs:
            derived.append(([(lit(par), o, n, rc) for par, o, n, rc in segs], up))
            return -len(derived)
        if up:
            derived.append(([(lit(sq), 0, len(sq), False)], True))
            return -len(derived)
        return lit(sq)


def _score_requests_narrow(engine, reqs: Sequence[Score]) -> List[object]:
    """Evaluates every Score request on the device, per-read reduction included (finish_kernel): per request a list
    with one score (float) or None per read, or the exception the reference would raise (KeyError for a read with a
    base outside invert_base's alphabet, SF:1421).

    One sequence set and one plan for all requests: request t is "locus" t of the plan, its reads are the plan's
    reads in order.  The arrays are put together with numpy per request, not per read."""
    sb = _SetBuilder()
    seqs, derived, describe = sb.seqs, sb.derived, sb.describe

    # per request: scalars only; the per-read and per-pair columns are expanded from them in one go below
    rq_n, rq_k, rq_kind, rq_lref, rq_lalt, rq_blk_a, rq_blk_b = [], [], [], [], [], [], []
    bl_rq, bl_ref, bl_alt, bl_flags = [], [], [], []         # blocks of pairs: (request, its two allele sequences, pair flags)
    miss: List[int] = []
    first_read, read_seq_first = [], []
    n_reads_tot = 0
    for t, r in enumerate(reqs):
        n = len(r.reads)
        first_read.append(n_reads_tot)
        if n == 0:
            read_seq_first.append(len(seqs))
            continue
        # allele sequences of this request: as given, and (abs_dis_m1b, SF:183-184) upper-cased where that differs
        ri, ai = describe(r.ref_seq, False), describe(r.alt_seq, False)
        if r.kind in ("del", "s1") and not (_is_upper(r.ref_seq) and _is_upper(r.alt_seq)):
            uri, uai = describe(r.ref_seq, True), describe(r.alt_seq, True)
        else:
            uri, uai = ri, ai
        read_seq_first.append(len(seqs))
        seqs += [x[0] for x in r.reads]                      # (reads are never shared between requests: no look-up)
        miss += [int(x[1]) for x in r.reads]
        k = len(rq_n)
        if r.kind == "del" and uri != ri:
            blk_a = len(bl_rq)
            bl_rq += [k, k]; bl_ref += [uri, ri]; bl_alt += [uai, ai]; bl_flags += [L.PF_C1, L.PF_C2]
            blk_b = blk_a + 1
        else:
            # (a deletion whose alleles are upper case already: one fill serves both scorers)
            blk_a = blk_b = len(bl_rq)
            bl_rq.append(k)
            plain = r.kind in ("del", "s2", "s3")
            bl_ref.append(ri if plain else uri); bl_alt.append(ai if plain else uai)
            bl_flags.append(L.PF_C1 | L.PF_C2 if r.kind == "del" else _FLAGS[r.kind])
        rq_n.append(n); rq_k.append(int(r.k)); rq_kind.append(_KIND[r.kind]); rq_lref.append(len(r.ref_seq)); rq_lalt.append(len(r.alt_seq))
        rq_blk_a.append(blk_a); rq_blk_b.append(blk_b)
        n_reads_tot += n
    if n_reads_tot == 0:
        return [[] for _ in reqs]
    i32 = np.int32
    nz = [t for t, r in enumerate(reqs) if len(r.reads)]     # requests with reads, in order (rq_* are indexed by position here)
    rq_n_a = np.asarray(rq_n, dtype=np.int64)
    rq_first = np.concatenate(([0], np.cumsum(rq_n_a)[:-1]))             # first read of a request in the read table
    rq_q0 = np.asarray([read_seq_first[t] for t in nz], dtype=np.int64)  # its first read sequence
    miss_a = np.asarray(miss, dtype=i32)
    # blocks -> pairs: block b holds, per read i of its request, the pairs (read, allele) and (read, allele + 1)
    bl_rq_a = np.asarray(bl_rq, dtype=np.int64)
    bl_n = rq_n_a[bl_rq_a]
    bl_base = 2 * np.concatenate(([0], np.cumsum(bl_n)[:-1]))            # first pair of a block
    br_blk = np.repeat(np.arange(len(bl_rq_a)), bl_n)                     # per (block, read): its block
    br_i = np.arange(int(bl_n.sum())) - np.repeat(bl_base // 2, bl_n)     # ... and the read's index in the request
    br_rq = bl_rq_a[br_blk]
    pairs = np.zeros(2 * len(br_blk), dtype=L.PAIR_DTYPE)
    pairs["seq1"] = np.repeat((rq_q0[br_rq] + br_i).astype(i32), 2)
    n_lit = len(seqs)

    def placed(v):                                            # derived sequence d: behind the literals
        v = np.asarray(v, dtype=np.int64)
        return np.where(v < 0, n_lit - 1 - v, v).astype(i32)
    al = np.empty(2 * len(br_blk), dtype=i32)
    al[0::2] = placed(bl_ref)[br_blk]
    al[1::2] = placed(bl_alt)[br_blk]
    pairs["seq2"] = al
    pairs["off2"] = np.repeat(miss_a[rq_first[br_rq] + br_i], 2)
    pairs["k"] = np.repeat(np.asarray(rq_k, dtype=i32)[br_rq], 2)
    pairs["flags"] = np.repeat(np.asarray(bl_flags, dtype=np.uint32)[br_blk], 2)
    # read table: read i of request r takes its statistics from pairs base(block) + 2 i (+ 1 for the other allele)
    rd_rq = np.repeat(np.arange(len(rq_n_a)), rq_n_a)
    rd_i = np.arange(n_reads_tot) - rq_first[rd_rq]
    pa = (bl_base[np.asarray(rq_blk_a, dtype=np.int64)][rd_rq] + 2 * rd_i).astype(i32)
    pb = (bl_base[np.asarray(rq_blk_b, dtype=np.int64)][rd_rq] + 2 * rd_i).astype(i32)
    table = np.zeros(n_reads_tot, dtype=L.READ_DTYPE)
    table["ref_a"], table["alt_a"], table["ref_b"], table["alt_b"] = pa, pa + 1, pb, pb + 1
    table["kind"] = np.asarray(rq_kind, dtype=i32)[rd_rq]
    table["locus"] = np.asarray(nz, dtype=i32)[rd_rq]
    table["len_ref"] = np.asarray(rq_lref, dtype=i32)[rd_rq]
    table["len_alt"] = np.asarray(rq_lalt, dtype=i32)[rd_rq]
    ss = engine.seqset(seqs, None, derived) if derived else engine.seqset(seqs)
    try:
        plan = engine.plan(ss, pairs)
        try:
            plan.set_reads(table, len(reqs))
            plan.run_loci(want_host=False, want_scores=True)
            sc = plan.read_scores[:n_reads_tot]
        finally:
            plan.close()
        # pairs the library rejects, as the reference would have raised: a read k-mer with a base outside
        # invert_base's alphabet (SF:1421), a sequence beyond the device's 16-bit positions
        bad_inv = np.asarray(ss.n_invalid) > 0
        lens = np.asarray(ss.lens)
    finally:
        ss.close()
    # per request with reads: longest read, any read the library could not have hashed (one pass over all reads)
    rd_q = rq_q0[rd_rq] + rd_i
    rd_len = lens[rd_q]
    max_read = np.maximum.reduceat(rd_len, rq_first)
    rd_inv = bad_inv[rd_q] & (rd_len - np.asarray(rq_k, dtype=np.int64)[rd_rq] + 1 > 0)
    any_inv = np.logical_or.reduceat(rd_inv, rq_first)
    vals = sc.tolist()
    if sc.size and bool(np.isnan(sc).any()):
        vals = [None if x != x else x for x in vals]
    out: List[object] = []
    j = 0
    for t, r in enumerate(reqs):
        n = len(r.reads)
        if n == 0:
            out.append([])
            continue
        if k_unsupported(r.k) or max(len(r.ref_seq), len(r.alt_seq)) > L.MAX_SEQ_LEN or int(max_read[j]) > L.MAX_SEQ_LEN:
            out.append(ValueError("sequence longer than %d bases or unsupported window size" % L.MAX_SEQ_LEN))
        elif any_inv[j]:
            out.append(KeyError("invert_base"))              # what SF:1421 raises on a base outside ATCGN/atcgn
        else:
            out.append(vals[first_read[t]:first_read[t] + n])
        j += 1
    return out


# ------------------------------------------------------------------------------------------
# `--realign`: every read against both alleles (drivers.Realign)
# ------------------------------------------------------------------------------------------
def realign_requests(engine, reqs: Sequence[object]) -> List[object]:
    """Evaluates every Realign request of a batch: one sequence set (reads as literals, alleles described where they are
    drivers.Alleles: nothing of a derived allele crosses the link), two pairs a read - the read against the reference allele and
    against the alt allele, both from miss_bp on - and one engine.realign call.  Per request a realign.Payload, or None when one
    of its pairs came back with a status.  An engine without the kernel raises (Engine.realign): there is no other route."""
    from . import realign
    sb = _SetBuilder()
    rows = []                         # (read, allele, miss_bp), the reference allele's pair before the alt allele's
    first = []
    for r in reqs:
        first.append(len(rows))
        if not r.reads:
            continue
        ri, ai = sb.describe(r.ref_seq, False), sb.describe(r.alt_seq, False)
        for x in r.reads:
            q = len(sb.seqs)
            sb.seqs.append(x[0])                             # (reads are never shared between requests: no look-up)
            rows += [(q, ri, int(x[1])), (q, ai, int(x[1]))]
    first.append(len(rows))
    ss = pairs = d = None                  # (a batch without a read has no set, no table and nothing to trace)
    try:
        if rows:
            n_lit = len(sb.seqs)
            pairs = np.zeros(len(rows), dtype=L.PAIR_DTYPE)
            tab = np.asarray(rows, dtype=np.int64)
            pairs["seq1"] = tab[:, 0]
            pairs["seq2"] = np.where(tab[:, 1] < 0, n_lit - 1 - tab[:, 1], tab[:, 1])       # derived sequence d: behind the literals
            pairs["off2"] = tab[:, 2]
            ss = engine.seqset(sb.seqs, None, sb.derived) if sb.derived else engine.seqset(sb.seqs)
            d, st = engine.realign(ss, pairs, realign.BAND)
            out = [realign.payload(d[a:b:2], d[a + 1:b:2], st[a:b:2], st[a + 1:b:2]) for a, b in zip(first[:-1], first[1:])]
        else:
            out = [realign.Payload() for _ in reqs]
        # the steps the requests' options ask for, in their order; the junction's call has a set of its own
        if ss is not None and any(r.trace for r in reqs):
            _realign_traces(engine, ss, reqs, out, pairs, d, first)
        if any(r.polish for r in reqs):
            _realign_polish(engine, ss, reqs, out, pairs, first, d)
    finally:
        if ss is not None:
            ss.close()
    if any(r.junction for r in reqs):
        _realign_junction(engine, reqs, out)     # (an empty pile has fewer than MIN_COV reads: no junction applies)
    return out


def _realign_traces(engine, ss, reqs, out, pairs, d, first) -> None:
    """`--realign-out`: one engine.realign_trace call over the set of the distances' call, one pair a read of
    every request that asks for traces and has a payload - the read against the allele it fits (realign.fits_alt) - at a modest
    cap_runs, and one more call for the pairs that overflowed, at n + m + 1, which always holds.  The traces ride on the
    payload (`.traces`)."""
    from . import realign
    pick, where = [], []                      # the pair of the distances' table a read is traced on; (request, read)
    for t, (r, a) in enumerate(zip(reqs, first[:-1])):
        if not r.trace or out[t] is None:
            continue
        for k, diff in enumerate(out[t]):
            pick.append(a + 2 * k + (1 if realign.fits_alt(diff) else 0))
            where.append((t, k))
    got = {}
    todo, cap = list(range(len(pick))), realign.FIRST_CAP_RUNS
    for attempt in (0, 1):
        if not todo:
            break
        tp = pairs[np.asarray([pick[q] for q in todo], dtype=np.int64)]
        head, runs = engine.realign_trace(ss, tp, realign.BAND, cap)
        over = []
        for q, h, w in zip(todo, head, runs):
            if int(h[1]) == L.E_OVERFLOW and attempt == 0:
                over.append(q)
            else:
                got[q] = (int(h[1]), int(h[2]), int(h[3]), realign.runs_of(h, w) if int(h[1]) == 0 else [])
        todo, cap = over, 2 * L.MAX_SEQ_LEN + 1
        if over:                              # (a path has at most n + m steps)
            cap = min(cap, 1 + max(len(reqs[t].reads[k][0]) + max(len(reqs[t].ref_seq), len(reqs[t].alt_seq))
                                   for t, k in (where[q] for q in over)))
    for t, r in enumerate(reqs):
        if r.trace and out[t] is not None:
            out[t].traces = realign.Traces(r.ref_seq, r.alt_seq, [])
    for q, (t, k) in enumerate(where):
        status, i_end, j_end, rr = got[q]
        x = reqs[t].reads[k]
        a = first[t]
        out[t].traces.reads.append((x[0], int(x[1]), int(d[a + 2 * k]), int(d[a + 2 * k + 1]), i_end, j_end, rr if status == 0 else []))


def _realign_polish(engine, ss, reqs, out, pairs, first, d=None) -> None:
    """`--realign-polish`: one engine.realign_polish call over the set of the distances' call for the requests
    that ask and have a payload - per request one locus, its pairs the alt pair of every read that votes ALT.  The statistics
    ride on the payload (`.polish`); the polished allele is spelt only where a sink takes it (the request asks for traces and
    has them).  A request without reads has nothing in the set: its pile is empty, which needs no call.
    `--realign-revote`: where a request of the batch asks, the one call is engine.realign_revote instead - the
    same loci and pairs, and as vote pairs the alt pair of every read of a request that asks and has at least MIN_COV voters.
    What comes back rides on the payload (`.revote`) beside d_ref of the first call (`d`, the distances of `pairs`)."""
    from . import polish, realign, revote
    pick, pfirst, col_off, who = [], [0], [0], []
    votes, vfirst = [], [0]
    for t, (r, a) in enumerate(zip(reqs, first[:-1])):
        if not r.polish or out[t] is None:
            continue
        if not r.reads:
            out[t].polish = polish.Polish([0] * 8, str(r.alt_seq) if out[t].traces is not None else None)
            continue
        mine = [a + 2 * k + 1 for k, diff in enumerate(out[t]) if diff >= realign.MARGIN]
        pick += mine
        pfirst.append(len(pick))
        if r.revote and len(mine) >= polish.MIN_COV:
            votes += [a + 2 * k + 1 for k in range(len(out[t]))]
        vfirst.append(len(votes))
        col_off.append(col_off[-1] + len(r.alt_seq))
        who.append(t)
    if not who:
        return
    if any(reqs[t].revote for t in who):
        stats, calls, sites, ins, _counts, vout, lout, _so, _spelt = engine.realign_revote(
            ss, pairs[np.asarray(pick, dtype=np.int64)], realign.BAND, pfirst, col_off, pairs[np.asarray(votes, dtype=np.int64)], vfirst)
        for g, t in enumerate(who):
            mine = vout[vfirst[g]:vfirst[g + 1]]
            if reqs[t].revote and len(mine):
                bad = [int(v[1]) for v in mine if int(v[1]) != 0]
                a = first[t]
                out[t].revote = revote.Revote(int(lout[g][0]) or (bad[0] if bad else 0), [int(d[a + 2 * k]) for k in range(len(mine))],
                                              [int(v[0]) for v in mine])
    else:
        stats, calls, sites, ins, _counts = engine.realign_polish(ss, pairs[np.asarray(pick, dtype=np.int64)], realign.BAND, pfirst, col_off)
    for g, t in enumerate(who):
        text = None
        # (the text is spelt for a sink, and for the junction where the polish applies; a locus the entry refuses keeps its
        # allele: the columns say '.')
        if reqs[t].trace or (reqs[t].junction and int(stats[g][0]) == 0 and int(stats[g][1]) >= polish.MIN_COV):
            text = str(reqs[t].alt_seq)
            if int(stats[g][0]) == 0:
                text = polish.apply(text, calls[col_off[g]:col_off[g + 1]], sites[g], ins[g])
        out[t].polish = polish.Polish(stats[g], text)


def _lens_window(r):
    """(first, symbols) of the stretch of r.ref_seq that the called allele spans: from the start of its first segment to the end
    of its last, where both are forward slices of r.ref_seq; otherwise all of it.  Only an INS call below 5 000 bases differs
    from the whole window: vapor_simple_ins reads that window len(ins) bases past the right flank."""
    segs = getattr(r.alt_seq, "segs", None)
    if segs and all(par is r.ref_seq and not rc for par, _o, _n, rc in (segs[0], segs[-1])):
        lo, hi = int(segs[0][1]), int(segs[-1][1]) + int(segs[-1][2])
        if 0 <= lo < hi <= len(r.ref_seq):
            return lo, hi - lo
    return 0, len(r.ref_seq)


def _realign_junction(engine, reqs, out) -> None:
    """`--realign-junction`: one engine.realign_junction call for the requests that ask and whose polish applies
    (status 0, at least MIN_COV reads piled) - per request two pairs, the call's own alt allele and the polished one, each
    against the window the called allele spans (_lens_window), the shorter sequence first - over one small sequence set:
    windows and called alleles described as for the distances, polished alleles as literals.  The nine integers ride on the
    payload (`.junction`), left and right in r.ref_seq's coordinates; where a pair comes back with a status there is none."""
    from . import junction, polish, realign
    from .drivers import Allele
    sb = _SetBuilder()
    rows, who, cut = [], [], []              # (`cut`: the described windows, alive while the builder keys them by id)
    for t, r in enumerate(reqs):
        po = out[t].polish if out[t] is not None else None
        if not r.junction or po is None or po.text is None or po.stats[polish.STATUS] != 0 or po.stats[polish.PAIRS] < polish.MIN_COV:
            continue
        lo, n_win = _lens_window(r)
        win = r.ref_seq
        if (lo, n_win) != (0, len(r.ref_seq)):
            win = Allele(r.ref_seq[lo:lo + n_win])
            win.segs = [(r.ref_seq, lo, n_win, False)]
            cut.append(win)
        wi, ai = sb.describe(win, False), sb.describe(r.alt_seq, False)
        pi = len(sb.seqs)
        sb.seqs.append(po.text)                          # (a polished allele belongs to one request: no look-up)
        forms = (junction.deletion_form(len(r.alt_seq), n_win), junction.deletion_form(len(po.text), n_win))
        rows += [(ai, wi) if forms[0] else (wi, ai), (pi, wi) if forms[1] else (wi, pi)]
        who.append((t, forms, lo))
    if not who:
        return
    n_lit = len(sb.seqs)
    tab = np.asarray(rows, dtype=np.int64)
    tab = np.where(tab < 0, n_lit - 1 - tab, tab)        # derived sequence d: behind the literals
    pairs = np.zeros(len(rows), dtype=L.PAIR_DTYPE)
    pairs["seq1"], pairs["seq2"] = tab[:, 0], tab[:, 1]
    ss = engine.seqset(sb.seqs, None, sb.derived) if sb.derived else engine.seqset(sb.seqs)
    try:
        recs, _row_off, _rows = engine.realign_junction(ss, pairs, realign.BAND)
    finally:
        ss.close()
    for g, (t, forms, lo) in enumerate(who):
        called, polished = recs[2 * g], recs[2 * g + 1]
        if int(called[0]) == 0 and int(polished[0]) == 0:
            c0, l0, r0, g0, _k0 = junction.of_record(called, forms[0])
            c1, l1, r1, g1, k1 = junction.of_record(polished, forms[1])
            out[t].junction = junction.Junction((c0, l0 + lo, r0 + lo, g0, c1, l1 + lo, r1 + lo, g1, k1))
        if not reqs[t].trace:
            out[t].polish.text = None                    # (no sink takes it)


# ------------------------------------------------------------------------------------------
# breakpoint refinement: grids of candidate alleles (drivers.ScoreGrid)
# ------------------------------------------------------------------------------------------
GRID_PAIRS_PER_PLAN = 150000      # a plan of grids is sized by pairs, not by loci (121 candidates x 20 reads: some 5 000 pairs a locus;
                                  # a chunk of 2 048 unrefined loci makes a plan of about as many pairs)


def has_grid(engine) -> bool:
    """Whether `engine` has breakpoint refinement's device step (vapor_plan_set_grid / vapor_plan_run_grid): an engine that
    can say so (Engine.grid_available) over a library that has it.  The tests' stand-in and the CPU twin have not."""
    avail = getattr(engine, "grid_available", None)
    return bool(avail()) if callable(avail) else False


def score_grids(engine, reqs: Sequence[object], route: Optional[str] = None, want_all: bool = False) -> List[object]:
    """Evaluates every ScoreGrid request: per request a refine.GridResult, or the exception its scoring ended with.
    route 'batched': one sequence set and one plan for many grids, the choice on the device (_score_grids_batched);
    'brute': refine.score_grid_brute per request; None: VAPOR_REFINE_ROUTE, else batched where the engine has the device step.
    A request the narrow route refuses (a window size other than 10/20/30/40, a sequence longer than MAX_SEQ_LEN) goes the
    brute-force way on either route, where the wide and any-k routes take it."""
    import os
    from . import refine
    route = route or os.environ.get("VAPOR_REFINE_ROUTE") or ("batched" if has_grid(engine) else "brute")
    if route not in ("batched", "brute"):
        raise ValueError("refinement route %r (batched | brute)" % route)
    if route == "batched" and not has_grid(engine):
        raise NotImplementedError("the loaded library has no refinement kernel (vapor_plan_run_grid)")
    out: List[object] = [None] * len(reqs)
    fast = []
    for t, r in enumerate(reqs):
        narrow = (not k_unsupported(r.k) and len(r.reads) > 0 and 0 < len(r.alts) <= L.MAX_CANDIDATES
                  and max([len(r.ref_seq)] + [len(a) for a in r.alts] + [len(x[0]) for x in r.reads]) <= L.MAX_SEQ_LEN)
        if route == "batched" and narrow:
            fast.append(t)
        else:
            out[t] = refine.score_grid_brute(engine, r)
    # plans by pairs: a grid request holds (candidates + 1) x reads x blocks pairs
    batch, n_pairs = [], 0
    for t in fast + [None]:
        cost = 0 if t is None else 2 * (len(reqs[t].alts) + 1) * len(reqs[t].reads)
        if batch and (t is None or n_pairs + cost > GRID_PAIRS_PER_PLAN):
            for q, v in zip(batch, _score_grids_batched(engine, [reqs[q] for q in batch], want_all)):
                out[q] = v
            batch, n_pairs = [], 0
        if t is not None:
            batch.append(t)
            n_pairs += cost
    return out


def _score_grids_batched(engine, reqs: Sequence[object], want_all: bool = False) -> List[object]:
    """The batched route: one sequence set and one plan for all requests.  Per request the window and every read are uploaded
    once and every candidate allele is a derived sequence of the window; the pairs are (read, window) once per read and
    block of pairs (the upper-cased and the plain block of a soft-masked deletion, as _score_requests_narrow cuts them) plus
    (read, candidate) per candidate; the read table has a row per (candidate, read) whose ref_a / ref_b point at the shared
    (read, window) pair; the plan's loci are the candidates and its groups the requests (Plan.set_grid).  finish_kernel
    scores every candidate, grid_pick_kernel behind it chooses; the winners' records and scores come back."""
    from . import refine
    sb = _SetBuilder()
    i32 = np.int32
    pr_seq1, pr_seq2, pr_off2, pr_k, pr_flags = [], [], [], [], []
    tb = {f: [] for f in ("ref_a", "alt_a", "ref_b", "alt_b", "kind", "locus", "len_ref", "len_alt")}
    first_locus = [0]
    read_q0 = []
    n_pairs = 0
    for r in reqs:
        n, nc = len(r.reads), len(r.alts)
        soft = r.kind in ("del", "s1") and not (_is_upper(r.ref_seq) and all(_is_upper(a) for a in r.alts))
        ri = sb.describe(r.ref_seq, False)
        ai = [sb.describe(a, False) for a in r.alts]
        if soft:
            uri, uai = sb.describe(r.ref_seq, True), [sb.describe(a, True) for a in r.alts]
        else:
            uri, uai = ri, ai
        if r.kind == "del" and soft:
            blocks = [(uri, uai, L.PF_C1), (ri, ai, L.PF_C2)]
        else:
            plain = r.kind in ("del", "s2", "s3")
            blocks = [(ri if plain else uri, ai if plain else uai, L.PF_C1 | L.PF_C2 if r.kind == "del" else _FLAGS[r.kind])]
        nb = len(blocks)
        q0 = len(sb.seqs)
        read_q0.append(q0)
        sb.seqs.extend(x[0] for x in r.reads)                 # (reads are never shared between requests: no look-up)
        rd = np.arange(q0, q0 + n, dtype=np.int64)
        miss = np.asarray([int(x[1]) for x in r.reads], dtype=np.int64)
        base = n_pairs
        # pairs: block b's (read, window) at base + b n + i, its (read, candidate c) at base + nb n + (c nb + b) n + i
        rows = (nc + 1) * nb
        w_idx = np.asarray([blk[0] for blk in blocks], dtype=np.int64)
        a_idx = np.asarray([blk[1] for blk in blocks], dtype=np.int64).T.reshape(-1)        # (candidate, block) order
        pr_seq1.append(np.tile(rd, rows)); pr_off2.append(np.tile(miss, rows))
        pr_seq2.append(np.repeat(np.concatenate((w_idx, a_idx)), n))
        pr_flags.append(np.tile(np.repeat(np.asarray([blk[2] for blk in blocks], dtype=np.int64), n), nc + 1))
        pr_k.append(np.full(rows * n, int(r.k), dtype=np.int64))
        n_pairs += rows * n
        it = np.arange(n, dtype=np.int64)
        cand = np.repeat(np.arange(nc, dtype=np.int64), n)
        alt_a = base + nb * n + cand * (nb * n) + np.tile(it, nc)
        tb["ref_a"].append(np.tile(base + it, nc)); tb["alt_a"].append(alt_a)
        tb["ref_b"].append(np.tile(base + (nb - 1) * n + it, nc)); tb["alt_b"].append(alt_a + (nb - 1) * n)
        tb["kind"].append(np.full(nc * n, _KIND[r.kind], dtype=np.int64))
        tb["locus"].append(first_locus[-1] + cand)
        tb["len_ref"].append(np.full(nc * n, len(r.ref_seq), dtype=np.int64))
        tb["len_alt"].append(np.repeat(np.asarray([len(x) for x in r.alts], dtype=np.int64), n))
        first_locus.append(first_locus[-1] + nc)
    n_lit = len(sb.seqs)
    pairs = np.zeros(n_pairs, dtype=L.PAIR_DTYPE)
    pairs["seq1"] = np.concatenate(pr_seq1).astype(i32)
    s2 = np.concatenate(pr_seq2)
    pairs["seq2"] = np.where(s2 < 0, n_lit - 1 - s2, s2).astype(i32)      # derived sequence d: behind the literals
    pairs["off2"] = np.concatenate(pr_off2).astype(i32)
    pairs["k"] = np.concatenate(pr_k).astype(i32)
    pairs["flags"] = np.concatenate(pr_flags).astype(np.uint32)
    n_rows = sum(len(x) for x in tb["kind"])
    table = np.zeros(n_rows, dtype=L.READ_DTYPE)
    for f, cols in tb.items():
        table[f] = np.concatenate(cols).astype(i32)
    # (the descriptors as arrays, put together in one go: a grid of 121 candidates is some 250 derived sequences)
    flat = [g for sg, _u in sb.derived for g in sg]
    seg_first = np.zeros(len(sb.derived) + 1, dtype=i32)
    np.cumsum([len(sg) for sg, _u in sb.derived], out=seg_first[1:])
    segs = np.zeros(max(len(flat), 1), dtype=L.SEG_DTYPE)
    if flat:
        cols = np.asarray(flat, dtype=np.int64)
        segs["parent"][:len(flat)], segs["off"][:len(flat)], segs["len"][:len(flat)] = cols[:, 0], cols[:, 1], cols[:, 2]
        segs["flags"][:len(flat)] = np.where(cols[:, 3] != 0, L.SEG_REVCOMP, 0)
    dflags = np.asarray([L.SEQ_UPPER if u else 0 for _sg, u in sb.derived], dtype=np.uint8)
    ss = engine.seqset(sb.seqs, None, (seg_first, segs, dflags)) if sb.derived else engine.seqset(sb.seqs)
    try:
        plan = engine.plan(ss, pairs)
        try:
            plan.set_reads(table, first_locus[-1])
            plan.set_grid(np.asarray(first_locus, dtype=i32))
            widx, rec, wsc, off = plan.run_grid()
            widx, rec, wsc = widx.copy(), rec.copy(), wsc.copy()
            if want_all:
                all_recs = plan.run_loci(want_host=True, want_scores=True).copy()
                all_sc = plan.read_scores[:n_rows].copy()
        finally:
            plan.close()
        bad_inv = np.asarray(ss.n_invalid) > 0
        lens = np.asarray(ss.lens)
    finally:
        ss.close()

    def as_list(a):
        return [None if x != x else x for x in a.tolist()]
    out: List[object] = []
    row0 = 0
    for g, r in enumerate(reqs):
        n, nc = len(r.reads), len(r.alts)
        q = np.arange(read_q0[g], read_q0[g] + n)
        if bool((bad_inv[q] & (lens[q] - int(r.k) + 1 > 0)).any()):
            out.append(KeyError("invert_base"))              # what SF:1421 raises on a base outside ATCGN/atcgn
        else:
            res = refine.GridResult(widx[g], rec[g, :L.LOCUS_STRIDE], rec[g, L.LOCUS_STRIDE:], as_list(wsc[off[g]:off[g + 1]]))
            if want_all:
                res.all_recs = all_recs[first_locus[g]:first_locus[g + 1]]
                res.all_scores = [as_list(all_sc[row0 + c * n:row0 + (c + 1) * n]) for c in range(nc)]
            out.append(res)
        row0 += nc * n
    return out


def scorer_outputs(engine, kind: str, ref_seq: str, alt_seq: str, x, k):
    """[a, b] of calcu_vapor_single_read_score_{abs_dis_m1b, within_10Perc_m1b, directed_dis_m1b_redefine_diagnal}
    (kind 's1', 's2', 's3'; SF:182-203, 277-294, 241-257) for one read: the two dot plots' statistics from the
    device, the scorer's own gates and ratios on the host in float64 (vapor_amd.finish)."""
    from . import finish
    anyk = k_unsupported(k) and has_anyk(engine)
    if anyk:
        k = check_any_k(k)
    up = kind == "s1"
    ss = engine.seqset([x[0], ref_seq, alt_seq], [False, up, up])
    wide = has_wide(engine) and max(len(x[0]), len(ref_seq), len(alt_seq)) > L.MAX_SEQ_LEN
    try:
        pr = engine.make_pairs([(0, 1, int(x[1]), int(k), _FLAGS[kind]), (0, 2, int(x[1]), int(k), _FLAGS[kind])])
        st = engine.score_anyk(ss, pr) if anyk else engine.score_wide(ss, pr) if wide else engine.score(ss, pr)
    finally:
        ss.close()
    _raise_for_status(st[0])
    _raise_for_status(st[1])
    fn = {"s1": finish.score_abs_dis_m1b, "s2": finish.score_within_10Perc_m1b,
          "s3": finish.score_directed_dis_m1b_redefine_diagnal}[kind]
    return fn(st[0], st[1], len(ref_seq), len(alt_seq))


import re as _re

_NOCOMP = _re.compile("[^ACGTNacgtn]")       # what complementary() drops (SF:471-478)


def _is_upper(s: str) -> bool:
    return s.isupper() or s.upper() == s


def k_unsupported(k) -> bool:
    return int(k) not in (10, 20, 30, 40)


# ------------------------------------------------------------------------------------------
# executors
# ------------------------------------------------------------------------------------------

def _answer(engine, reqs: Sequence[object], figure_fn) -> List[object]:
    res: List[object] = [None] * len(reqs)
    wi = [t for t, r in enumerate(reqs) if isinstance(r, Window)]
    si = [t for t, r in enumerate(reqs) if isinstance(r, Score)]
    if wi:
        for t, v in zip(wi, refine_windows(engine, [reqs[t].seq for t in wi])):
            res[t] = v
    if si:
        for t, v in zip(si, score_requests(engine, [reqs[t] for t in si])):
            res[t] = v
    gi = [t for t, r in enumerate(reqs) if isinstance(r, ScoreGrid)]
    if gi:
        for t, v in zip(gi, score_grids(engine, [reqs[t] for t in gi])):
            res[t] = v
    ri = [t for t, r in enumerate(reqs) if isinstance(r, Realign)]
    if ri:
        for t, v in zip(ri, realign_requests(engine, [reqs[t] for t in ri])):
            res[t] = v
    if figure_fn is not None:
        figs = [r for r in reqs if isinstance(r, Figure)]
        batch = getattr(figure_fn, "batch", None)      # (figures.make_event_figure_1: one device pass, drawing in worker processes)
        if figs and batch is not None:
            batch(figs, engine)             # (the chunk's own engine: a library context serves one host thread)
        else:
            for r in figs:
                figure_fn(r)
    return res


def run_sync(gen, engine=None, figure_fn: Optional[Callable] = None):
    """Drive one locus generator to completion; returns its score list."""
    engine = engine or get_engine()
    try:
        req = next(gen)
        while True:
            ans = _answer(engine, [req], figure_fn)[0]
            req = gen.throw(ans) if isinstance(ans, BaseException) else gen.send(ans)
    except StopIteration as e:
        return e.value
    finally:
        wait = getattr(figure_fn, "wait", None)
        if wait is not None:
            wait()


def _prefetch_threads(n_gens: int) -> int:
    """Threads that start the loci of a batch (VAPOR_PREFETCH_THREADS; default up to 8, 1 = off)."""
    import os
    from . import seqio
    if n_gens < 16 or not getattr(seqio.get_backend(), "threads_ok", False) or os.environ.get("VAPOR_BAM_NATIVE", "1") == "0":
        return 1
    want = os.environ.get("VAPOR_PREFETCH_THREADS")
    if want is not None:
        return max(1, int(want))
    ranks_here = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))       # ranks sharing this host's cores (torchrun)
    return max(1, min(8, _usable_cores() // ranks_here))


def _usable_cores() -> int:
    """Cores this process may use: its affinity mask, cut to the container's CPU quota where there is one."""
    import os
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: (t.split()[0], t.split()[1])),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", lambda t: (t.strip(), open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read().strip()))):
        try:
            quota, period = parse(open(path).read())
            if quota not in ("max", "-1") and int(period) > 0:
                cores = max(1, min(cores, -(-int(quota) // int(period))))
            break
        except (OSError, ValueError, IndexError):
            continue
    return cores


def run_batch(gens: Sequence, engine=None, figure_fn: Optional[Callable] = None) -> List[object]:
    """Drive many locus generators in lockstep.  Returns, per generator, its score list or the
    exception it ended with."""
    engine = engine or get_engine()
    results: List[object] = [None] * len(gens)
    pending: Dict[int, object] = {}

    def advance(t, first=False, value=None):
        g = gens[t]
        try:
            if first:
                req = next(g)
            elif isinstance(value, BaseException):
                req = g.throw(value)
            else:
                req = g.send(value)
            pending[t] = req
        except StopIteration as e:
            results[t] = e.value
            pending.pop(t, None)
        except Exception as e:              # noqa: BLE001 - recorded for the caller to re-raise in order
            results[t] = e
            pending.pop(t, None)

    # A stretch of a locus generator holds its read extraction (window from the FASTA, reads of the region from the BAM:
    # BGZF inflation in the library's host helper, which releases the GIL) - the first stretch for the deletion and
    # insertion drivers, the one after the window refinements for the others (reads are fetched only when the windows
    # pass, CLI:334-367 via SF:1512-1530).  With a backend whose handles are per thread the generators of a batch advance on
    # a few threads, so that one locus inflates while another's Python runs.
    n_thr = _prefetch_threads(len(gens))
    pool = None
    if n_thr > 1:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=n_thr)

    def spread(work):
        """`work`: argument tuples of advance(); in slices over the pool (a future per item costs as much as a short stretch)."""
        if pool is None or len(work) < 16:
            for a in work:
                advance(*a)
            return
        step = max(1, len(work) // (n_thr * 8))

        def some(k):
            for a in work[k:k + step]:
                advance(*a)
        list(pool.map(some, range(0, len(work), step)))

    try:
        spread([(t, True) for t in range(len(gens))])
        while pending:
            idx = sorted(pending)
            ans = _answer(engine, [pending[t] for t in idx], figure_fn)
            spread([(t, False, a) for t, a in zip(idx, ans)])
    finally:
        if pool is not None:
            pool.shutdown(wait=True)
        wait = getattr(figure_fn, "wait", None)
        if wait is not None:
            wait()                                   # the batch's figures are on disk when it returns
    return results
