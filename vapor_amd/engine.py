"""Thin object layer over the C ABI: contexts, resident sequence sets and plans.

Device memory stays inside libvapor_hip.so; numpy arrays cross the boundary.
"""
from __future__ import annotations

import ctypes
import weakref
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


_utf8 = ctypes.pythonapi.PyUnicode_AsUTF8AndSize
_utf8.restype = ctypes.c_void_p
_utf8.argtypes = [ctypes.py_object, ctypes.POINTER(ctypes.c_ssize_t)]


def _ascii_data_offset() -> int:
    """Where the characters of a compact ASCII str lie relative to id(str) in this interpreter (measured, not assumed)."""
    probe = "ACGTACGTACGTACGT" * 4
    size = ctypes.c_ssize_t()
    p = _utf8(probe, ctypes.byref(size))
    return (p - id(probe)) if p and size.value == len(probe) else -1


_ASCII_OFF = _ascii_data_offset()


def _derived_lens(seg_first, segs) -> np.ndarray:
    """The lengths of derived sequences: the sum of each one's segment lengths."""
    dl = np.zeros(len(seg_first) - 1, dtype=np.int32)
    np.add.at(dl, np.repeat(np.arange(len(dl)), np.diff(seg_first)), segs["len"][:int(seg_first[-1])])
    return dl


def _as_bytes(s) -> bytes:
    return s if isinstance(s, (bytes, bytearray)) else s.encode("latin-1", "replace")


class DevRead:
    """A read whose bases are on the device already (Engine.bam_chop_device): `addr` the device address of the record's
    BAM-packed bases inside `batch` (kept alive by this object), `kind` 1 = the `length` bases from base `first` on, 2 = the
    reverse complement of the `length` bases that end at `first` (a right-anchored read).  It stands where a read's text
    stands in a Score request; a SeqSet takes it by address (vapor_seqset_create_mixed) - no base crosses the link."""
    __slots__ = ("addr", "first", "length", "kind", "batch")

    def __init__(self, addr, first, length, kind, batch):
        self.addr, self.first, self.length, self.kind, self.batch = int(addr), int(first), int(length), int(kind), batch

    def __len__(self):
        return self.length


class SeqSet:
    """Sequences packed on the device.  `n_exc[s]` = symbols outside upper-case ACGT,
    `n_invalid[s]` = symbols outside invert_base's alphabet after IUPAC folding."""

    def __init__(self, engine: "Engine", seqs: Sequence, upper: Optional[Sequence[bool]] = None, derived=None):
        """`derived`: sequences described instead of uploaded (include/vapor_hip.h, vapor_seqset_create_derived) - a list of
        (segments, upper) with segments = [(parent index into `seqs`, off, len, revcomp), ...]; derived sequence d is index
        len(seqs) + d of the set.  The device assembles their planes from the parents'."""
        self.engine = engine
        self.n_lit = len(seqs)
        self.n = len(seqs)
        n1 = max(self.n, 1)
        # One pointer per sequence, no concatenated copy: an ASCII str is handed over as it lies in memory (CPython
        # keeps it one byte per character; PyUnicode_AsUTF8AndSize returns that buffer), anything else as the
        # bytes it is or encodes to (characters outside Latin-1 become '?', which matches nothing anyway).
        keep = []
        self.lens = np.zeros(self.n, dtype=np.int32)
        size = ctypes.c_ssize_t()
        fast = (self.n > 64 and 0 < _ASCII_OFF < 256 and isinstance(seqs, (list, tuple)) and set(map(type, seqs)) == {str}
                and all(map(str.isascii, seqs)))
        src_kind = src_first = None           # (set when some sequences are DevRead: the set is a mixed one)
        if fast:
            # all ASCII str (the usual case): the characters of every one lie at the same offset behind the object, so the
            # pointers are id() + offset - four passes of map() instead of a ctypes call per sequence (2 200 sequences:
            # 1.1 ms -> 0.3 ms of a 2.4 ms upload)
            addr = np.fromiter(map(id, seqs), dtype=np.uint64, count=self.n) + np.uint64(_ASCII_OFF)
            self.lens = np.fromiter(map(len, seqs), dtype=np.int32, count=self.n)
            for t in (0, self.n // 2, self.n - 1):          # (spot check against the interpreter's own answer)
                if _utf8(seqs[t], ctypes.byref(size)) != int(addr[t]) or size.value != int(self.lens[t]):
                    fast = False
        if fast:
            ptrs = ctypes.cast(addr.ctypes.data, ctypes.POINTER(ctypes.c_void_p))
            keep.append(addr)
        else:
            ptrs = (ctypes.c_void_p * n1)()
        for t, sq in enumerate(() if fast else seqs):
            if type(sq) is DevRead:
                if src_kind is None:
                    src_kind, src_first = np.zeros(n1, dtype=np.uint8), np.zeros(n1, dtype=np.int64)
                ptrs[t] = sq.addr
                self.lens[t] = sq.length
                src_kind[t], src_first[t] = sq.kind, sq.first
                continue
            if isinstance(sq, str):
                p = _utf8(sq, ctypes.byref(size))
                if p and size.value == len(sq):
                    ptrs[t] = p
                    self.lens[t] = len(sq)
                    continue
                sq = sq.encode("latin-1", "replace")
            elif not isinstance(sq, bytes):
                sq = bytes(sq)
            keep.append(sq)
            ptrs[t] = ctypes.cast(ctypes.c_char_p(sq), ctypes.c_void_p).value
            self.lens[t] = len(sq)
        flags = np.zeros(n1, dtype=np.uint8)
        if upper is not None:
            flags[:self.n] = np.asarray(upper, dtype=bool).astype(np.uint8) * L.SEQ_UPPER
        h = ctypes.c_void_p()
        lib = L.load()
        lens = self.lens if self.n else np.zeros(1, np.int32)
        if derived or src_kind is not None:
            nd = len(derived) if derived else 0
            derived = derived or []
            if isinstance(derived, tuple) and len(derived) == 3 and isinstance(derived[0], np.ndarray):
                seg_first, segs, dflags = derived                      # (already as arrays: pipeline builds them in one go)
                nd = len(seg_first) - 1
            else:
                seg_first = np.zeros(nd + 1, dtype=np.int32)
                np.cumsum([len(sg) for sg, _u in derived], out=seg_first[1:])
                segs = np.zeros(max(int(seg_first[-1]), 1), dtype=L.SEG_DTYPE)
                w = 0
                for sg, _u in derived:
                    for par, off, ln, rc in sg:
                        segs[w] = (par, off, ln, L.SEG_REVCOMP if rc else 0)
                        w += 1
                dflags = np.asarray([L.SEQ_UPPER if u else 0 for _sg, u in derived] or [0], dtype=np.uint8)
            info = np.zeros(2 * max(self.n + nd, 1), dtype=np.int32)
            if src_kind is not None:
                L.check(lib.vapor_seqset_create_mixed(engine._ctx, self.n, ptrs, L.ptr(lens, ctypes.c_int32), L.ptr(flags, ctypes.c_uint8),
                                                      L.ptr(src_kind, ctypes.c_uint8), src_first.ctypes.data_as(ctypes.c_void_p), nd,
                                                      L.ptr(np.ascontiguousarray(seg_first, dtype=np.int32), ctypes.c_int32),
                                                      np.ascontiguousarray(segs, dtype=L.SEG_DTYPE).ctypes.data_as(ctypes.c_void_p),
                                                      L.ptr(np.ascontiguousarray(dflags, dtype=np.uint8), ctypes.c_uint8),
                                                      L.ptr(info, ctypes.c_int32), ctypes.byref(h)))
            else:
                L.check(lib.vapor_seqset_create_derived(engine._ctx, self.n, ptrs, L.ptr(lens, ctypes.c_int32), L.ptr(flags, ctypes.c_uint8),
                                                    nd, L.ptr(np.ascontiguousarray(seg_first, dtype=np.int32), ctypes.c_int32),
                                                    np.ascontiguousarray(segs, dtype=L.SEG_DTYPE).ctypes.data_as(ctypes.c_void_p),
                                                    L.ptr(np.ascontiguousarray(dflags, dtype=np.uint8), ctypes.c_uint8),
                                                    L.ptr(info, ctypes.c_int32), ctypes.byref(h)))
            self.lens = np.concatenate([self.lens[:self.n], _derived_lens(seg_first, segs)])
            self.n += nd
        else:
            info = np.zeros(2 * n1, dtype=np.int32)
            L.check(lib.vapor_seqset_create_ptrs(engine._ctx, self.n, ptrs, L.ptr(lens, ctypes.c_int32),
                                                 L.ptr(flags, ctypes.c_uint8), L.ptr(info, ctypes.c_int32), ctypes.byref(h)))
        del keep
        self._h = h
        engine._live.add(self)
        self.n_exc = info[0::2][:self.n].copy()
        self.n_invalid = info[1::2][:self.n].copy()

    @classmethod
    def from_addresses(cls, engine: "Engine", addr: np.ndarray, lens: np.ndarray, derived=None, keepalive=None,
                       src_kind=None, src_first=None) -> "SeqSet":
        """A set whose byte sequences are given as (address, length) pairs - slices of strings and buffers the caller keeps
        alive (`keepalive`) until this returns: a read is a slice of its record's sequence, a window a slice of its contig;
        nothing is copied on the Python side.  `derived` as (seg_first, segs, flags) arrays.  `src_kind` (uint8 per sequence;
        vapor_seqset_create_mixed): 1 where `addr` is the DEVICE address of BAM-packed bases inside a live BamBatch and the
        sequence the `lens` bases from base `src_first` on (Engine.bam_chop_device's reads); those never cross the link.  2: such
        a source taken reverse complemented - the complement of base `src_first`, then of the bases before it (its
        right-anchored reads)."""
        self = cls.__new__(cls)
        self.engine = engine
        self.n_lit = self.n = int(len(addr))
        addr = np.ascontiguousarray(addr, dtype=np.uint64)
        self.lens = np.ascontiguousarray(lens, dtype=np.int32)
        ptrs = ctypes.cast(addr.ctypes.data, ctypes.POINTER(ctypes.c_void_p))
        h = ctypes.c_void_p()
        lib = L.load()
        nd = 0
        if derived is not None:
            seg_first, segs, dflags = derived
            nd = len(seg_first) - 1
        info = np.zeros(2 * max(self.n + nd, 1), dtype=np.int32)
        lens_p = L.ptr(self.lens if self.n else np.zeros(1, np.int32), ctypes.c_int32)
        if src_kind is not None:
            kind = np.ascontiguousarray(src_kind, dtype=np.uint8)
            first = np.ascontiguousarray(src_first, dtype=np.int64)
            if len(kind) != self.n or len(first) != self.n:
                raise ValueError("src_kind / src_first: one entry per sequence")
            if nd:
                seg_first = np.ascontiguousarray(seg_first, dtype=np.int32)
                segs = np.ascontiguousarray(segs, dtype=L.SEG_DTYPE)
                dfl = np.ascontiguousarray(dflags, dtype=np.uint8)
            L.check(lib.vapor_seqset_create_mixed(engine._ctx, self.n, ptrs, lens_p, None, L.ptr(kind, ctypes.c_uint8), first.ctypes.data_as(ctypes.c_void_p),
                                                  nd, L.ptr(seg_first, ctypes.c_int32) if nd else None,
                                                  segs.ctypes.data_as(ctypes.c_void_p) if nd else None,
                                                  L.ptr(dfl, ctypes.c_uint8) if nd else None, L.ptr(info, ctypes.c_int32), ctypes.byref(h)))
        elif nd:
            seg_first = np.ascontiguousarray(seg_first, dtype=np.int32)
            segs = np.ascontiguousarray(segs, dtype=L.SEG_DTYPE)
            L.check(lib.vapor_seqset_create_derived(engine._ctx, self.n, ptrs, lens_p, None, nd, L.ptr(seg_first, ctypes.c_int32),
                                                    segs.ctypes.data_as(ctypes.c_void_p), L.ptr(np.ascontiguousarray(dflags, dtype=np.uint8), ctypes.c_uint8),
                                                    L.ptr(info, ctypes.c_int32), ctypes.byref(h)))
        else:
            L.check(lib.vapor_seqset_create_ptrs(engine._ctx, self.n, ptrs, lens_p, None, L.ptr(info, ctypes.c_int32), ctypes.byref(h)))
        if nd:
            self.lens = np.concatenate([self.lens, _derived_lens(seg_first, segs)])
            self.n += nd
        del keepalive
        self._h = h
        engine._live.add(self)
        self.n_exc = info[0::2][:self.n].copy()
        self.n_invalid = info[1::2][:self.n].copy()
        return self

    def planes(self, idx: int):
        """(p2, e1, x4) uint32 arrays of sequence `idx` as they lie in HBM: 2, 1 and 4 words per 32-symbol chunk."""
        ch = (int(self.lens[idx]) + 31) // 32
        p2, e1, x4 = np.zeros(2 * ch, np.uint32), np.zeros(ch, np.uint32), np.zeros(4 * ch, np.uint32)
        L.check(L.load().vapor_seqset_planes(self._h, int(idx), p2.ctypes.data_as(ctypes.c_void_p), e1.ctypes.data_as(ctypes.c_void_p),
                                             x4.ctypes.data_as(ctypes.c_void_p)))
        return p2, e1, x4

    def close(self) -> None:
        if self._h:
            L.load().vapor_seqset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BamBatch:
    """The inflated blocks of one vapor_bam_chop_device call on the device (the reads' packed bases lie in them)."""

    name_keys = None                # `--dedup-qname`: the name keys (seqio.name_key) of the call's entries, in their order (uint64)

    def __init__(self, handle):
        self._h = handle

    def read_name_keys(self, n: int) -> np.ndarray:
        """vapor_bam_batch_name_keys: the keys of the n entries the call that made this batch returned.  VaporHipError for a
        batch made without the option or by a tagged call; NotImplementedError where the library has no such entry."""
        fn = Engine._wide_entry("vapor_bam_batch_name_keys", "name keys of a device batch")
        keys = np.zeros(max(int(n), 1), dtype=np.uint64)
        L.check(fn(self._h, int(n), keys.ctypes.data_as(ctypes.c_void_p)))
        return keys[:int(n)]

    def close(self) -> None:
        if self._h:
            L.load().vapor_bam_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass


class Plan:
    def __init__(self, engine: "Engine", seqset: SeqSet, pairs: np.ndarray):
        self.engine = engine
        self.seqset = seqset
        self.pairs = np.ascontiguousarray(pairs, dtype=L.PAIR_DTYPE)
        self.n = len(self.pairs)
        h = ctypes.c_void_p()
        L.check(L.load().vapor_plan_create(engine._ctx, seqset._h, self.n, self.pairs.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.byref(h)))
        self._h = h
        engine._live.add(self)
        self.stats = np.zeros((max(self.n, 1), L.STATS_STRIDE), dtype=np.int64)

    def run(self) -> np.ndarray:
        """One pass of the hot path; returns the (n_pairs, 16) int64 statistics."""
        L.check(L.load().vapor_plan_run(self._h, L.ptr(self.stats, ctypes.c_int64)))
        return self.stats[:self.n]

    def timings(self) -> dict:
        ms = np.zeros(12, dtype=np.float64)
        L.check(L.load().vapor_plan_timings(self._h, L.ptr(ms, ctypes.c_double), 12))
        return {"join_ms": ms[0], "clean_ms": ms[1], "total_ms": ms[2], "join_launches": int(ms[3]),
                "retried_pairs": int(ms[4]), "finish_ms": ms[5], "pairs_served_by_shared_joins": int(ms[6]), "shared_joins": int(ms[7]),
                "clean_workgroups_per_cu": int(ms[8]), "remap_in_clean": int(ms[9]),
                # (of the task table the last run took, parameter join_align)
                "join_tasks": int(ms[10]), "table_builds": int(ms[11])}

    def record_counts(self) -> np.ndarray:
        """Run records per pair of the last run (the device stores runs of consecutive dots as one record)."""
        out = np.zeros(max(self.n, 1), dtype=np.int64)
        L.check(L.load().vapor_plan_record_counts(self._h, L.ptr(out, ctypes.c_int64)))
        return out[:self.n]

    def set_reads(self, reads: np.ndarray, n_loci: int) -> None:
        """Describe which pairs score which read of which locus (READ_DTYPE rows sorted by locus) so that
        run_loci() can finish on the device."""
        from . import finish
        self.reads = np.ascontiguousarray(reads, dtype=L.READ_DTYPE)
        self.n_loci = int(n_loci)
        L.check(L.load().vapor_plan_set_reads(self._h, len(self.reads), self.reads.ctypes.data_as(ctypes.c_void_p),
                                              self.n_loci, L.ptr(finish.gt_table(), ctypes.c_double)))
        self.loci = np.zeros((max(self.n_loci, 1), L.LOCUS_STRIDE), dtype=np.float64)
        self.read_scores = np.zeros(max(len(self.reads), 1), dtype=np.float64)

    def run_loci(self, device_out: int = 0, want_host: bool = True, want_scores: bool = False):
        """join -> clean -> finish on the device.  Returns the (n_loci, 8) float64 records
        [QS, GS, GT index, GQ, n scored, n positive, n rounding to <= 0, 0] (NaN row = 'NA'); with
        `device_out` (a device pointer, e.g. tensor.data_ptr()) they are also written there."""
        L.check(L.load().vapor_plan_run_loci(self._h, ctypes.c_void_p(device_out) if device_out else None,
                                             L.ptr(self.loci, ctypes.c_double) if want_host else None,
                                             L.ptr(self.read_scores, ctypes.c_double) if want_scores else None))
        return self.loci[:self.n_loci]

    def set_grid(self, first_locus: np.ndarray) -> None:
        """Breakpoint refinement (vapor_plan_set_grid): the plan's loci are candidates, group g the loci first_locus[g] ..
        first_locus[g + 1].  NotImplementedError when the loaded library has no refinement kernel (the CPU twin)."""
        fn = Engine._wide_entry("vapor_plan_set_grid", "refinement kernel")
        self.first_locus = np.ascontiguousarray(first_locus, dtype=np.int32)
        self.n_groups = len(self.first_locus) - 1
        L.check(fn(self._h, self.n_groups, L.ptr(self.first_locus, ctypes.c_int32)))

    def run_grid(self):
        """vapor_plan_run_grid: join -> clean -> finish -> the choice among each group's candidates, on the device.  Returns
        (winner index per group, (n_groups, 16) float64: the winner's record and candidate 0's, the winners' per-read scores,
        score_off (n_groups + 1,): group g's scores are winner_scores[score_off[g]:score_off[g + 1]])."""
        fn = Engine._wide_entry("vapor_plan_run_grid", "refinement kernel")
        ng = self.n_groups
        lf = np.zeros(self.n_loci + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.reads["locus"], minlength=self.n_loci), out=lf[1:])
        n_sc = int((lf[self.first_locus[:-1] + 1] - lf[self.first_locus[:-1]]).sum()) if ng else 0
        idx = np.zeros(max(ng, 1), dtype=np.int32)
        rec = np.zeros((max(ng, 1), 2 * L.LOCUS_STRIDE), dtype=np.float64)
        sc = np.zeros(max(n_sc, 1), dtype=np.float64)
        off = np.zeros(ng + 1, dtype=np.int64)
        L.check(fn(self._h, L.ptr(idx, ctypes.c_int32), L.ptr(rec, ctypes.c_double), L.ptr(sc, ctypes.c_double), L.ptr(off, ctypes.c_int64)))
        if int(off[ng]) != n_sc:
            raise RuntimeError("vapor_plan_run_grid: %d winner scores, %d expected" % (int(off[ng]), n_sc))
        return idx[:ng], rec[:ng], sc[:n_sc], off

    def run_loci_async(self, device_out: int = 0) -> None:
        """Enqueue join -> clean -> finish without waiting (after one run_loci(), which sizes the slots)."""
        L.check(L.load().vapor_plan_run_loci_async(self._h, ctypes.c_void_p(device_out) if device_out else None))

    def then(self, hip_stream: int) -> None:
        """Make `hip_stream` (a caller's stream) wait on the device for this plan's most recently enqueued step."""
        L.check(L.load().vapor_plan_then(self._h, ctypes.c_void_p(hip_stream)))

    def after(self, hip_stream: int) -> None:
        """Make this plan's next step wait for what has been enqueued on `hip_stream` so far."""
        L.check(L.load().vapor_plan_after(self._h, ctypes.c_void_p(hip_stream)))

    def sync(self, want_host: bool = True):
        """Wait for the enqueued steps; timings() then holds their averages.  Returns the last step's records."""
        L.check(L.load().vapor_plan_sync(self._h, L.ptr(self.loci, ctypes.c_double) if want_host else None))
        return self.loci[:self.n_loci]

    def algorithmic(self) -> Tuple[int, int]:
        b = ctypes.c_int64()
        c = ctypes.c_int64()
        L.check(L.load().vapor_plan_algorithmic_bytes(self._h, ctypes.byref(b), ctypes.byref(c)))
        return b.value, c.value

    def fetch_hits(self, idx: Iterable[int], want_flags: bool = True):
        """(hits (m,2) int32 [j,i], flags (m,) uint8 or None, off (len(idx)+1,) int64)."""
        idx = np.ascontiguousarray(list(idx), dtype=np.int64)
        off = np.zeros(len(idx) + 1, dtype=np.int64)
        if len(idx) == 0:
            return np.zeros((0, 2), np.int32), (np.zeros(0, np.uint8) if want_flags else None), off
        tot = int(self.stats[idx, L.ST_N_HITS][self.stats[idx, L.ST_STATUS] == 0].sum())
        hits = np.zeros((max(tot, 1), 2), dtype=np.int32)
        flags = np.zeros(max(tot, 1), dtype=np.uint8) if want_flags else None
        L.check(L.load().vapor_plan_fetch_hits(self._h, len(idx), L.ptr(idx, ctypes.c_int64), L.ptr(hits, ctypes.c_int32),
                                               L.ptr(flags, ctypes.c_uint8) if want_flags else None, tot,
                                               L.ptr(off, ctypes.c_int64)))
        return hits[:tot], (flags[:tot] if want_flags else None), off

    def close(self) -> None:
        if self._h:
            L.load().vapor_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One HIP context (device + stream).  Raises if the library or the GPU is missing."""

    def __init__(self, device: int = 0):
        lib = L.load()
        self._ctx = ctypes.c_void_p()
        L.check(lib.vapor_init(device, ctypes.byref(self._ctx)))
        self.device = device
        self._live = weakref.WeakSet()      # sequence sets and plans of this context: closed with it, plans first

    def set_param(self, name: str, value: int) -> None:
        L.check(L.load().vapor_set_param(self._ctx, name.encode(), int(value)))

    def set_stream(self, hip_stream: int) -> None:
        """Enqueue on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream); 0: the library's own."""
        L.check(L.load().vapor_set_stream(self._ctx, ctypes.c_void_p(hip_stream) if hip_stream else None))

    def seqset(self, seqs: Sequence, upper: Optional[Sequence[bool]] = None, derived=None) -> SeqSet:
        return SeqSet(self, seqs, upper, derived)

    def bam_chop_device(self, native_bam, tids, starts, ends, flanks, chunk_first, chunks, max_keep: int = 20, tagged: bool = False,
                        right: bool = False, sites=None, name_keys: bool = False):
        """vapor_bam_chop_device: the read selection of many regions of an open BAM file on the device.  Returns (kept_first,
        device addresses of the kept reads' packed bases, q0, miss_bp, status per region, BamBatch); the batch owns the data the
        addresses point into - close it after the sequence sets made from them.  tagged (`--phased`,
        vapor_bam_chop_device_tagged): the reads of a region are the union of its three group lists, and three more arrays
        follow the batch - member (uint32 per read), phase_set (int64 per region, phase.PS_NONE for none), tagged (per region);
        NotImplementedError where the library has no such entry (the CPU twin).  right (`--both-ends`,
        vapor_bam_chop_device_right): the right-anchored reads of every region - q0 is then the base a read's reverse complement
        starts with (SeqSet.from_addresses: src_kind 2) and miss_bp counts from the window end.  sites (`--phase-vcf`, with tagged;
        vapor_bam_chop_device_haplotag): the regions' phased sites as phase.device_site_tables makes them - the tags are then made
        on the device from them and the records' own HP / PS fields are not read.  name_keys (`--dedup-qname`, a handle with
        vapor_bam_set_dedup; not with tagged): the entries' name keys are put on the batch (batch.name_keys); the tuple keeps
        its shape."""
        if tagged and right:
            raise ValueError("right-anchored reads are not read with tags")
        if sites is not None and not tagged:
            raise ValueError("sites come with tagged=True")
        chop_fn = Engine._wide_entry("vapor_bam_chop_device_right", "right-anchored device reader") if right else None
        if tagged:
            tagged_fn = Engine._wide_entry("vapor_bam_chop_device_tagged", "tagged device reader")
            if sites is not None:
                tagged_fn = Engine._wide_entry("vapor_bam_chop_device_haplotag", "haplotagging device reader")
        n = len(tids)
        tids = np.ascontiguousarray(tids, dtype=np.int32)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        ends = np.ascontiguousarray(ends, dtype=np.int64)
        flanks = np.ascontiguousarray(flanks, dtype=np.int64)
        chunk_first = np.ascontiguousarray(chunk_first, dtype=np.int32)
        chunks = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1)
        if len(chunk_first) != n + 1 or len(chunks) != 2 * int(chunk_first[-1]):
            raise ValueError("chunk_first / chunks do not describe %d regions" % n)
        kept_first = np.zeros(n + 1, dtype=np.int32)
        cap = max(n * max_keep * (3 if tagged else 1), 1)
        addr = np.zeros(cap, dtype=np.uint64)
        q0 = np.zeros(cap, dtype=np.int64)
        miss = np.zeros(cap, dtype=np.int64)
        status = np.zeros(max(n, 1), dtype=np.int32)
        h = ctypes.c_void_p()
        vp = ctypes.c_void_p
        if tagged:
            member = np.zeros(cap, dtype=np.uint32)
            pset = np.zeros(max(n, 1), dtype=np.int64)
            tg = np.zeros(max(n, 1), dtype=np.int32)
            more = ()
            if sites is not None:
                site_first, ent, ps_first, ps_values = sites
                site_first = np.ascontiguousarray(site_first, dtype=np.int32)
                ps_first = np.ascontiguousarray(ps_first, dtype=np.int32)
                ent = np.ascontiguousarray(ent)
                ps_values = np.ascontiguousarray(ps_values, dtype=np.int64)
                if (len(site_first) != n + 1 or len(ps_first) != n + 1 or ent.dtype.itemsize != 8 or len(ent) != int(site_first[-1])
                        or len(ps_values) != int(ps_first[-1])):
                    raise ValueError("the site tables do not describe %d regions" % n)
                more = (site_first.ctypes.data_as(vp), ent.ctypes.data_as(vp) if len(ent) else None, ps_first.ctypes.data_as(vp),
                        ps_values.ctypes.data_as(vp) if len(ps_values) else None)
            L.check(tagged_fn(
                self._ctx, native_bam, n, tids.ctypes.data_as(vp), starts.ctypes.data_as(vp), ends.ctypes.data_as(vp),
                flanks.ctypes.data_as(vp), chunk_first.ctypes.data_as(vp), chunks.ctypes.data_as(vp) if len(chunks) else None,
                int(max_keep), kept_first.ctypes.data_as(vp), addr.ctypes.data_as(vp), q0.ctypes.data_as(vp), miss.ctypes.data_as(vp),
                member.ctypes.data_as(vp), pset.ctypes.data_as(vp), tg.ctypes.data_as(vp), status.ctypes.data_as(vp), ctypes.byref(h), *more))
            w = int(kept_first[n])
            return kept_first, addr[:w], q0[:w], miss[:w], status[:n], BamBatch(h), member[:w], pset[:n], tg[:n]
        L.check((chop_fn or L.load().vapor_bam_chop_device)(self._ctx, native_bam, n, tids.ctypes.data_as(vp), starts.ctypes.data_as(vp), ends.ctypes.data_as(vp),
                                               flanks.ctypes.data_as(vp), chunk_first.ctypes.data_as(vp), chunks.ctypes.data_as(vp) if len(chunks) else None,
                                               int(max_keep), kept_first.ctypes.data_as(vp), addr.ctypes.data_as(vp), q0.ctypes.data_as(vp),
                                               miss.ctypes.data_as(vp), status.ctypes.data_as(vp), ctypes.byref(h)))
        w = int(kept_first[n])
        batch = BamBatch(h)
        if name_keys:
            batch.name_keys = batch.read_name_keys(w)
        return kept_first, addr[:w], q0[:w], miss[:w], status[:n], batch

    def _bam_evidence_device(self, entry, what, native_bam, tids, rows, width, out_words, out_dtype, chunk_first, chunks, names=None, label="regions"):
        """One call of an evidence entry (vapor_bam_depth_device, _signature_device, _links_device, _support_device): rows is
        (n, width) int64, the answer (n, out_words) of out_dtype; names, for the entry that takes one, the call's byte blob."""
        fn = Engine._wide_entry(entry, what)
        n = len(tids)
        tids = np.ascontiguousarray(tids, dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        chunk_first = np.ascontiguousarray(chunk_first, dtype=np.int32)
        chunks = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1)
        if len(rows) != width * n or len(chunk_first) != n + 1 or len(chunks) != 2 * int(chunk_first[-1]):
            raise ValueError("%s / chunk_first / chunks do not describe %d regions" % (label, n))
        out = np.zeros(out_words * max(n, 1), dtype=out_dtype)
        status = np.zeros(max(n, 1), dtype=np.int32)
        vp = ctypes.c_void_p
        blob = () if names is None else (ctypes.c_char_p(bytes(names)), len(bytes(names)))
        L.check(fn(self._ctx, native_bam, n, tids.ctypes.data_as(vp), rows.ctypes.data_as(vp), *blob, chunk_first.ctypes.data_as(vp),
                   chunks.ctypes.data_as(vp) if len(chunks) else None, out.ctypes.data_as(vp), status.ctypes.data_as(vp)))
        return out[:out_words * n].reshape(n, out_words), status[:n]

    def bam_depth_device(self, native_bam, tids, bounds, chunk_first, chunks):
        """vapor_bam_depth_device (`--depth`): the read depth of many depth regions of an open BAM file on the
        device.  bounds: (n, 4) int64, chunk_first / chunks as in bam_chop_device.  Returns (cov, status): cov (n, 3) uint64,
        status per region - 0, or the code of a region that is the host route's (its sums are 0 then).  Nothing stays on the
        device.  NotImplementedError where the library has no such entry."""
        return self._bam_evidence_device("vapor_bam_depth_device", "device depth reader", native_bam, tids, bounds, 4, 3, np.uint64, chunk_first, chunks,
                                         label="bounds")

    def bam_signature_device(self, native_bam, tids, regions, chunk_first, chunks):
        """vapor_bam_signature_device (`--signatures`): split-read and CIGAR evidence of many signature regions
        of an open BAM file on the device.  regions: (n, 9) int64 - w0, w3, x0, x1, tol, min_clip, nmin, nmax, mask
        (signature.FIELDS); chunk_first / chunks as in bam_chop_device.  Returns (out, status): out (n, 10) int64 - the six
        counts, then offset and count of each target's mode - and status per region: 0, or the code of a region that is the host
        route's (its words are 0 then).  Nothing stays on the device.  NotImplementedError where the library has no such entry."""
        return self._bam_evidence_device("vapor_bam_signature_device", "device signature reader", native_bam, tids, regions, 9, 10, np.int64, chunk_first, chunks)

    def bam_links_device(self, native_bam, tids, regions, chunk_first, chunks, names=b""):
        """vapor_bam_links_device (`--links`): split reads joined through their SA tags, many link regions of an
        open BAM file on the device.  regions: (n, 11) int64 - w0, w3, x, y, tol, min_clip, ev, pend, rel (links.FIELDS), then
        offset and length of the partner contig's name in `names`, one byte blob for the call; chunk_first / chunks as in
        bam_chop_device.  Returns (out, status): out (n, 5) int64 - n_clip, n_split, n_link, offset and count of the mode - and
        status per region: 0, or the code of a region that is the host route's (its words are 0 then).  Nothing stays on the
        device.  NotImplementedError where the library has no such entry."""
        return self._bam_evidence_device("vapor_bam_links_device", "device links reader", native_bam, tids, regions, 11, 5, np.int64, chunk_first, chunks,
                                         names=names)

    def bam_support_device(self, native_bam, tids, regions, chunk_first, chunks):
        """vapor_bam_support_device (`--support`): alt and ref alignments of many support regions of an open BAM
        file on the device.  regions: (n, 11) int64 - signature.FIELDS, then flank and gmin (support.FIELDS); chunk_first /
        chunks as in bam_chop_device.  Returns (out, status): out (n, 7) int64 - alt_cg, alt_l, alt_r, ref_0, ref_1, cov_0,
        cov_1 - and status per region: 0, or the code of a region that is the host route's (its words are 0 then).  Nothing
        stays on the device.  NotImplementedError where the library has no such entry."""
        return self._bam_evidence_device("vapor_bam_support_device", "device support reader", native_bam, tids, regions, 11, 7, np.int64, chunk_first, chunks)

    def bam_last_stats(self) -> dict:
        """What this engine's last bam_chop_device did (vapor_bam_last_stats)."""
        out = np.zeros(7, dtype=np.float64)
        L.check(L.load().vapor_bam_last_stats(self._ctx, out.ctypes.data_as(ctypes.c_void_p), 7))
        return {"regions": int(out[0]), "blocks": int(out[1]), "compressed_bytes": int(out[2]), "inflated_bytes": int(out[3]),
                "inflate_ms": float(out[4]), "call_ms": float(out[5]), "d2h_bytes": int(out[6])}

    def fasta_windows_device(self, fd: int, vbeg, vend, text_cap: int):
        """vapor_fasta_windows_device: reference windows of a bgzipped FASTA (open descriptor `fd`), window i the raw text between
        the virtual offsets vbeg[i] and vend[i], inflated and cut on the device.  `text_cap`: the sum of the windows' raw sizes
        (or more).  Returns (texts: str per window, None where status != 0; traits: uint8 VAPOR_FASTA_TR_* bits; status: int32,
        0 or the VAPOR_FASTA_* reason the window is left to the host reader)."""
        vbeg = np.ascontiguousarray(vbeg, dtype=np.uint64)
        vend = np.ascontiguousarray(vend, dtype=np.uint64)
        n = len(vbeg)
        if len(vend) != n:
            raise ValueError("vbeg and vend differ in length")
        text = np.empty(max(int(text_cap), 1), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.int64)
        traits = np.zeros(max(n, 1), dtype=np.uint8)
        status = np.zeros(max(n, 1), dtype=np.int32)
        vp = ctypes.c_void_p
        L.check(L.load().vapor_fasta_windows_device(self._ctx, int(fd), n, vbeg.ctypes.data_as(vp), vend.ctypes.data_as(vp), text.ctypes.data_as(vp),
                                                    int(text_cap), off.ctypes.data_as(vp), traits.ctypes.data_as(vp), status.ctypes.data_as(vp)))
        raw = text[:int(off[n])].tobytes()
        o = off.tolist()
        st = status[:n]
        bad = st.tolist()
        texts = [None if bad[i] else raw[o[i]:o[i + 1]].decode("ascii") for i in range(n)]
        return texts, traits[:n], st

    def fasta_last_stats(self) -> dict:
        """What this engine's last fasta_windows_device did (vapor_fasta_last_stats)."""
        out = np.zeros(6, dtype=np.float64)
        L.check(L.load().vapor_fasta_last_stats(self._ctx, out.ctypes.data_as(ctypes.c_void_p), 6))
        return {"windows": int(out[0]), "blocks": int(out[1]), "compressed_bytes": int(out[2]), "inflated_bytes": int(out[3]),
                "kernel_ms": float(out[4]), "call_ms": float(out[5])}

    def seqset_raw(self, addr: np.ndarray, lens: np.ndarray, derived=None, keepalive=None, src_kind=None, src_first=None) -> SeqSet:
        """A set from (address, length) pairs - slices of strings the caller keeps alive - and derived sequences as arrays."""
        return SeqSet.from_addresses(self, addr, lens, derived, keepalive, src_kind, src_first)

    def plan(self, seqset: SeqSet, pairs: np.ndarray) -> Plan:
        return Plan(self, seqset, pairs)

    @staticmethod
    def make_pairs(rows: Sequence[Tuple[int, int, int, int, int]]) -> np.ndarray:
        a = np.zeros(len(rows), dtype=L.PAIR_DTYPE)
        for t, r in enumerate(rows):
            a[t] = tuple(r)
        return a

    def score(self, seqset: SeqSet, pairs: np.ndarray) -> np.ndarray:
        p = Plan(self, seqset, pairs)
        try:
            return p.run().copy()
        finally:
            p.close()

    def dotplots(self, seqset: SeqSet, pairs: np.ndarray) -> Tuple[np.ndarray, List[np.ndarray]]:
        """Statistics plus, per pair, the (n,2) [j,i] hit array sorted the way dotdata() lists it."""
        p = Plan(self, seqset, pairs)
        try:
            st = p.run().copy()
            hits, _f, off = p.fetch_hits(range(p.n), want_flags=False)
        finally:
            p.close()
        out = []
        for t in range(len(off) - 1):
            h = hits[off[t]:off[t + 1]]
            out.append(h[np.lexsort((h[:, 1], h[:, 0]))])
        return st, out

    def _clean_lists(self, fn, lists, flags):
        n = len(lists)
        arrs = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 2) for a in lists]
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(a) for a in arrs], out=off[1:])
        allh = np.concatenate(arrs + [np.zeros((1, 2), np.int32)])
        fl = np.asarray(flags if flags is not None else [3] * n, dtype=np.uint32)
        st = np.zeros((max(n, 1), 16), dtype=np.int64)
        hf = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
        L.check(fn(self._ctx, n, L.ptr(allh, ctypes.c_int32), L.ptr(off, ctypes.c_int64),
                   L.ptr(fl if n else np.zeros(1, np.uint32), ctypes.c_uint32), L.ptr(st, ctypes.c_int64), L.ptr(hf, ctypes.c_uint8)))
        return st[:n], [hf[off[t]:off[t + 1]] for t in range(n)]

    def clean_hits(self, lists: Sequence[np.ndarray], flags: Optional[Sequence[int]] = None):
        """Cleaning + reductions on explicit dot lists -> (stats (n,16), [flag bytes per list])."""
        return self._clean_lists(L.load().vapor_clean_hits, lists, flags)

    # ---- the optional entry points: the wide route (sequences up to MAX_WIDE_SEQ_LEN), the any-k route, refinement ----
    @staticmethod
    def _wide_entry(name: str, what: str = "wide route"):
        """An optional entry point of the loaded library - any of them, not the wide route's alone (the name is older than the
        others) - or NotImplementedError."""
        lib = L.load()
        # (the CPU twin of the C ABI exports the names with a stub that refuses every call: it has none of these routes either)
        flags = lib.vapor_build_flags() if hasattr(lib, "vapor_build_flags") else b""
        if not hasattr(lib, name) or "cpu-twin" in (flags or b"").decode().split(","):
            raise NotImplementedError("%s: the loaded library has no %s" % (name, what))
        return getattr(lib, name)

    def _available(self, *names: str) -> bool:
        try:
            for name in names:
                self._wide_entry(name)
        except NotImplementedError:
            return False
        return True

    def wide_available(self) -> bool:
        """Whether the loaded library has the wide route (the CPU twin of the C ABI has not)."""
        return self._available("vapor_wide_batch", "vapor_clean_hits_wide")

    def _score_dots(self, name: str, seqset: SeqSet, pairs: np.ndarray, want_hits: bool, sort: bool):
        fn = self._wide_entry(name)
        pairs = np.ascontiguousarray(pairs, dtype=L.PAIR_DTYPE)
        n = len(pairs)
        st = np.zeros((max(n, 1), 16), dtype=np.int64)
        off = np.zeros(n + 1, dtype=np.int64)
        pp = pairs.ctypes.data if n else None
        if not want_hits:
            L.check(fn(self._ctx, seqset._h, n, pp, L.ptr(st, ctypes.c_int64), None, 0, L.ptr(off, ctypes.c_int64)))
            return st[:n]
        cap = 1 << 16
        while True:
            hits = np.zeros((cap, 2), dtype=np.int32)
            rc = fn(self._ctx, seqset._h, n, pp, L.ptr(st, ctypes.c_int64), L.ptr(hits, ctypes.c_int32), cap,
                    L.ptr(off, ctypes.c_int64))
            if rc == L.E_OVERFLOW and int(off[n]) > cap:
                cap = int(off[n])
                continue
            L.check(rc)
            break
        out = [hits[off[t]:off[t + 1]] for t in range(n)]
        return st[:n], [h[np.lexsort((h[:, 1], h[:, 0]))] if sort else h.copy() for h in out]

    def score_wide(self, seqset: SeqSet, pairs: np.ndarray, want_hits: bool = False):
        """Statistics (n,16) of every pair on the wide route (vapor_wide_batch); with want_hits also, per pair, the (n,2) [j,i]
        hit array sorted the way dotdata() lists it."""
        return self._score_dots("vapor_wide_batch", seqset, pairs, want_hits, sort=True)

    def grid_available(self) -> bool:
        """Whether the loaded library has breakpoint refinement's device step (the CPU twin of the C ABI has not)."""
        return self._available("vapor_plan_set_grid", "vapor_plan_run_grid")

    def grid_pick(self, records: np.ndarray, first_locus, read_first, read_scores):
        """vapor_grid_pick: grid_pick_kernel on the caller's tables - (n, 8) candidate records, groups first_locus[g] ..
        first_locus[g + 1], candidate c's per-read scores read_scores[read_first[c]:read_first[c + 1]].  Returns what
        Plan.run_grid returns."""
        fn = self._wide_entry("vapor_grid_pick", "refinement kernel")
        rec = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, L.LOCUS_STRIDE)
        fl = np.ascontiguousarray(first_locus, dtype=np.int32)
        rf = np.ascontiguousarray(read_first, dtype=np.int32)
        sc = np.ascontiguousarray(read_scores, dtype=np.float64)
        ng = len(fl) - 1
        if len(rf) != len(rec) + 1 or int(fl[-1]) != len(rec) or (len(rf) and int(rf[-1]) != len(sc)):
            raise ValueError("grid_pick: the tables do not describe each other")
        n_sc = int((rf[fl[:-1] + 1] - rf[fl[:-1]]).sum()) if ng else 0
        idx = np.zeros(max(ng, 1), dtype=np.int32)
        out = np.zeros((max(ng, 1), 2 * L.LOCUS_STRIDE), dtype=np.float64)
        win = np.zeros(max(n_sc, 1), dtype=np.float64)
        off = np.zeros(ng + 1, dtype=np.int64)
        L.check(fn(self._ctx, ng, L.ptr(fl, ctypes.c_int32), L.ptr(rec if len(rec) else np.zeros((1, 8)), ctypes.c_double), L.ptr(rf, ctypes.c_int32),
                   L.ptr(sc if len(sc) else np.zeros(1), ctypes.c_double), L.ptr(idx, ctypes.c_int32), L.ptr(out, ctypes.c_double),
                   L.ptr(win, ctypes.c_double), L.ptr(off, ctypes.c_int64)))
        return idx[:ng], out[:ng], win[:n_sc], off

    # ---- the any-k route: kmerhits at every k from 1 to MAX_ANY_K ----
    def anyk_available(self) -> bool:
        """Whether the loaded library has the any-k route (the CPU twin of the C ABI has not)."""
        return self._available("vapor_anyk_batch")

    def score_anyk(self, seqset: SeqSet, pairs: np.ndarray, want_hits: bool = False):
        """Statistics (n,16) of every pair on the any-k route (vapor_anyk_batch: k from 1 to MAX_ANY_K, PF_FORWARD for
        kmerhits(..., inversions=False)); with want_hits also, per pair, the (n,2) [j,i] hit array in the reference's order."""
        return self._score_dots("vapor_anyk_batch", seqset, pairs, want_hits, sort=False)

    # ---- `--realign`: the banded edit distance of every pair ----
    def realign_available(self) -> bool:
        """Whether the loaded library has vapor_realign_batch (the CPU twin of the C ABI has not)."""
        return self._available("vapor_realign_batch")

    def realign(self, seqset: SeqSet, pairs: np.ndarray, band: int):
        """(d, status) of every pair, two int32 arrays (vapor_realign_batch): d the edit distance of seq1 against seq2[off2:]
        inside the band, start anchored, both ends free - -1 where status is E_ARG.  A pair's k and flags are ignored.
        NotImplementedError where the library has no such entry: there is no other route."""
        fn = self._wide_entry("vapor_realign_batch", "realignment kernel (--realign)")
        pairs = np.ascontiguousarray(pairs, dtype=L.PAIR_DTYPE)
        n = len(pairs)
        out = np.zeros((max(n, 1), 2), dtype=np.int32)
        L.check(fn(self._ctx, seqset._h, n, pairs.ctypes.data if n else None, int(band), L.ptr(out, ctypes.c_int32)))
        return out[:n, 0].copy(), out[:n, 1].copy()

    # ---- `--realign-out`: the alignment behind the distance ----
    def realign_trace_available(self) -> bool:
        """Whether the loaded library has vapor_realign_trace (the CPU twin of the C ABI has not)."""
        return self._available("vapor_realign_trace")

    def realign_trace(self, seqset: SeqSet, pairs: np.ndarray, band: int, cap_runs: int):
        """(head, runs) of every pair (vapor_realign_trace): head an (n, 8) int32 array, a row {d, status, i_end, j_end, n_runs,
        0, 0, 0}; runs an (n, cap_runs) uint32 array, a pair's runs (len << 2 | op; 0 '=', 1 'X', 2 'I', 3 'D') the last n_runs
        words of its row, in path order (realign.runs_of reads them).  status is E_OVERFLOW for a pair that needs more than
        cap_runs runs - n_runs says how many - and E_ARG, with d = -1, for a pair the entry refuses.
        NotImplementedError where the library has no such entry: there is no other route."""
        fn = self._wide_entry("vapor_realign_trace", "traceback kernel (--realign-out)")
        pairs = np.ascontiguousarray(pairs, dtype=L.PAIR_DTYPE)
        n, cap = len(pairs), int(cap_runs)
        head = np.zeros((max(n, 1), 8), dtype=np.int32)
        runs = np.zeros((max(n, 1), max(cap, 1)), dtype=np.uint32)
        L.check(fn(self._ctx, seqset._h, n, pairs.ctypes.data if n else None, int(band), cap, L.ptr(head, ctypes.c_int32),
                   L.ptr(runs, ctypes.c_uint32)))
        return head[:n], runs[:n]

    # ---- `--realign-polish`: the consensus of a locus's pairs on its allele ----
    def realign_polish_available(self) -> bool:
        """Whether the loaded library has vapor_realign_polish (the CPU twin of the C ABI has not)."""
        return self._available("vapor_realign_polish")

    def _polish_marshal(self, who, seqset, pairs, band, tables, want_counts):
        """What the calls of vapor_realign_polish and vapor_realign_revote share: (args, outs, tabs, pairs) - the entries' thirteen
        leading arguments; the five outputs behind them, cut to the call's loci and columns; `tables` (first, col_off and what
        the entry has beside them, one entry a locus and one more each) as int64 arrays; and the pair table `args` points into."""
        from . import polish
        pairs = np.ascontiguousarray(pairs, dtype=L.PAIR_DTYPE)
        tabs = [np.ascontiguousarray(t, dtype=np.int64) for t in tables]
        if any(len(t) != len(tabs[0]) for t in tabs) or len(tabs[0]) < 1:
            raise ValueError("%s hold one entry a locus and one more" % who)
        n, ng = len(pairs), len(tabs[0]) - 1
        cols = max(int(tabs[1][-1]), 0)
        stats = np.zeros((max(ng, 1), 8), dtype=np.int32)
        calls = np.zeros(max(cols, 1), dtype=np.uint8)
        sites = np.zeros((max(ng, 1), polish.MAX_SITES, 2), dtype=np.int32)
        ins = np.zeros((max(ng, 1), polish.MAX_SITES, polish.RMAX), dtype=np.uint8)
        counts = np.zeros((max(cols, 1), 8), dtype=np.uint32) if want_counts else None
        args = (self._ctx, seqset._h, n, pairs.ctypes.data if n else None, int(band), ng, L.ptr(tabs[0], ctypes.c_int64),
                L.ptr(tabs[1], ctypes.c_int64), L.ptr(stats, ctypes.c_int32), L.ptr(calls, ctypes.c_uint8), L.ptr(sites, ctypes.c_int32),
                L.ptr(ins, ctypes.c_uint8), L.ptr(counts, ctypes.c_uint32) if want_counts else None)
        return args, (stats[:ng], calls[:cols], sites[:ng], ins[:ng], counts[:cols] if want_counts else None), tabs, pairs

    def realign_polish(self, seqset: SeqSet, pairs: np.ndarray, band: int, first, col_off, want_counts: bool = False):
        """(stats, calls, sites, ins, counts) of every locus (vapor_realign_polish): the pairs of locus g are first[g] ..
        first[g + 1], all against the locus's allele, whose columns are col_off[g] .. col_off[g + 1].  stats (n_loci, 8) int32,
        a row {status, pairs piled, PCOV, PSUB, PDEL, sites kept, PINS, sites dropped}; calls one uint8 a column; sites
        (n_loci, 256, 2) int32, a kept site's (column, bases); ins (n_loci, 256, 64) uint8, its text; counts (columns, 8) uint32
        with want_counts, else None (polish.statement says what they hold).  A locus the entry refuses has status E_ARG or
        E_NOMEM, zero statistics and every column KEEP.
        NotImplementedError where the library has no such entry: there is no other route."""
        fn = self._wide_entry("vapor_realign_polish", "pileup kernels (--realign-polish)")
        args, outs, _tabs, _pairs = self._polish_marshal("realign_polish: first and col_off", seqset, pairs, band, (first, col_off), want_counts)
        L.check(fn(*args))
        return outs

    # ---- `--realign-revote`: every read against the polished allele ----
    def realign_revote_available(self) -> bool:
        """Whether the loaded library has vapor_realign_revote (the CPU twin of the C ABI has not)."""
        return self._available("vapor_realign_revote")

    def realign_revote(self, seqset: SeqSet, pairs: np.ndarray, band: int, first, col_off, votes: np.ndarray, vfirst,
                       want_counts: bool = False, want_spelt: bool = False, spelt_off=None):
        """(stats, calls, sites, ins, counts, vout, lout, spelt_off, spelt) of every locus (vapor_realign_revote): realign_polish's
        five, bit for bit, and the second alignment behind them.  The vote pairs of locus g are votes[vfirst[g] .. vfirst[g + 1]),
        seq1 the read, seq2 the locus's allele, off2 in the called allele's columns.  vout (n_votes, 4) int32, a row {d_pol,
        status, off2', m'}; lout (n_loci, 4) int32, a row {vstatus, plen, 0, 0} (revote.statement says what they hold).  With
        want_spelt, spelt is a uint8 array that holds the plen codes of locus g from spelt_off[g] on - slots of the largest
        polished allele a locus can have unless `spelt_off` gives others -; else both are None.
        NotImplementedError where the library has no such entry: there is no other route."""
        from . import polish
        fn = self._wide_entry("vapor_realign_revote", "re-vote kernels (--realign-revote)")
        args, outs, (_fl, co, vf), _pairs = self._polish_marshal("realign_revote: first, col_off and vfirst", seqset, pairs, band,
                                                                 (first, col_off, vfirst), want_counts)
        votes = np.ascontiguousarray(votes, dtype=L.PAIR_DTYPE)
        nv, ng = len(votes), len(vf) - 1
        vout = np.zeros((max(nv, 1), 4), dtype=np.int32)
        lout = np.zeros((max(ng, 1), 4), dtype=np.int32)
        so = spelt = None
        if want_spelt:
            if spelt_off is None:
                span = np.diff(co)
                spelt_off = np.concatenate(([0], np.cumsum(span + polish.RMAX * np.minimum(span, polish.MAX_SITES))))
            so = np.ascontiguousarray(spelt_off, dtype=np.int64)
            if len(so) != len(vf):
                raise ValueError("realign_revote: spelt_off holds one entry a locus and one more")
            spelt = np.zeros(max(int(so.max()), 1), dtype=np.uint8)
        L.check(fn(*args, nv, votes.ctypes.data if nv else None, L.ptr(vf, ctypes.c_int64), L.ptr(vout, ctypes.c_int32),
                   L.ptr(lout, ctypes.c_int32), L.ptr(so, ctypes.c_int64) if want_spelt else None,
                   L.ptr(spelt, ctypes.c_uint8) if want_spelt else None))
        return outs + (vout[:nv], lout[:ng], so, spelt)

    # ---- `--realign-junction`: the one jump between the two sequences of a pair ----
    def realign_junction_available(self) -> bool:
        """Whether the loaded library has vapor_realign_junction (the CPU twin of the C ABI has not)."""
        return self._available("vapor_realign_junction")

    def realign_junction(self, seqset: SeqSet, pairs: np.ndarray, band: int, want_rows: bool = False):
        """(out, row_off, rows) of every pair (vapor_realign_junction): seq1 the shorter sequence, seq2 the longer, off2 0.  out an
        (n, 8) int32 array, a row {status, cost, i, j1, j2, f_F(i), f_R(ns - i), 0}: seq1 is seq2 with seq2[j1:j2] skipped at
        row i, at `cost` further edits (junction.junction says it in numpy); status E_ARG and zeros for a pair the entry refuses.
        With want_rows, rows is a (row_off[-1], 4) int32 array whose rows row_off[t] .. row_off[t + 1] are pair t's
        {f_F, jf_F, f_R, jf_R} (junction.row_table), len(seq1) + 1 of them; else row_off and rows are None.
        NotImplementedError where the library has no such entry: there is no other route."""
        fn = self._wide_entry("vapor_realign_junction", "junction kernels (--realign-junction)")
        pairs = np.ascontiguousarray(pairs, dtype=L.PAIR_DTYPE)
        n = len(pairs)
        out = np.zeros((max(n, 1), 8), dtype=np.int32)
        row_off = rows = None
        if want_rows:
            lens = np.asarray(seqset.lens, dtype=np.int64)
            s1 = np.asarray(pairs["seq1"], dtype=np.int64)
            ok = (s1 >= 0) & (s1 < len(lens))
            need = np.where(ok, lens[np.where(ok, s1, 0)] + 1, 0) if n else np.zeros(0, dtype=np.int64)
            row_off = np.concatenate(([0], np.cumsum(need))).astype(np.int64)
            rows = np.zeros((max(int(row_off[-1]), 1), 4), dtype=np.int32)
        L.check(fn(self._ctx, seqset._h, n, pairs.ctypes.data if n else None, int(band), L.ptr(out, ctypes.c_int32),
                   L.ptr(row_off, ctypes.c_int64) if want_rows else None, L.ptr(rows, ctypes.c_int32) if want_rows else None))
        return out[:n], row_off, rows[:int(row_off[-1])] if want_rows else None

    def clean_hits_wide(self, lists: Sequence[np.ndarray], flags: Optional[Sequence[int]] = None):
        """clean_hits for lists with coordinates up to MAX_WIDE_SEQ_LEN (vapor_clean_hits_wide)."""
        return self._clean_lists(self._wide_entry("vapor_clean_hits_wide"), lists, flags)

    def close(self) -> None:
        if self._ctx:
            live = list(self._live)
            for obj in sorted(live, key=lambda o: isinstance(o, SeqSet)):
                obj.close()
            L.load().vapor_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
