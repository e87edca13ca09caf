"""Reference/read extraction around an SV window (component #3).

The reference shells out to samtools twice or more per locus and parses the text
(`ref_seq_readin` SF:1203-1217, `chop_pacbio_read_by_pos` SF:339-354).  Here the same
text protocol is served by a pluggable backend so that whole shards of loci can be
prepared in-process before anything goes to the GPU:

* `SamtoolsCLI`     - the real `samtools faidx` / `samtools view` (when installed);
* `MemorySamtools`  - an in-memory world (`vapor_amd.synth.SynthWorld`) answering the
                      same two queries with the same line formats.

The trimming rules (POS filter, CIGAR walk, miss_bp cut, 20-read cap) keep the
reference's semantics exactly; they are host-side integer/string work.
"""
from __future__ import annotations

import os
import threading
import re
import shutil
import subprocess
from typing import Iterable, List, Optional

_backend = None


class _EvidenceMany:
    """The four evidence readers of a backend (`--depth`, `--signatures`, `--links`, `--support`) by
    their public names: per region (chroms[g], rows[g]: the module's FIELDS; depth: the four bounds; links: partners[g] the
    partner contig's name) the module's words - depth [cov0, cov1, cov2], signatures ten, links five, support seven.  Each
    hands its rule module to the backend's one _evidence_many(module, engine, bam, chroms, rows, partners=None), which reads
    the regions as the module's reader surface says and holds them to module.statement."""

    def depth_many(self, engine, bam: str, chroms, bounds):
        from . import depth
        return self._evidence_many(depth, engine, bam, chroms, bounds)

    def signature_many(self, engine, bam: str, chroms, regions):
        from . import signature
        return self._evidence_many(signature, engine, bam, chroms, regions)

    def links_many(self, engine, bam: str, chroms, regions, partners):
        from . import links
        return self._evidence_many(links, engine, bam, chroms, regions, partners)

    def support_many(self, engine, bam: str, chroms, regions):
        from . import support
        return self._evidence_many(support, engine, bam, chroms, regions)


def _sam_records(module, fields_of_lines) -> list:
    """The alignment lines of `view` as module.statement's records: (POS, operations), with FLAG and the SA field for a module
    whose records are LINKED."""
    from .depth import parse_cigar
    if not module.LINKED:
        return [(int(f[3]), parse_cigar(f[5])) for f in fields_of_lines]
    from .links import sa_of_sam
    return [(int(f[3]), parse_cigar(f[5]), int(f[1]), sa_of_sam(f[11:])) for f in fields_of_lines]


class SamtoolsCLI(_EvidenceMany):
    """Runs the samtools binary; raises if it is missing instead of yielding nothing."""

    # `--min-mapq`, `--exclude-flags`: (min_mapq, exclude_flags) - a record is filtered iff MAPQ < min_mapq or
    # FLAG & exclude_flags, and a filtered record is as if it were not in the file.  view_lines lists what `samtools view` lists;
    # the lines are filtered on columns 2 and 5 where they are read (_sam_fields)
    read_filter = (0, 0)
    # `--dedup-qname`: among the kept records of one (file, region, anchor kind) one per QNAME survives
    # (dedup_kept); the SAM text readers take FLAG from column 2
    dedup_qname = False

    def __init__(self, exe: str = "samtools") -> None:
        self.exe = shutil.which(exe)
        if self.exe is None:
            raise RuntimeError("samtools not found on PATH; install it or select "
                               "vapor_amd.seqio.MemorySamtools via set_backend()")

    def faidx_lines(self, ref: str, region: str) -> Iterable[str]:
        p = subprocess.run([self.exe, "faidx", ref, region], capture_output=True, text=True)
        return p.stdout.splitlines()

    def view_lines(self, bam: str, region: str) -> Iterable[str]:
        p = subprocess.run([self.exe, "view", bam, region], capture_output=True, text=True)
        return p.stdout.splitlines()

    def isfile(self, path: str) -> bool:
        return os.path.isfile(path)

    def fai_lines(self, ref: str) -> Iterable[str]:
        with open(ref + ".fai") as f:
            return f.read().splitlines()

    # `--depth`: the length every bound of a depth region is clipped to, and the regions' sums
    def contig_length(self, bam: str, ref: str, chrom: str) -> int:
        """From the reference's .fai; 0 for a contig it does not list."""
        cache = self.__dict__.setdefault("_fai_len", {})
        if ref not in cache:
            cache[ref] = {f[0]: int(f[1]) for f in (ln.split("\t") for ln in self.fai_lines(ref)) if len(f) > 1}
        return cache[ref].get(chrom, 0)

    def _evidence_many(self, module, engine, bam: str, chroms, rows, partners=None):
        """module.statement over the alignment lines of `view`, filtered where they are read (_sam_fields) with module.EXCLUDE
        among the excluded flags; the entries' mapQ (links) meets the filter's minimum MAPQ."""
        lo, hi = module.WINDOW
        out = []
        for g, (chrom, row) in enumerate(zip(chroms, rows)):
            if not row[hi] > row[lo]:
                out.append(list(module.ZERO))
                continue
            recs = _sam_records(module, _sam_fields(self, bam, chrom, int(row[lo]) + 1, int(row[hi]), module.EXCLUDE))
            out.append(module.statement(recs, row, partners[g] if partners is not None else None, getattr(self, "read_filter", (0, 0))[0]))
        return out


class FaiFasta:
    """In-process `samtools faidx ref chrom:start-end` through the .fai index (no process per locus)."""

    def __init__(self, path: str):
        self.path = path
        self.index = {}
        with open(path + ".fai") as f:
            for ln in f:
                t = ln.rstrip("\n").split("\t")
                if len(t) >= 5:
                    self.index[t[0]] = (int(t[1]), int(t[2]), int(t[3]), int(t[4]))
        self._fh = open(path, "rb")

    def fetch(self, chrom: str, start: int, end: int) -> str:
        """1-based inclusive, clipped to the contig like samtools."""
        if chrom not in self.index:
            return ""
        length, offset, linebases, linewidth = self.index[chrom]
        start = max(int(start), 1)
        end = min(int(end), length)
        if end < start:
            return ""
        a, b = start - 1, end
        first = offset + (a // linebases) * linewidth + a % linebases
        last = offset + ((b - 1) // linebases) * linewidth + (b - 1) % linebases + 1
        raw = os.pread(self._fh.fileno(), last - first, first)      # (positioned read: several threads may fetch at once)
        return raw.replace(b"\n", b"").replace(b"\r", b"").decode("ascii")

    def lines(self, region: str) -> List[str]:
        """`samtools faidx` text: header line, then the sequence in lines of 60."""
        chrom, _, span = region.rpartition(":")
        if not chrom:
            chrom, a, b = region, 1, self.index.get(region, (0,))[0]
        else:
            a, _, b = span.partition("-")
            a, b = int(a.replace(",", "")), int(b.replace(",", ""))
        seq = self.fetch(chrom, a, b)
        return [">" + region] + [seq[i:i + 60] for i in range(0, len(seq), 60)]


class BgzfFasta:
    """FaiFasta for a bgzip-compressed FASTA (`samtools faidx ref.fa.gz`): the .fai geometry applied to the uncompressed stream,
    found through the .gzi block table (htslib's: a little-endian uint64 count, then (compressed, uncompressed) offset pairs
    of the blocks after the first; without a .gzi the same table is built in memory by walking the block headers).  Blocks are
    inflated by the library's host decoder and checked by their CRC-32 and size; a damaged block raises.  A small cache of
    inflated blocks; positioned reads, so that several threads may fetch at once."""

    CACHE_BLOCKS = 64

    def __init__(self, path: str):
        import numpy as np
        self.path = path
        self.index = {}
        with open(path + ".fai") as f:
            for ln in f:
                t = ln.rstrip("\n").split("\t")
                if len(t) >= 5:
                    self.index[t[0]] = (int(t[1]), int(t[2]), int(t[3]), int(t[4]))
        self._fh = open(path, "rb")
        self._fd = self._fh.fileno()
        if not is_bgzf(path):
            raise ValueError(_not_bgzf_msg(path))
        gzi = path + ".gzi"
        if os.path.exists(gzi):
            raw = open(gzi, "rb").read()
            cnt = int.from_bytes(raw[:8], "little") if len(raw) >= 8 else -1
            if cnt < 0 or len(raw) != 8 + 16 * cnt:
                raise ValueError("%s is not a BGZF index (.gzi)" % gzi)
            pairs = np.frombuffer(raw, dtype="<u8", count=2 * cnt, offset=8).reshape(-1, 2)
            coff, uoff = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
        else:
            coff, uoff = self._walk()
        self.coff = np.concatenate(([0], coff)).astype(np.int64)        # (the first block's (0, 0) is implicit)
        self.uoff = np.concatenate(([0], uoff)).astype(np.int64)
        self._cache = {}
        self._lock = threading.Lock()

    def _walk(self):
        """The .gzi table from the block headers (BSIZE and ISIZE; nothing is inflated)."""
        import numpy as np
        size = os.fstat(self._fd).st_size
        c, u = 0, 0
        cs, us = [], []
        while c < size:
            bsize = _bgzf_bsize(os.pread(self._fd, 512, c))
            tail = os.pread(self._fd, 4, c + bsize - 4) if bsize else b""
            if bsize is None or len(tail) < 4:
                raise ValueError("%s: no whole BGZF block at offset %d" % (self.path, c))
            c += bsize
            u += int.from_bytes(tail, "little")
            if c < size:
                cs.append(c)
                us.append(u)
        return np.asarray(cs, dtype=np.int64), np.asarray(us, dtype=np.int64)

    def _header(self, coff: int, hdr: bytes = None):
        """(BSIZE, CRC32, ISIZE) of the block at `coff`; raises for anything that is not a whole BGZF block."""
        if hdr is None:
            hdr = os.pread(self._fd, 65536, coff)
        bsize = _bgzf_bsize(hdr)
        if bsize is None or len(hdr) < bsize:
            raise ValueError("%s: no whole BGZF block at offset %d" % (self.path, coff))
        crc = int.from_bytes(hdr[bsize - 8:bsize - 4], "little")
        isize = int.from_bytes(hdr[bsize - 4:bsize], "little")
        if isize > 65536:
            raise ValueError("%s: BGZF block at offset %d claims %d bytes (at most 65536)" % (self.path, coff, isize))
        return bsize, crc, isize

    def block(self, k: int) -> bytes:
        """The data of block k of the table, inflated and checked."""
        coff = int(self.coff[k])
        got = self._cache.get(coff)
        if got is not None:
            return got
        import ctypes
        from . import _lib
        raw = os.pread(self._fd, 65536, coff)
        bsize, crc, isize = self._header(coff, raw)
        xlen = raw[10] | (raw[11] << 8)
        payload = raw[12 + xlen:bsize - 8]
        lib = _lib.load()
        out = ctypes.create_string_buffer(max(isize, 1))
        if lib.vapor_inflate_raw(payload, len(payload), out, isize) != 0:
            raise ValueError("%s: BGZF block at offset %d does not inflate to its %d bytes" % (self.path, coff, isize))
        data = out.raw[:isize]
        if (lib.vapor_crc32(data, isize, 0) if isize else 0) != crc:
            raise ValueError("%s: BGZF block at offset %d fails its CRC32 check" % (self.path, coff))
        with self._lock:
            if len(self._cache) >= self.CACHE_BLOCKS:
                self._cache.clear()
            self._cache[coff] = data
        return data

    def raw_range(self, chrom: str, start: int, end: int):
        """[first, last) of the window's raw text (newlines included) in the uncompressed stream, or None: FaiFasta.fetch's
        clipping (1-based inclusive, clipped to the contig; unknown contig or empty range: None)."""
        if chrom not in self.index:
            return None
        length, offset, linebases, linewidth = self.index[chrom]
        start = max(int(start), 1)
        end = min(int(end), length)
        if end < start:
            return None
        a, b = start - 1, end
        first = offset + (a // linebases) * linewidth + a % linebases
        last = offset + ((b - 1) // linebases) * linewidth + (b - 1) % linebases + 1
        return first, last

    def block_of(self, u):
        """Index of the block that holds uncompressed offset u (an array of them too)."""
        import numpy as np
        return np.searchsorted(self.uoff, u, side="right") - 1

    def virtual(self, u):
        """Virtual offsets (compressed block offset << 16 | offset in its data) of uncompressed offsets u (numpy arrays); a
        position past a block's 64 KB cannot be said that way and comes back as -1."""
        import numpy as np
        u = np.asarray(u, dtype=np.int64)
        k = self.block_of(u)
        w = u - self.uoff[k]
        return np.where(w < 65536, (self.coff[k] << 16) | w, -1)

    def read_raw(self, first: int, last: int) -> bytes:
        k0, k1 = int(self.block_of(first)), int(self.block_of(last - 1))
        parts = []
        for k in range(k0, k1 + 1):
            d = self.block(k)
            u0 = int(self.uoff[k])
            parts.append(d[max(first - u0, 0):last - u0])
        raw = b"".join(parts)
        if len(raw) != last - first:
            raise ValueError("%s: the BGZF blocks hold %d of the %d bytes at offset %d" % (self.path, len(raw), last - first, first))
        return raw

    def fetch(self, chrom: str, start: int, end: int) -> str:
        """1-based inclusive, clipped to the contig like samtools."""
        r = self.raw_range(chrom, start, end)
        if r is None:
            return ""
        return self.read_raw(*r).replace(b"\n", b"").replace(b"\r", b"").decode("ascii")

    lines = FaiFasta.lines


def _bgzf_bsize(hdr: bytes):
    """BSIZE of the BGZF block whose header starts `hdr`, or None when it is not one (gzip with the BC extra field)."""
    if len(hdr) < 18 or hdr[:4] != b"\x1f\x8b\x08\x04":
        return None
    xlen = hdr[10] | (hdr[11] << 8)
    p = 12
    while p + 4 <= 12 + xlen and p + 4 <= len(hdr):
        slen = hdr[p + 2] | (hdr[p + 3] << 8)
        if hdr[p] == 66 and hdr[p + 1] == 67 and slen == 2 and p + 6 <= len(hdr):
            bsize = (hdr[p + 4] | (hdr[p + 5] << 8)) + 1
            return bsize if bsize >= xlen + 20 else None
        p += 4 + slen
    return None


def is_bgzf(path: str) -> bool:
    with open(path, "rb") as f:
        return _bgzf_bsize(f.read(512)) is not None


def _not_bgzf_msg(path: str) -> str:
    return ("%s is gzip-compressed but not BGZF: a FASTA must be compressed with `bgzip` (and indexed with `samtools faidx`) "
            "to be read by region" % path)


def open_fasta(path: str):
    """The reader for a FASTA with its .fai: BgzfFasta for a bgzip-compressed file (its first block a gzip member with the BC
    extra field), FaiFasta for plain text.  Any other gzip file raises."""
    try:
        with open(path, "rb") as f:
            head = f.read(512)
    except OSError:
        return FaiFasta(path)             # (which raises as it always has)
    if head[:2] == b"\x1f\x8b":
        if _bgzf_bsize(head) is None:
            raise ValueError(_not_bgzf_msg(path))
        return BgzfFasta(path)
    return FaiFasta(path)


def write_bgzf_fasta(path: str, contigs, line_width: int = 60, block_size: int = 65280, crlf: bool = False) -> str:
    """A bgzipped FASTA of `contigs` (name -> sequence, or (name, sequence) pairs) with the .fai `samtools faidx` writes for it
    (uncompressed offsets) and the .gzi of its blocks; blocks of `block_size` uncompressed bytes (bgzip's 65 280 by default)
    and the BGZF end-of-file block.  Returns `path`."""
    import struct
    from . import bamio
    items = list(contigs.items()) if hasattr(contigs, "items") else list(contigs)
    nl = "\r\n" if crlf else "\n"
    text, fai = [], []
    off = 0
    for name, seq in items:
        hdr = ">" + name + nl
        off += len(hdr)
        text.append(hdr)
        fai.append("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), off, line_width, line_width + len(nl)))
        body = "".join(seq[i:i + line_width] + nl for i in range(0, len(seq), line_width))
        text.append(body)
        off += len(body)
    data = "".join(text).encode("ascii")
    gzi = []
    c = 0
    with open(path, "wb") as f:
        for u in range(0, len(data), block_size):
            if u:
                gzi.append((c, u))
            blk = bamio._bgzf_block(data[u:u + block_size])
            f.write(blk)
            c += len(blk)
        if data:
            gzi.append((c, len(data)))             # (as htslib indexes it: an entry for every block after the first, the EOF block's too)
        f.write(bamio._BGZF_EOF)
    with open(path + ".fai", "w") as f:
        f.write("".join(fai))
    with open(path + ".gzi", "wb") as f:
        f.write(struct.pack("<Q", len(gzi)) + b"".join(struct.pack("<QQ", a, b) for a, b in gzi))
    return path


class SamtoolsHybrid(SamtoolsCLI):
    """samtools for the BAM, the .fai index read in-process for the reference windows: one process per
    locus instead of two or more."""

    def __init__(self, exe: str = "samtools") -> None:
        super().__init__(exe)
        self._fa = {}

    def faidx_lines(self, ref: str, region: str) -> Iterable[str]:
        fa = self._fa.get(ref)
        if fa is None:
            if not os.path.exists(ref + ".fai"):
                return super().faidx_lines(ref, region)
            fa = self._fa[ref] = open_fasta(ref)
        return fa.lines(region)


# The scheduler of the device readers' calls: InProcessBam.chop_many_device and ._evidence_many hand their
# regions' .bai chunks to the three functions below and keep only what is theirs - the windows, the arguments of a call, and
# what becomes of an answer and of a region no call takes.
def _flat_chunks(chunk_lists):
    """The regions' chunk lists as the arrays a device reader takes: (chunk_first, flat_a) - chunk_first int32 of len + 1, region
    k's chunks are flat_a[chunk_first[k]:chunk_first[k + 1]]; flat_a uint64 of shape (m, 2), a chunk's two virtual offsets a
    row.  A region without chunks is an empty range; no region at all is ([0], shape (0, 2))."""
    import numpy as np
    chunk_first = np.zeros(len(chunk_lists) + 1, dtype=np.int32)
    flat = []
    for k, chunks in enumerate(chunk_lists):
        for c in chunks:
            flat.append(c[0])
            flat.append(c[1])
        chunk_first[k + 1] = len(flat) >> 1
    return chunk_first, np.asarray(flat, dtype=np.uint64).reshape(-1, 2)


def _size_groups(chunk_first, flat_a):
    """The regions cut into the groups [(a, e), ...] of one call each, in order and without a gap.  One call holds the blocks of
    all its regions on the device at once, compressed and inflated: a region counts (end >> 16) - (begin >> 16) + 65600
    compressed bytes a chunk (the file range and a last block), and a group always takes its first region and a further one
    only while the sum stays within VAPOR_BAM_DEVICE_BATCH_MB (default 192, read at every call; in MB of 2^20 bytes) - the
    inflated data of such a group stays far below the library's 2 GB a call."""
    import numpy as np
    n = len(chunk_first) - 1
    comp = np.zeros(n, dtype=np.int64)
    if len(flat_a):
        per_chunk = ((flat_a[:, 1] >> np.uint64(16)) - (flat_a[:, 0] >> np.uint64(16))).astype(np.int64) + 65600
        np.add.at(comp, np.repeat(np.arange(n), np.diff(chunk_first)), per_chunk)
    cap = int(os.environ.get("VAPOR_BAM_DEVICE_BATCH_MB", "192")) << 20
    groups = []
    a = 0
    while a < n:
        e, tot = a, 0
        while e < n and (e == a or tot + int(comp[e]) <= cap):
            tot += int(comp[e])
            e += 1
        groups.append((a, e))
        a = e
    return groups


def _run_groups(groups, call):
    """call(a, e) for every group, from the front: yields (a, e, what the call returned).  A group the library refuses for its
    size (a VaporHipError that says "in one call") goes back to the front as its halves [a, (a + e) // 2) and [(a + e) // 2, e);
    a single region refused so - its blocks alone are more than a call takes - is yielded as (a, a + 1, None), the host
    route's.  Every other error passes through."""
    from . import _lib
    groups = list(groups)
    while groups:
        a, e = groups.pop(0)
        try:
            got = call(a, e)
        except _lib.VaporHipError as err:
            if "in one call" not in str(err):
                raise
            if e - a >= 2:
                groups[:0] = [(a, (a + e) // 2), ((a + e) // 2, e)]
                continue
            got = None
        yield a, e, got


class InProcessBam(SamtoolsHybrid):
    """BAM and BAI read in-process as well (vapor_amd.bamio): no process per locus at all, and the records reach
    the trimming code as fields, not as text to be split again.  The default backend."""

    threads_ok = True                  # pipeline.run_batch may start loci on several threads (native chop, positioned reads)
    chunk_threads_ok = True            # cli.score_jobs may score several chunks at once, a thread each
    phase_sites = None                 # `--phase-vcf`: the phase.Sites a tagged chop of this backend makes its (hap, ps) from
    # (read_filter, inherited: `--min-mapq`, `--exclude-flags` - every open file carries it, bamio.BamFile.set_filter)

    def __init__(self) -> None:        # noqa: D401 - does not require the samtools binary
        self.exe = None
        self._fa = {}
        self._bam = {}
        self._open_lock = threading.Lock()

    def _open(self, bam: str):
        from . import bamio
        b = self._bam.get(bam)
        if b is None:
            with self._open_lock:
                b = self._bam.get(bam)
                if b is None:
                    b = self._bam[bam] = bamio.BamFile(bam)
        if b.read_filter != self.read_filter:          # (the run's read filter, DESIGN.md 4.17: the file and its native handles carry it)
            b.set_filter(*self.read_filter)
        if b.dedup_qname != bool(self.dedup_qname):    # (`--dedup-qname`, DESIGN.md 4.18: likewise)
            b.set_dedup(self.dedup_qname)
        return b

    def view_lines(self, bam: str, region: str) -> Iterable[str]:
        chrom, _, span = region.rpartition(":")
        a, _, e = span.partition("-")
        return self._open(bam).fetch_lines(chrom, int(a), int(e))

    def records(self, bam: str, chrom: str, start: int, end: int, flags: bool = False):
        """(QNAME, POS, CIGAR, SEQ) per alignment overlapping chrom:start-end; with flags also FLAG."""
        return [r if flags else r[:4] for r in self._open(bam).fetch_records(chrom, int(start), int(end))]

    def chop(self, bam: str, chrom: str, start: int, end: int, flank_length: int, tagged: bool = False, right: bool = False, sites=None):
        """chop_pacbio_read_by_pos (SF:339-354) straight from the BAM file: the library's native reader
        (vapor_bam_chop), or with VAPOR_BAM_NATIVE=0 the Python statement of the same steps below.  `tagged` (`--phased`):
        every entry is [read, miss_bp, qname, hap, ps] (vapor_bam_chop_tagged; vapor_amd.phase has the tag rule) - with sites
        (`--phase-vcf`: a phase.Sites, the argument or this backend's phase_sites) hap and ps are phase.haplotag's from the
        locus's phased sites (vapor_bam_chop_haplotag) and the records' tags are not read.  `right`
        (`--both-ends`): the right-anchored reads (vapor_bam_chop_right, or _chop_records over the records as text)."""
        if tagged and sites is None:
            sites = self.phase_sites
        b = self._open(bam)
        # (a library without vapor_bam_set_filter does not filter: a run with a filter goes through the Python statement then)
        # (nor does one without vapor_bam_set_dedup de-duplicate)
        native = not _env_is(b"VAPOR_BAM_NATIVE", b"0") and b.native_filter_ok() and b.native_dedup_ok()
        if right:
            if native:
                from . import _lib
                if hasattr(_lib.load(), "vapor_bam_chop_right"):
                    return b.chop_native(chrom, int(start), int(end), int(flank_length), right=True)
            dd = bool(self.dedup_qname)
            return _chop_records(self.records(bam, chrom, start, end, flags=dd), int(start), int(end), flank_length, right=True, dedup=dd)
        st = {"sites": sites} if tagged and sites is not None else {}
        if native:
            return b.chop_native(chrom, int(start), int(end), int(flank_length), tagged=tagged, **st)
        return self.chop_python(bam, chrom, start, end, flank_length, tagged=tagged, **st)

    def chop_many(self, bam: str, chroms, starts, ends, flanks, max_keep: int = 20, groups: bool = False, sites=None):
        """MemorySamtools.chop_many's contract from a BAM file: every region through the library's native reader (vapor_bam_chop:
        threaded inflate, binary CIGAR walk, only the kept bases decoded) on a few threads, the kept reads of a region as slices
        of ONE text per region - (kept_first, addr, q0 = 0, miss, status, keepalive).  minimize_pacbio_read_list (SF:1091-1102)
        on the numbers: the first max_keep in a stable order by miss_bp.  groups (`--phased`): through vapor_bam_chop_tagged,
        with the selection of phase.select_numbers - see MemorySamtools.chop_many; with sites (`--phase-vcf`, as in chop)
        through vapor_bam_chop_haplotag."""
        import numpy as np
        from .engine import _ASCII_OFF
        if _env_is(b"VAPOR_BAM_NATIVE", b"0") or not (0 < _ASCII_OFF < 256):
            raise NotImplementedError("chop_many needs the native reader")
        if groups and sites is None:
            sites = self.phase_sites
        st_kw = {"sites": sites} if groups and sites is not None else {}
        n = len(chroms)
        b = self._open(bam)
        if not b.native_filter_ok():
            raise NotImplementedError("the loaded library has no read filter")
        if not b.native_dedup_ok():
            raise NotImplementedError("the loaded library does not de-duplicate by QNAME")
        st, en, fl = [int(x) for x in starts], [int(x) for x in ends], [int(x) for x in flanks]

        def one(g):
            try:
                return b.chop_native_raw(chroms[g], st[g], en[g], fl[g], tagged=groups, **st_kw)
            except IndexError:
                return IndexError                       # (a record without CIGAR: the drivers' route raises it where the reference does)
        from . import pipeline
        n_thr = pipeline._prefetch_threads(n)
        if n_thr > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=n_thr) as pool:
                got = list(pool.map(one, range(n), chunksize=max(1, n // (n_thr * 8))))
        else:
            got = [one(g) for g in range(n)]
        kept_first = np.zeros(n + 1, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        pa, pm, keep = [], [], []
        w = 0
        if groups:
            from . import phase
            member, pset, tagged = [], np.full(n, phase.PS_NONE, dtype=np.int64), np.zeros(n, dtype=np.int32)
        for g, r in enumerate(got):
            kept_first[g] = w
            if r is IndexError:
                status[g] = -4
                continue
            if r is None:
                continue
            whole, off, ln, miss = r[:4]
            if groups:
                tagged[g], pset[g], order, words = phase.select_numbers(miss, r[4], r[5], max_keep)
                order = np.asarray(order, dtype=np.int64)
                member += words
            else:
                order = np.arange(len(off))
            if not groups and len(order) > max_keep:
                order = np.argsort(miss, kind="stable")[:max_keep]
            keep.append(whole)
            pa.append((off[order] + (id(whole) + _ASCII_OFF)).astype(np.uint64))
            pm.append(miss[order])
            w += len(order)
        kept_first[n] = w
        addr = np.concatenate(pa) if pa else np.zeros(0, dtype=np.uint64)
        miss_a = np.concatenate(pm).astype(np.int64) if pm else np.zeros(0, dtype=np.int64)
        if groups:
            return kept_first, addr, np.zeros(w, dtype=np.int64), miss_a, status, keep, np.asarray(member, dtype=np.uint32), pset, tagged
        return kept_first, addr, np.zeros(w, dtype=np.int64), miss_a, status, keep

    def chop_many_device(self, engine, bam: str, chroms, starts, ends, flanks, max_keep: int = 20, groups: bool = False,
                         right: bool = False, sites=None):
        """chop_many with the work on the device (vapor_bam_chop_device: the regions' BGZF blocks go over the link compressed,
        one wavefront inflates a block, one walks a region's records): (kept_first, DEVICE addresses of the kept reads' packed
        bases, q0 = first base of each read's part, miss, status, keepalive).  A region the device leaves to the host route
        (status != 0: a damaged block, a record without CIGAR, ...) is answered by the caller's per-locus route, which words
        the reference's errors.  groups (`--phased`): vapor_bam_chop_device_tagged - the reads of a region are the union of its
        three group lists, selected on the device; member, phase set and tagged follow as in MemorySamtools.chop_many.  right
        (`--both-ends`): the right-anchored reads of every region (vapor_bam_chop_device_right) - q0 is then the base a read's
        reverse complement starts with: such a read goes into a sequence set with src_kind 2.  sites (`--phase-vcf`, with
        groups; as in chop): vapor_bam_chop_device_haplotag - the tags behind the selection are made on the device from every
        region's phased sites (phase.device_site_tables); a region with more phase sets than a wavefront tallies comes back
        with a status, for the host route."""
        import numpy as np
        if _env_is(b"VAPOR_BAM_NATIVE", b"0") or _env_is(b"VAPOR_BAM_DEVICE", b"0") or not hasattr(engine, "bam_chop_device"):
            raise NotImplementedError("no device reader")
        from . import _lib
        lib = _lib.load()
        if not hasattr(lib, "vapor_bam_chop_device"):
            raise NotImplementedError("no device reader")
        phased = bool(groups)                 # (`groups` below is the list of region batches)
        more = {"tagged": True} if phased else {"right": True} if right else {}
        if right and (phased or not hasattr(lib, "vapor_bam_chop_device_right")):
            raise NotImplementedError("no right-anchored device reader")
        b = self._open(bam)
        if not b.native_filter_ok():
            raise NotImplementedError("the loaded library has no read filter")
        if not b.native_dedup_ok():
            raise NotImplementedError("the loaded library does not de-duplicate by QNAME")
        if b.dedup_qname and not phased:
            # (the entries' name keys come back on every batch, BamBatch.name_keys: rule V of `--both-ends` compares them)
            if not hasattr(lib, "vapor_bam_batch_name_keys"):
                raise NotImplementedError("the loaded library has no name keys")
            more["name_keys"] = True
        n = len(chroms)
        if phased and sites is None:
            sites = self.phase_sites
        tables = None
        if phased and sites is not None:
            if not hasattr(lib, "vapor_bam_chop_device_haplotag"):
                raise NotImplementedError("no haplotagging device reader")
            from . import phase
            tables = phase.device_site_tables(sites, chroms, starts, ends)
        # (a region on a contig the file does not have: tid 0 and no chunk)
        tid_of = [b.tid.get(c) for c in chroms]
        tids = np.asarray([t or 0 for t in tid_of], dtype=np.int32)
        index_chunks = b.index.chunks
        chunk_first, flat_a = _flat_chunks([index_chunks(t, max(int(starts[g]) - 1, 0), int(ends[g])) if t is not None else ()
                                            for g, t in enumerate(tid_of)])

        def call(a, e):
            c0, c1 = int(chunk_first[a]), int(chunk_first[e])
            if tables is not None:                  # (the batch's slice of the site tables, its offsets from zero)
                sf, ent, pf, psv = tables
                more["sites"] = (sf[a:e + 1] - sf[a], ent[int(sf[a]):int(sf[e])], pf[a:e + 1] - pf[a], psv[int(pf[a]):int(pf[e])])
            return engine.bam_chop_device(tl["native"], tids[a:e], starts[a:e], ends[a:e], flanks[a:e], chunk_first[a:e + 1] - c0,
                                          flat_a[c0:c1].reshape(-1), max_keep, **more)
        parts, batches = [], []
        with b.handle(lib) as tl:
            try:
                for a, e, got in _run_groups(_size_groups(chunk_first, flat_a), call):
                    if got is None:
                        # one region whose blocks alone are more than a call takes: the host route's (it streams them)
                        parts.append((np.zeros(2, dtype=np.int32), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64),
                                      np.zeros(0, dtype=np.int64), np.ones(1, dtype=np.int32), np.zeros(0, dtype=np.uint32),
                                      np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32)))
                        continue
                    parts.append(got[:5] + got[6:])
                    batches.append(got[5])
            except BaseException:
                # (whatever ends the run early: the batches so far are closed here, on the thread that made them)
                for bt in batches:
                    bt.close()
                raise
        kf = np.zeros(n + 1, dtype=np.int32)
        w = 0
        g = 0
        for p in parts:
            m = len(p[0]) - 1
            kf[g:g + m + 1] = p[0] + w
            w += int(p[0][-1])
            g += m
        cat = lambda k, dt: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, dtype=dt)    # noqa: E731
        if phased:
            return kf, cat(1, np.uint64), cat(2, np.int64), cat(3, np.int64), cat(4, np.int32), batches, cat(5, np.uint32), cat(6, np.int64), cat(7, np.int32)
        return kf, cat(1, np.uint64), cat(2, np.int64), cat(3, np.int64), cat(4, np.int32), batches

    def contig_length(self, bam: str, ref: str, chrom: str) -> int:
        """(`--depth`) l_ref of the BAM header; 0 for a contig the file does not have."""
        b = self._open(bam)
        t = b.tid.get(chrom)
        return int(b.refs[t][1]) if t is not None else 0

    def _evidence_many(self, module, engine, bam: str, chroms, rows, partners=None):
        """The routes of the evidence readers over a BAM file.  The regions go to the device in groups by compressed size
        (_size_groups), a group the library refuses for its size ("in one call") in halves (_run_groups; module.ENTRIES[1] through the
        Engine's module.DEVICE: one wavefront a region); a region the device hands back with a status - for links one with a
        record whose aux area is malformed among them -, and every region with VAPOR_BAM_DEVICE=0 or without a device reader,
        goes to the native host reader (the BamFile's module.NATIVE).  A library without the entries, one without the read
        filter the file carries, or VAPOR_BAM_NATIVE=0: the Python statement, module.statement over fetch_raw (LINKED:
        fetch_links) with module.EXCLUDE added to the excluded flags.  A region on an unknown contig or with an empty walk
        window [row[lo], row[hi]) is module.ZERO.  `engine`: an Engine, or None for the one of pipeline.get_engine() when the
        device is asked.  partners (links): the native readers do not know contig names - the partners' go as one byte blob,
        every name once, handed to the device and the native entry as their `names`, and each region's row ends in its
        name's offset and length."""
        width, (lo, hi) = module.ROW_WIDTH, module.WINDOW
        more = {}
        if partners is not None:
            where, blob, rows = {}, bytearray(), [list(r) for r in rows]
            for row, pc in zip(rows, partners):
                name = pc.encode("latin-1") if isinstance(pc, str) else bytes(pc)
                if name not in where:
                    where[name] = len(blob)
                    blob += name
                row += [where[name], len(name)]
            more["names"] = names = bytes(blob)

        def python(b, chrom, row):
            if module.LINKED:
                recs = b.fetch_links(chrom, int(row[lo]) + 1, int(row[hi]), exclude_more=module.EXCLUDE)
            else:
                recs = [(r[1], r[2]) for r in b.fetch_raw(chrom, int(row[lo]) + 1, int(row[hi]), exclude_more=module.EXCLUDE)]
            partner = names[int(row[-2]):int(row[-2]) + int(row[-1])] if partners is not None else None
            return module.statement(recs, row, partner, b.read_filter[0])
        zero, entries, device, native = module.ZERO, module.ENTRIES, module.DEVICE, module.NATIVE
        import numpy as np
        from . import _lib
        n = len(chroms)
        b = self._open(bam)
        bounds = np.ascontiguousarray(rows, dtype=np.int64).reshape(n, width)
        out = [list(zero) for _ in range(n)]
        todo = [g for g in range(n) if chroms[g] in b.tid and bounds[g][hi] > bounds[g][lo]]
        lib = _lib.load()
        if _env_is(b"VAPOR_BAM_NATIVE", b"0") or not hasattr(lib, entries[0]) or not b.native_filter_ok():
            for g in todo:
                out[g] = python(b, chroms[g], bounds[g])
            return out
        tid_of, index_chunks = b.tid, b.index.chunks
        chunks_of = {g: index_chunks(tid_of[chroms[g]], int(bounds[g][lo]), int(bounds[g][hi])) for g in todo}
        host = todo
        flags = lib.vapor_build_flags() or b""
        if (todo and not _env_is(b"VAPOR_BAM_DEVICE", b"0") and hasattr(lib, entries[1])
                and b"cpu-twin" not in flags.split(b",")):
            if engine is None:
                from . import pipeline
                engine = pipeline.get_engine()
        else:
            engine = None
        if engine is not None and hasattr(engine, device):
            host = []
            tids = np.asarray([tid_of[chroms[g]] for g in todo], dtype=np.int32)
            chunk_first, flat_a = _flat_chunks([chunks_of[g] for g in todo])
            bt = bounds[todo]

            def call(a, e):
                c0, c1 = int(chunk_first[a]), int(chunk_first[e])
                return getattr(engine, device)(tl["native"], tids[a:e], bt[a:e], chunk_first[a:e + 1] - c0, flat_a[c0:c1].reshape(-1), **more)
            with b.handle(lib) as tl:
                for a, e, got in _run_groups(_size_groups(chunk_first, flat_a), call):
                    if got is None:
                        host.append(todo[a])              # (one region whose blocks alone are more than a call takes)
                        continue
                    cov, status = got
                    for k in range(a, e):
                        if status[k - a]:
                            host.append(todo[k])
                        else:
                            out[todo[k]] = [int(x) for x in cov[k - a]]
        for g in host:
            out[g] = getattr(b, native)(tid_of[chroms[g]], bounds[g], chunks_of[g], **more)
        return out

    def isfile(self, path: str) -> bool:
        # (bam_in_decide, SF:69-89, asks once per locus: a file this reader holds open is a file - no stat, and no release of
        # the interpreter lock around one, for the loci after the first)
        return path in self._bam or os.path.isfile(path)

    def chop_python(self, bam: str, chrom: str, start: int, end: int, flank_length: int, tagged: bool = False, sites=None):
        """The same from the records as Python parses them: the CIGAR is walked in its binary form (the library's
        host helper) and only the reads that are kept have their bases decoded.  sites (with tagged: a phase.Sites): the
        tags are phase.haplotag's from the locus's sites (bamio's fetch_raw)."""
        import ctypes
        import numpy as np
        from . import _lib, bamio
        walk = _lib.load().vapor_cigar2alignstart_ops
        res = np.zeros(2, dtype=np.int64)
        res_p = res.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        out = []
        flags = []
        rows = {"sites": sites.rows(chrom, int(start), int(end))} if tagged and sites is not None else {}
        for qname, pos, cig, sq, l_seq, flag, tags in self._open(bam).fetch_raw(chrom, int(start), int(end), **rows):
            if not pos < start + 1:
                continue
            ops = np.ascontiguousarray(cig, dtype=np.uint32)
            rc = walk(ops.ctypes.data, len(ops), int(pos), int(start), res_p)
            if rc != 0:
                raise IndexError("string index out of range")  # what '' [1] raises in SF:331 for a record without CIGAR
            q0, miss_bp = int(res[0]), int(res[1])
            if not miss_bp > flank_length / 2:
                seq = bamio._decode_seq(sq, l_seq) or "*"
                tail = seq[q0:]
                want = end - start - miss_bp
                if len(tail) > want:
                    out.append([tail[:want], miss_bp, qname] + (list(tags) if tagged else []))
                    flags.append(flag)
        return dedup_kept(out, flags) if self.dedup_qname else out

    def _fasta(self, ref: str):
        fa = self._fa.get(ref)
        if fa is None:
            with self._open_lock:
                fa = self._fa.get(ref)
                if fa is None:
                    fa = self._fa[ref] = open_fasta(ref)
        return fa

    def faidx_lines(self, ref: str, region: str) -> Iterable[str]:
        return self._fasta(ref).lines(region)

    def fetch_seq(self, ref: str, chrom: str, start: int, end: int) -> str:
        return self._fasta(ref).fetch(chrom, start, end)


class MemorySamtools(_EvidenceMany):
    # cli.score_jobs may score several chunks at once, a thread each: the native chop writes to arrays of the call's own
    # (not with VAPOR_MEMORY_CHOP=records: that path's CIGAR walk answers into one module-level array, see cli._chunk_threads_ok)
    chunk_threads_ok = True
    phase_sites = None                 # `--phase-vcf`: the phase.Sites a tagged chop of this backend makes its (hap, ps) from
    # `--min-mapq`, `--exclude-flags`: every list of records below holds the records that pass (_recs)
    read_filter = (0, 0)
    # `--dedup-qname`: every chop below applies rule W to the records it keeps (dedup_kept)
    dedup_qname = False

    """Answers faidx/view from a `SynthWorld`; file names are ignored."""

    def __init__(self, world) -> None:
        self.world = world

    def _recs(self, chrom: str):
        """The contig's records that pass the read filter: the world's own list without a filter, else a list made once per
        (record list, filter)."""
        recs = self.world.reads.get(chrom, ())
        q, f = self.read_filter
        if not (q or f) or not recs:
            return recs
        cache = self.__dict__.setdefault("_filter_cache", {})
        got = cache.get(id(recs))
        if got is None or got[0] is not recs or got[1] != (q, f, len(recs)):
            from .bamio import record_passes
            got = (recs, (q, f, len(recs)), [r for r in recs if record_passes(r.mapq, r.flag, q, f)])
            if getattr(self.world, "cache_ok", True):
                if len(cache) > 200000:
                    cache.clear()
                cache[id(recs)] = got
        return got[2]

    def _overlapping(self, chrom: str, start: int, end: int):
        """world.overlapping over the records that pass."""
        q, f = self.read_filter
        recs = self.world.overlapping(chrom, start, end)
        if not (q or f):
            return recs
        from .bamio import record_passes
        return [r for r in recs if record_passes(r.mapq, r.flag, q, f)]

    @staticmethod
    def _region(region: str):
        chrom, _, span = region.rpartition(":")
        if not chrom:
            return region, None, None
        a, _, b = span.partition("-")
        return chrom, int(a), int(b)

    def faidx_lines(self, ref: str, region: str) -> Iterable[str]:
        chrom, a, b = self._region(region)
        if a is None:
            seq = self.world.contigs.get(chrom, "")
        else:
            seq = self.world.fetch(chrom, a, b) if chrom in self.world.contigs else ""
        out = [">" + region]
        out.extend(seq[i:i + 60] for i in range(0, len(seq), 60))
        return out

    def view_lines(self, bam: str, region: str) -> Iterable[str]:
        chrom, a, b = self._region(region)
        return [r.line() for r in self._overlapping(chrom, a, b)]

    def records(self, bam: str, chrom: str, start: int, end: int, flags: bool = False):
        if flags:
            return [(r.qname, r.pos, r.cigar, r.seq, r.flag) for r in self._overlapping(chrom, int(start), int(end))]
        return [(r.qname, r.pos, r.cigar, r.seq) for r in self._overlapping(chrom, int(start), int(end))]

    def fetch_seq(self, ref: str, chrom: str, start: int, end: int) -> str:
        return self.world.fetch(chrom, start, end) if chrom in self.world.contigs else ""

    # chop_pacbio_read_by_pos in one native call per region: the contig's records as small arrays (positions, spans, read
    # lengths, pointers to the CIGAR texts - made once per record list; nothing is parsed ahead: the walk reads a CIGAR only as
    # far as the window start), the region rule / CIGAR walk / keep rules in the library's host helper (vapor_chop_records),
    # only the kept reads sliced here.  The per-record path (records + cigar2alignstart_by_pos per read) stays the statement
    # it is tested against; VAPOR_MEMORY_CHOP=records selects it.
    def _arrays(self, chrom: str):
        cache = self.__dict__.setdefault("_chop_cache", {})
        recs = self._recs(chrom)
        key = id(recs)                       # (contigs that share one record list - tiled worlds - share its arrays)
        keep_it = getattr(self.world, "cache_ok", True)      # (a world that makes its record lists on demand: nothing is kept)
        got = cache.get(key) if keep_it else None
        if got is None or got[0] is not recs or got[4] != len(recs):
            import ctypes
            import numpy as np
            # (a str's own UTF-8 buffer, NUL-terminated and alive as long as the str: no copy of a 10 kb CIGAR per read)
            from .engine import _utf8
            size = ctypes.c_ssize_t()
            cig = [r.cigar for r in recs]
            ptrs = (ctypes.c_void_p * max(len(recs), 1))(*[_utf8(c, ctypes.byref(size)) for c in cig])
            arrs = (np.array([r.pos for r in recs], dtype=np.int64), np.array([r.ref_span for r in recs], dtype=np.int64),
                    np.array([len(r.seq) for r in recs], dtype=np.int64))
            got = (recs, arrs, (arrs[0].ctypes.data, arrs[1].ctypes.data, ctypes.addressof(ptrs), arrs[2].ctypes.data), (cig, ptrs), len(recs))
            if len(cache) > 200000:
                cache.clear()
            if keep_it:
                cache[key] = got
        return got

    def chop(self, bam: str, chrom: str, start: int, end: int, flank_length, tagged: bool = False, right: bool = False, sites=None):
        """`tagged` (`--phased`): every entry is [read, miss_bp, qname, hap, ps], the tags read from the record's SAM text
        fields (phase.tags_from_sam) - or, with sites (`--phase-vcf`: a phase.Sites, the argument or this backend's
        phase_sites), made by phase.haplotag from the locus's phased sites, the record's tags not looked at.  `right`
        (`--both-ends`): the right-anchored reads, reverse complemented - the walk in
        the library's host helper (vapor_chop_records_right), or _chop_records itself with VAPOR_MEMORY_CHOP=records."""
        if right:
            return self._chop_right(chrom, int(start), int(end), flank_length)
        if tagged:
            from .phase import haplotag, tags_from_sam
            if sites is None:
                sites = self.phase_sites
            rows = sites.rows(chrom, int(start), int(end)) if sites is not None else None
        dd = bool(self.dedup_qname)
        if _memory_chop_by_records():
            recs = self._overlapping(chrom, int(start), int(end))
            if tagged and sites is not None:
                return _chop_records([(r.qname, r.pos, r.cigar, r.seq, r.flag) for r in recs], start, end, flank_length,
                                     [haplotag(r.pos, r.cigar, r.seq, rows) for r in recs], dedup=dd)
            return _chop_records([(r.qname, r.pos, r.cigar, r.seq, r.flag) for r in recs], start, end, flank_length,
                                 [tags_from_sam(r.tag_fields()) for r in recs] if tagged else None, dedup=dd)
        recs, arrs, ptr, _keep, _n = self._arrays(chrom)
        if not recs:
            return []
        fn = self.__dict__.get("_chop_fn")
        if fn is None:
            from . import _lib
            fn = self.__dict__["_chop_fn"] = _lib.load_holding_gil().vapor_chop_records      # (a ~10 us call: see there)
        import numpy as np
        # (the answers go to arrays of the call's own: chunks of a run are scored on two threads, and tiled worlds share a
        # record list between contigs)
        qm_a, keep_a = np.empty(2 * len(recs), dtype=np.int64), np.empty(len(recs), dtype=np.uint8)
        start, end = int(start), int(end)
        if fn(len(recs), ptr[0], ptr[1], ptr[2], ptr[3], start, end, int(flank_length), qm_a.ctypes.data, keep_a.ctypes.data) != 0:
            raise IndexError("string index out of range")      # what '' [1] raises in SF:331
        kept = keep_a.nonzero()[0]
        if not len(kept):
            return []
        qm = qm_a.tolist()
        out = []
        for t in kept.tolist():
            q0, miss = qm[2 * t], qm[2 * t + 1]
            r = recs[t]
            out.append([r.seq[q0:q0 + (end - start - miss)] if q0 >= 0 else r.seq[q0:][:end - start - miss], miss, r.qname])
            if tagged:
                out[-1] += list(haplotag(r.pos, r.cigar, r.seq, rows) if sites is not None else tags_from_sam(r.tag_fields()))
        return dedup_kept(out, [recs[t].flag for t in kept.tolist()]) if dd else out

    def _chop_right(self, chrom: str, start: int, end: int, flank_length):
        from . import _lib
        fn = None if _memory_chop_by_records() else getattr(_lib.load_holding_gil(), "vapor_chop_records_right", None)
        if fn is None or end - start < flank_length:        # (a window shorter than its flank: Python's slice rules decide)
            return _chop_records([(r.qname, r.pos, r.cigar, r.seq, r.flag) for r in self._overlapping(chrom, start, end)],
                                 start, end, flank_length, right=True, dedup=bool(self.dedup_qname))
        recs, arrs, ptr, _keep, _n = self._arrays(chrom)
        if not recs:
            return []
        import numpy as np
        qm_a, keep_a = np.empty(2 * len(recs), dtype=np.int64), np.empty(len(recs), dtype=np.uint8)
        if fn(len(recs), ptr[0], ptr[1], ptr[2], ptr[3], start, end, int(flank_length), qm_a.ctypes.data, keep_a.ctypes.data) != 0:
            raise IndexError("string index out of range")
        qm = qm_a.tolist()
        out = []
        kept = keep_a.nonzero()[0].tolist()
        for t in kept:
            q1, miss = qm[2 * t], qm[2 * t + 1]
            r = recs[t]
            stop = len(r.seq) - q1                  # (the kept part ends here: q1 bases are dropped from the read's end)
            out.append([rc_read(r.seq[stop - (end - start - miss):stop]), miss, r.qname])
        return dedup_kept(out, [recs[t].flag for t in kept]) if self.dedup_qname else out

    def chop_many(self, bam: str, chroms, starts, ends, flanks, max_keep: int = 20, groups: bool = False, sites=None):
        """groups (`--phased`, not in the reference): the reads of a region are the union of the lists of its three groups (A: all
        kept records, H1 / H2: those of one haplotype in the region's phase set; phase.select) in record order, at most
        3 * max_keep, and three arrays follow the keepalive - member (uint32 per read: bits 0-2 the read is in the list of A / H1 /
        H2, bits 8-15, 16-23, 24-31 its position there), phase set (int64 per region, phase.PS_NONE for none) and tagged (per
        region: a kept record has hap != 0); with sites (`--phase-vcf`, as in chop) hap and ps are phase.haplotag's.  Without it:
        chop_pacbio_read_by_pos (SF:339-354) + minimize_pacbio_read_list (SF:1091-1102) for many regions in ONE native call
        (vapor_chop_records_many): per region its kept reads as numbers, not as lists of strings -
        (kept_first [n + 1], addr, q0, miss, status [n], keepalive): read t of region g (kept_first[g] <= t < kept_first[g + 1])
        is the `end - start - miss[t]` bytes at address addr[t] + q0[t] (inside the record's own sequence string, which
        `keepalive` holds); status[g] != 0: the region needs the per-record route (a record without CIGAR, a record whose
        sequence is not ASCII text)."""
        import ctypes
        import numpy as np
        from . import _lib
        from .engine import _ASCII_OFF
        n = len(chroms)
        # per contig, once: (records, pos*, span*, cigar**, seq_len*, addresses of the records' sequences or None)
        keep_it = getattr(self.world, "cache_ok", True)
        per = self.__dict__.setdefault("_many_cache", {}) if keep_it else {}

        def entry(c):
            recs, arrs, p, keep, _cnt = self._arrays(c)
            ok = 0 < _ASCII_OFF < 256 and all(type(r.seq) is str and r.seq.isascii() for r in recs)
            sa_c = (np.fromiter(map(id, (r.seq for r in recs)), dtype=np.uint64, count=len(recs)) + np.uint64(_ASCII_OFF)) if ok else None
            # (the arrays behind the pointers travel with the entry: they live as long as it does)
            e = per[c] = (len(recs), p[0], p[1], p[2], p[3], sa_c, recs, arrs, keep)
            return e
        ent = [per.get(c) or entry(c) for c in chroms]
        if keep_it:
            for g, e in enumerate(ent):                        # (a contig whose record list was replaced since)
                if e[6] is not self._recs(chroms[g]) or e[0] != len(e[6]):
                    ent[g] = entry(chroms[g])
        n_rec = np.fromiter((e[0] for e in ent), dtype=np.int32, count=n)
        ptr = np.asarray([(e[1], e[2], e[3], e[4]) for e in ent], dtype=np.uint64).reshape(n, 4).T.copy()
        sa_ptr = np.fromiter((e[5].ctypes.data if e[5] is not None else 0 for e in ent), dtype=np.uint64, count=n)
        bad = np.fromiter((e[5] is None and e[0] > 0 for e in ent), dtype=bool, count=n)
        keep_sel = max_keep
        dd = bool(self.dedup_qname)
        if groups or dd:                             # (every kept record comes back, in record order: the selection is below)
            max_keep = max(int(n_rec.max()) if n else 1, 1)
        cap = max_keep * max(n, 1)
        kept_first = np.zeros(n + 1, dtype=np.int32)
        rec_idx = np.zeros(cap, dtype=np.int32)
        q0 = np.zeros(cap, dtype=np.int64)
        miss = np.zeros(cap, dtype=np.int64)
        status = np.zeros(max(n, 1), dtype=np.int32)
        addr = np.zeros(cap, dtype=np.uint64)
        st = np.ascontiguousarray(starts, dtype=np.int64)
        en = np.ascontiguousarray(ends, dtype=np.int64)
        fl = np.ascontiguousarray(flanks, dtype=np.int64)
        rc = _lib.load().vapor_chop_records_many(n, n_rec.ctypes.data, ptr[0].ctypes.data, ptr[1].ctypes.data, ptr[2].ctypes.data,
                                                 ptr[3].ctypes.data, st.ctypes.data, en.ctypes.data, fl.ctypes.data, max_keep,
                                                 kept_first.ctypes.data, rec_idx.ctypes.data, q0.ctypes.data, miss.ctypes.data,
                                                 status.ctypes.data, sa_ptr.ctypes.data, addr.ctypes.data)
        if rc != 0:
            raise RuntimeError(_lib.load().vapor_bam_last_error().decode())
        tot = int(kept_first[n])
        addr = addr[:tot]
        status[:n][bad] = -1
        live = None
        if dd:
            # rule W on every region's kept records, before any list is made of them
            live = np.ones(tot, dtype=bool)
            for g in range(n):
                a, b = int(kept_first[g]), int(kept_first[g + 1])
                if b - a > 1 and status[g] == 0:
                    recs = ent[g][6]
                    ts = rec_idx[a:b].tolist()
                    live[a:b] = dedup_mask([recs[t].qname for t in ts], [recs[t].flag for t in ts])
        if dd and not groups:
            # minimize_pacbio_read_list on the survivors: the first keep_sel in a stable order by miss_bp
            kf2 = np.zeros(n + 1, dtype=np.int32)
            take = []
            for g in range(n):
                a, b = int(kept_first[g]), int(kept_first[g + 1])
                if status[g] == 0:
                    sel = a + np.flatnonzero(live[a:b])
                    if len(sel) > keep_sel:
                        sel = sel[np.argsort(miss[sel], kind="stable")[:keep_sel]]
                    take += sel.tolist()
                kf2[g + 1] = len(take)
            take = np.asarray(take, dtype=np.int64)
            return kf2, addr[take], q0[take], miss[take], status[:n], ent
        if groups:
            from . import phase
            if sites is None:
                sites = self.phase_sites
            pset, tagged = np.full(n, phase.PS_NONE, dtype=np.int64), np.zeros(n, dtype=np.int32)
            kf2 = np.zeros(n + 1, dtype=np.int32)
            take, member = [], []
            for g in range(n):
                a, b = int(kept_first[g]), int(kept_first[g + 1])
                if b > a and status[g] == 0:
                    recs = ent[g][6]
                    at = np.arange(a, b) if live is None else a + np.flatnonzero(live[a:b])    # (the survivors of rule W)
                    if sites is not None:
                        rows = sites.rows(chroms[g], int(st[g]), int(en[g]))
                        tg = [phase.haplotag(recs[t].pos, recs[t].cigar, recs[t].seq, rows) for t in rec_idx[at].tolist()]
                    else:
                        tg = [phase.tags_from_sam(recs[t].tag_fields()) for t in rec_idx[at].tolist()]
                    hap = np.asarray([h for h, _p in tg], dtype=np.int64)
                    ps = np.asarray([phase.PS_NONE if p is None else p for _h, p in tg], dtype=np.int64)
                    tagged[g], pset[g], order, words = phase.select_numbers(miss[at], hap, ps, keep_sel)
                    take += [int(at[i]) for i in order]
                    member += words
                kf2[g + 1] = len(take)
            take = np.asarray(take, dtype=np.int64)
            return kf2, addr[take], q0[take], miss[take], status[:n], ent, np.asarray(member, dtype=np.uint32), pset, tagged
        return kept_first, addr, q0[:tot], miss[:tot], status[:n], ent      # (the entries hold the records the addresses point into)

    def isfile(self, path: str) -> bool:
        return True

    def contig_length(self, bam: str, ref: str, chrom: str) -> int:
        """(`--depth`) the world's contig; 0 for one it does not have."""
        return len(self.world.contigs[chrom]) if chrom in self.world.contigs else 0

    def _cigar_ops(self, recs) -> list:
        """The operations of every record of one of the world's record lists, each CIGAR text parsed once per list."""
        from .depth import parse_cigar
        cache = self.__dict__.setdefault("_cigar_cache", {})
        got = cache.get(id(recs))
        if got is None or got[0] is not recs or got[1] != len(recs):
            got = (recs, len(recs), [parse_cigar(r.cigar) for r in recs])
            if getattr(self.world, "cache_ok", True):
                if len(cache) > 200000:
                    cache.clear()
                cache[id(recs)] = got
        return got[2]

    def _evidence_many(self, module, engine, bam: str, chroms, rows, partners=None):
        """module.statement over the world's records that pass the read filter with module.EXCLUDE among its flags and start
        before the end of the region's walk window: (POS, operations), and for a module whose records are LINKED FLAG and the
        SA value - the record's `SA` tag when that is a string."""
        from .bamio import record_passes
        q, f = self.read_filter
        f |= module.EXCLUDE
        lo, hi = module.WINDOW
        out = []
        for g, (chrom, row) in enumerate(zip(chroms, rows)):
            recs = self.world.reads.get(chrom, ())
            w0, w3 = int(row[lo]), int(row[hi])
            kept = [(r, ops) for r, ops in zip(recs, self._cigar_ops(recs)) if w0 < w3 and r.pos - 1 < w3 and record_passes(r.mapq, r.flag, q, f)]
            if module.LINKED:
                sas = [(r.tags or {}).get("SA") for r, _ops in kept]
                records = [(r.pos, ops, r.flag, sa.encode("latin-1") if isinstance(sa, str) else None) for (r, ops), sa in zip(kept, sas)]
            else:
                records = [(r.pos, ops) for r, ops in kept]
            out.append(module.statement(records, row, partners[g] if partners is not None else None, q))
        return out

    def fai_lines(self, ref: str) -> Iterable[str]:
        rows = self.world.fai_rows() if hasattr(self.world, "fai_rows") else [(k, len(v)) for k, v in self.world.contigs.items()]
        return ["%s\t%d\t0\t60\t61" % (k, n) for k, n in rows]


def _env_is(name: bytes, value: bytes) -> bool:
    # (os.environ is a mapping with an encode per lookup: 5 us a call, and these are asked once per locus)
    e = os.environ
    v = e._data.get(name) if hasattr(e, "_data") else e.get(name.decode())
    return v in (value, value.decode())


def _memory_chop_by_records() -> bool:
    return _env_is(b"VAPOR_MEMORY_CHOP", b"records")


def set_backend(b) -> None:
    global _backend
    _backend = b


def get_backend():
    global _backend
    if _backend is None:
        # In-process readers (.fai, BGZF/BAM + .bai) unless samtools is asked for: no process per locus, which is the
        # wall-clock floor once scoring runs on the GPU.  They raise on a missing .bai/.fai instead of returning nothing.
        want = os.environ.get("VAPOR_BAM_BACKEND", "inprocess")
        _backend = SamtoolsHybrid() if want == "samtools" else InProcessBam()
        import sys
        print("vapor_amd.seqio: %s backend for BAM regions (VAPOR_BAM_BACKEND=%s)"
              % ("samtools" if want == "samtools" else "in-process BGZF/BAI", want), file=sys.stderr)
    return _backend


# ---------------------------------------------------------------------------
# reference-named helpers
# ---------------------------------------------------------------------------
_COMP = {i: None for i in range(256)}
_COMP.update({ord(a): b for a, b in zip("ATGCNatgcn", "TACGNtacgn")})


def complementary(seq: str) -> str:
    """SF:471-478 - complements ATGCN/atgcn and silently drops everything else."""
    return seq.translate(_COMP)


def reverse(seq: str) -> str:
    return seq[::-1]


def ref_seq_readin(ref, chrom, start, end, reverse_flag="FALSE") -> str:
    """SF:1203-1217: `samtools faidx ref chrom:start-end`, header dropped, the first
    whitespace-separated token of every following line joined, stopping at a blank line."""
    be = get_backend()
    if hasattr(be, "fetch_seq"):
        seq = be.fetch_seq(ref, chrom, int(start), int(end))     # the same bases without the 60-column text in between
    else:
        lines = iter(be.faidx_lines(ref, "%s:%d-%d" % (chrom, int(start), int(end))))
        next(lines, None)
        parts: List[str] = []
        for ln in lines:
            tok = ln.strip().split()
            if not tok:
                break
            parts.append(tok[0])
        seq = "".join(parts)
    if reverse_flag == "FALSE":
        return seq
    return reverse(complementary(seq))


_CIGAR_RE = re.compile(r"(\d+)([MIDNSHP=X])")


def _cigar2alignstart_py(cigar: str, align_start: int, start: int, end: int):
    """SF:309-337 in Python (the statement the native helper is tested against)."""
    q = 0
    r = align_start
    last = None
    for m in _CIGAR_RE.finditer(cigar):
        n = int(m.group(1))
        op = m.group(2)
        if op == "S" or op == "I":
            q += n
        elif op == "M" or op == "=":
            q += n
            r += n
        elif op == "D":
            r += n
        last = op
        if r > start - 1:
            break
    if last is None:
        raise IndexError("string index out of range")  # what '' [1] raises in SF:331
    over = int(r) - start
    if last in ("M", "="):
        return [q - over, 0]
    return [q, over]


class PrefetchedBam(str):
    """A BAM file's name that carries reads already selected on the device: `prefetched` maps (chrom, start, end, flank, right)
    to the window's kept reads as [engine.DevRead, miss_bp, ""] entries (prefetch_views); chop_pacbio_read_by_pos answers
    from it, and a window that is not there - one the device left to the host route - goes the usual way."""
    prefetched = None
    batches = ()


def prefetch_views(engine, bam: str, windows, max_keep: int = 20) -> PrefetchedBam:
    """The reads of many windows - (chrom, start, end, flank, right) each - of one BAM file in two device calls
    (InProcessBam.chop_many_device: the left-anchored windows, the right-anchored ones), under minimize_pacbio_read_list's cap.
    Returns the file's name as a PrefetchedBam; it holds the batches the reads lie in."""
    from .engine import DevRead
    out = PrefetchedBam(bam)
    out.prefetched, out.batches = {}, []
    be = get_backend()
    for right in (False, True):
        ws = sorted({w for w in windows if bool(w[4]) == right and w[1] >= 0})
        if not ws:
            continue
        kf, addr, q, miss, status, batches = be.chop_many_device(
            engine, bam, [w[0] for w in ws], [w[1] for w in ws], [w[2] for w in ws], [w[3] for w in ws], max_keep,
            **({"right": True} if right else {}))
        out.batches += batches
        keep = tuple(batches)
        # (`--dedup-qname`: the device route carries no names - the third slot holds the read's name key, an int, for rule V)
        keys = None
        if getattr(be, "dedup_qname", False):
            import numpy as np
            keys = np.concatenate([bt.name_keys for bt in batches]) if batches else np.zeros(0, dtype=np.uint64)
            if len(keys) != int(kf[-1]):
                raise RuntimeError("prefetch_views: %d name keys for %d reads" % (len(keys), int(kf[-1])))
        for g, w in enumerate(ws):
            if status[g] == 0:
                out.prefetched[(w[0], int(w[1]), int(w[2]), int(w[3]), right)] = [
                    [DevRead(addr[t], q[t], w[2] - w[1] - int(miss[t]), 2 if right else 1, keep), int(miss[t]),
                     "" if keys is None else int(keys[t])]
                    for t in range(int(kf[g]), int(kf[g + 1]))]
    return out


def _cigar2alignend_py(cigar: str, align_start: int, end: int):
    """The mirror image of the walk above (`--both-ends`; not in the reference): the CIGAR walked from its far
    end, the reference cursor starting on the alignment's last reference base (align_start + M/=/D total - 1) and moving left,
    until it has reached `end` or passed it.  Returns [last reference base, q1 = read bases to drop from the read's END,
    miss_bp counted from the window end] - cigar2alignstart_by_pos of the reversed operations at L + 1 - last base against
    L + 1 - end, for any L."""
    ops = [(int(m.group(1)), m.group(2)) for m in _CIGAR_RE.finditer(cigar)]
    if not ops:
        raise IndexError("string index out of range")
    last_ref = align_start + sum(n for n, op in ops if op in "M=D") - 1
    q = 0
    c = last_ref
    last = None
    for n, op in reversed(ops):
        if op == "S" or op == "I":
            q += n
        elif op == "M" or op == "=":
            q += n
            c -= n
        elif op == "D":
            c -= n
        last = op
        if c < end + 1:
            break
    over = end - c
    if last in ("M", "="):
        return [last_ref, q - over, 0]
    return [last_ref, q, over]


# BAM's 4-bit alphabet "=ACMGRSVTWYHKDBN": the complement of a symbol is its nibble with the bits reversed (= and N stay); on
# text the same table in both letter cases, every other character as it is
_RC_TEXT = {ord(a): b for a, b in zip("ACMGRSVTWYHKDBNacmgrsvtwyhkdbn", "TGKCYSBAWRDMHVNtgkcysbawrdmhvn")}


def rc_read(seq: str) -> str:
    """The reverse complement of a read's SEQ (`--both-ends`): position reversal and the table above - nothing is dropped."""
    return seq.translate(_RC_TEXT)[::-1]


_cigar_out = None
_cigar_ptr = None
_cigar_fn = None


def cigar2alignstart_by_pos(cigar: str, align_start: int, start: int, end: int):
    """SF:309-337: walk the CIGAR until the reference cursor passes `start-1`; returns
    [offset into the read, miss_bp].  Only S/M/=/I advance the read and M/=/D the
    reference (N, H, P and X advance nothing, as in the reference).  Long-read CIGARs hold thousands of
    operations, so the walk is the library's host helper `vapor_cigar2alignstart` (a dozen times faster than the
    interpreter loop); `_cigar2alignstart_py` is the same in Python."""
    global _cigar_out, _cigar_ptr, _cigar_fn
    if _cigar_out is None:
        import ctypes
        import numpy as np
        from . import _lib
        _cigar_out = np.zeros(2, dtype=np.int64)
        _cigar_ptr = _cigar_out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))     # made once: a ctypes view per call costs more than the walk
        _cigar_fn = _lib.load().vapor_cigar2alignstart
    rc = _cigar_fn(cigar.encode("ascii", "replace"), int(align_start), int(start), _cigar_ptr)
    if rc != 0:
        raise IndexError("string index out of range")  # what '' [1] raises in SF:331
    return [int(_cigar_out[0]), int(_cigar_out[1])]


def _sam_fields(be, bam, chrom, start, end, exclude_more=0):
    """The fields of every alignment line of the backend's `view bam chrom:start-end` that passes the backend's read filter
    (FLAG is column 2, MAPQ column 5) - the one place SAM text is filtered.  exclude_more (`--depth`): flags
    excluded beside the filter's."""
    from .bamio import record_passes
    min_mapq, exclude = getattr(be, "read_filter", (0, 0))
    exclude |= exclude_more
    for line in be.view_lines(bam, "%s:%d-%d" % (chrom, start, end)):
        f = line.strip().split()
        if not f or f[0] == "@":
            continue
        if (min_mapq or exclude) and not record_passes(int(f[4]), int(f[1]), min_mapq, exclude):
            continue
        yield f


def chop_pacbio_read_by_pos(bam_in_new, chrom, start, end, flank_length, tagged=False, right=False, sites=None):
    """SF:339-354.  `tagged` (`--phased`, not in the reference): every kept record as [read, miss_bp, qname, hap, ps], its
    haplotype and phase set read from the HP and PS fields behind SEQ (vapor_amd.phase) - or, with sites (`--phase-vcf`: a
    phase.Sites, the argument or the backend's phase_sites), made from the locus's phased sites (phase.haplotag).  `right` (`--both-ends`, not in the
    reference): the right-anchored reads of the window - alignments that end at or after `end` - each as the
    reverse complement of its part that ends on the window end, miss_bp counted from there (_chop_records)."""
    out = []
    be = get_backend()
    dedup = bool(getattr(be, "dedup_qname", False))      # (`--dedup-qname`, DESIGN.md 4.18: rule W on the kept records)
    pre = getattr(bam_in_new, "prefetched", None)
    if pre is not None and not tagged:
        # (`--both-ends` from files: the reads of this window were selected on the device with the chunk's other windows)
        got = pre.get((chrom, int(start), int(end), int(flank_length), bool(right)))
        if got is not None:
            return [list(x) for x in got]
    if right:
        if tagged:
            raise ValueError("right-anchored reads are not read with tags")
        if hasattr(be, "chop"):
            return be.chop(bam_in_new, chrom, start, end, flank_length, right=True)
        if hasattr(be, "records") and not dedup:
            recs = be.records(bam_in_new, chrom, start, end)
        else:
            recs = [(f[0], f[3], f[5], f[9], int(f[1])) for f in _sam_fields(be, bam_in_new, chrom, start, end)]
        return _chop_records(recs, start, end, flank_length, right=True, dedup=dedup)
    if tagged and sites is None:
        sites = getattr(be, "phase_sites", None)
    if hasattr(be, "chop"):
        if tagged and sites is not None:
            return be.chop(bam_in_new, chrom, start, end, flank_length, tagged=True, sites=sites)
        return be.chop(bam_in_new, chrom, start, end, flank_length, tagged=True) if tagged else be.chop(bam_in_new, chrom, start, end, flank_length)
    tags = None
    if hasattr(be, "records") and not tagged and not dedup:
        recs = be.records(bam_in_new, chrom, start, end)
    else:
        from .phase import tags_from_sam
        recs, tags = [], ([] if tagged else None)
        for f in _sam_fields(be, bam_in_new, chrom, start, end):
            recs.append((f[0], f[3], f[5], f[9], int(f[1])))
            if tagged:
                tags.append(tags_from_sam(f[11:]))
        if tagged and sites is not None:
            from .phase import haplotag
            rows = sites.rows(chrom, int(start), int(end))
            tags = [haplotag(int(r[1]), r[2], r[3], rows) for r in recs]
    return _chop_records(recs, start, end, flank_length, tags, dedup=dedup)


def mirror_records(recs, length):
    """The records of a contig of `length` bases as the reverse-complemented contig holds them (x -> length + 1 - x):
    (qname, length + 1 - last reference base, CIGAR operations reversed, rc_read(SEQ)) - the definition the right-anchored chop
    is tested against.  The last reference base follows the cursor rule of SF:309-337 (M, = and D advance the reference)."""
    out = []
    for qname, pos, cigar, seq in recs:
        ops = _CIGAR_RE.findall(cigar)
        last_ref = int(pos) + sum(int(n) for n, op in ops if op in "M=D") - 1
        out.append((qname, length + 1 - last_ref, "".join(n + op for n, op in reversed(ops)) or cigar, rc_read(seq)))
    return out


def name_key(qname) -> int:
    """The identity of a molecule (`--dedup-qname`): two records are the same molecule iff name_key(QNAME) is
    equal.  b_0 .. b_{n-1} the QNAME bytes: h = n + sum_i (b_i + 1) * M^(i+1) mod 2^64 with M = 0x9E3779B97F4A7C15, key = the
    splitmix64 finaliser of h.  The Python statement of csrc/vapor_names.h name_key, which the native host reader and
    bam_dedup_kernel compute."""
    b = qname.encode("utf-8", "surrogateescape") if isinstance(qname, str) else bytes(qname)
    mask = 0xFFFFFFFFFFFFFFFF
    h, x = len(b), 0x9E3779B97F4A7C15
    for c in b:
        h = (h + (c + 1) * x) & mask
        x = (x * 0x9E3779B97F4A7C15) & mask
    h ^= h >> 30
    h = (h * 0xBF58476D1CE4E5B9) & mask
    h ^= h >> 27
    h = (h * 0x94D049BB133111EB) & mask
    return h ^ (h >> 31)


def dedup_mask(qnames, flags):
    """Rule W over the kept records of one (file, region, anchor kind), in record order: per name key exactly
    one survives, the one with the smallest ((FLAG & 0x900) != 0, record order) - the first that is neither secondary nor
    supplementary, else the first.  Returns one bool per record."""
    best = {}
    for i, (q, f) in enumerate(zip(qnames, flags)):
        k = name_key(q)
        rank = ((int(f) & 0x900) != 0, i)
        if k not in best or rank < best[k]:
            best[k] = rank
    live = {i for _s, i in best.values()}
    return [i in live for i in range(len(qnames))]


def dedup_kept(kept, flags):
    """Rule W on a list of kept entries ([read, miss_bp, qname, ...], in record order) and their records' FLAGs: the one place the
    Python readers de-duplicate (chop_python, _chop_records, MemorySamtools).  A dropped record is as if it were not in the
    file."""
    if len(kept) < 2:
        return kept
    return [e for e, ok in zip(kept, dedup_mask([e[2] for e in kept], flags)) if ok]


def _chop_records(recs, start, end, flank_length, tags=None, right=False, dedup=False):
    """The body of chop_pacbio_read_by_pos (SF:345-353) over (qname, pos, cigar, seq) records; tags: (hap, ps) per record, which
    the kept ones then carry.  dedup (`--dedup-qname`): the records are (qname, pos, cigar, seq, FLAG) and rule W (dedup_kept) is
    applied to the list that is returned.  right: the closed form of _chop_records(mirror_records(recs, L), L + 1 - end, L + 1 - start,
    flank_length) - an alignment qualifies when its last reference base is >= end, the walk goes from the far end of the CIGAR
    (_cigar2alignend_py), and of the read without its last q1 bases the last end - start - miss_bp are kept, reverse
    complemented, when more than that many are there."""
    out = []
    flags = []
    if right:
        for rec in recs:
            qname, pos, cigar, seq = rec[:4]
            # (the M / = / D total first: only an alignment that qualifies is walked - one without operation "ends" at pos - 1
            # and raises where the mirror would)
            if int(pos) + sum(int(n) for n, op in _CIGAR_RE.findall(cigar) if op in "M=D") - 1 < end:
                continue
            last_ref, q1, miss_bp = _cigar2alignend_py(cigar, int(pos), end)
            if not miss_bp > flank_length / 2:
                head = seq[:max(len(seq) - q1, 0)]
                want = end - start - miss_bp
                if len(head) > want:
                    out.append([rc_read(head)[:want] if want < 0 else rc_read(head[len(head) - want:]), miss_bp, qname])
                    if dedup:
                        flags.append(rec[4])
        return dedup_kept(out, flags) if dedup else out
    for t, rec in enumerate(recs):
        qname, pos, cigar, seq = rec[:4]
        if int(pos) < start + 1:
            q0, miss_bp = cigar2alignstart_by_pos(cigar, int(pos), start, end)
            if not miss_bp > flank_length / 2:
                tail = seq[q0:]
                want = end - start - miss_bp
                if len(tail) > want:
                    out.append([tail[:want], miss_bp, qname] + (list(tags[t]) if tags is not None else []))
                    if dedup:
                        flags.append(rec[4])
    return dedup_kept(out, flags) if dedup else out


def minimize_pacbio_read_list(x, ideal_list_length=20):
    """SF:1091-1102: keep at most 20 reads, smallest miss_bp first, input order inside
    one miss_bp value."""
    if len(x) <= ideal_list_length:
        return x
    by_miss = {}
    for rec in x:
        by_miss.setdefault(rec[1], []).append(rec)
    out = []
    for k in sorted(by_miss):
        if len(out) < ideal_list_length:
            out += by_miss[k]
    return out[:ideal_list_length]


def bam_in_decide(bam_in, bps):
    """SF:69-89: a file, or a per-chromosome pattern with XXX or * in the basename."""
    be = get_backend()
    if be.isfile(bam_in):
        return [bam_in]
    d = "/".join(bam_in.split("/")[:-1]) + "/"
    base = bam_in.split("/")[-1]
    if "XXX" in base:
        keys = base.split("XXX")
    elif "*" in base:
        keys = base.split("*")
    else:
        print("Error: invalid name for pacbio files !")
        raise NameError("bam_in_keys")  # the reference dies on the unbound name (SF:82)
    ext = bam_in.split(".")[-1]
    return [d + k for k in os.listdir(d)
            if k.split(".")[-1] == ext and all(y in k for y in keys)]


def simple_del_chop_pacbio_read_simple_short(bam_in, sv_info, flank_length, phased=False, right=False):
    """SF:1378-1390: reads around the left breakpoint only.  `phased` (`--phased`): the same list as a phase.PhasedReads, with
    the lists of the two haplotype groups beside it (phase.select over the kept records of all files, before the cap).
    `right` (`--both-ends`): the right-anchored reads of the same window (chop_pacbio_read_by_pos), under the same cap."""
    bams = bam_in_decide(bam_in, sv_info)
    if bams == "":
        return [[], [], []]
    x = []
    if right:
        for b in bams:
            x += chop_pacbio_read_by_pos(b, sv_info[0], int(sv_info[1]) - flank_length, int(sv_info[1]) + flank_length,
                                         flank_length, right=True)
        return minimize_pacbio_read_list(x)
    for b in bams:
        x += chop_pacbio_read_by_pos(b, sv_info[0], int(sv_info[1]) - flank_length,
                                     int(sv_info[1]) + flank_length, flank_length, *((True,) if phased else ()))
    if phased:
        from .phase import select
        return select(x)
    return minimize_pacbio_read_list(x)


def simple_chop_pacbio_read_simple_short(bam_in, sv_info, flank_length, phased=False):
    """SF:1392-1401: reads spanning first to last breakpoint.  `phased`: as in simple_del_chop_pacbio_read_simple_short."""
    bams = bam_in_decide(bam_in, sv_info)
    if bams == "":
        return [[], [], []]
    x = []
    for b in bams:
        x += chop_pacbio_read_by_pos(b, sv_info[0], int(sv_info[1]) - flank_length,
                                     int(sv_info[-1]) + flank_length, flank_length, *((True,) if phased else ()))
    if phased:
        from .phase import select
        return select(x)
    return minimize_pacbio_read_list(x)


class _Chromos(list):
    """The contig names as the list the reference builds, with `in` answered from a set (the drivers of the unclassified
    structures test every breakpoint token against it, SF:1490-1555: a scan of thousands of names each)."""

    def __init__(self, names):
        super().__init__(names)
        self._names = frozenset(names)

    def __contains__(self, x):
        try:
            return x in self._names
        except TypeError:                     # (an unhashable token: the list's own comparison)
            return list.__contains__(self, x)


_chromos_cache: dict = {}


def chromos_readin(ref) -> List[str]:
    """SF:356-363: contig names from the .fai.  The reference reads the file again for every unclassified record; the names
    are kept here per backend and index file as long as the file's size and modification time (or, for an in-memory world,
    its contig table) stay what they were - 2.5 ms a call on an index of 5 000 contigs otherwise."""
    be = get_backend()
    world = getattr(be, "world", None)
    if world is not None:
        stamp = (id(world.contigs), len(world.contigs))
    else:
        try:
            st = os.stat(str(ref) + ".fai")
            stamp = (st.st_mtime_ns, st.st_size)
        except OSError:
            stamp = None
    key = (id(be), ref)
    got = _chromos_cache.get(key)
    if got is not None and stamp is not None and got[0] == stamp:
        return got[1]
    out = []
    for ln in be.fai_lines(ref):
        f = ln.strip().split()
        if f:
            out.append(f[0])
    out = _Chromos(out)
    if stamp is not None:
        if len(_chromos_cache) > 64:
            _chromos_cache.clear()
        _chromos_cache[key] = (stamp, out, be)          # (the backend kept alive: its id() is part of the key)
    return out


def flank_length_calculate(bps) -> int:
    """SF:794-802: min(500, last - first breakpoint)."""
    span = int(bps[-1]) - int(bps[1])
    return span if span < 500 else 500
