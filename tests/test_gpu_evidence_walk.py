"""The record walk the four evidence kernels share (vapor_bamdev.h walk_records) where it refuses a region or ends one early, on
bam_depth_kernel, bam_signature_kernel, bam_link_kernel and bam_support_kernel alike: a record whose block_size is 20, one whose
l_seq makes its fields exceed block_size, one that runs past the bytes the call staged, a record of a higher contig in front of
one of the region's, and a region of two chunks with a passing record in each.  The oracle of the statuses is the chop entry
(vapor_bam_chop_device: bam_chop_body keeps a walk of its own) over the same chunks, contig and stop; a refused region has no
words, its good neighbour in the same call has the host reader's, and so have the two cases that are not refusals.

One file, written here byte by byte from records bamio encoded: the cases lie on contigs of their own, in an order no sorted file
has, and every region comes with explicit chunks - no index is asked."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import test_bamio as TB
import test_gpu_depth as GD
import test_signature_cpu as SC
from vapor_amd import _lib as L
from vapor_amd import bamio
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu

REG_BEYOND, REG_MALFORMED = 1, 2
M, I, D, N, S, H = range(6)
BLOCK = 4096
W3 = 20000                                              # every region: [0, W3) of its contig
OPS = [(40, S), (300, M), (30, D), (300, M), (40, S)]   # a record with both clips and a gap: something for every kernel to count
REFS = [("bs20", 30000), ("lseq", 30000), ("big", 90000), ("order", 30000), ("higher", 30000), ("two", 30000), ("ok", 30000)]
PARTNER = b"ok"


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(path, {case: (tid, chunks)}): the file and every case's region."""
    d = tmp_path_factory.mktemp("evidence_walk")
    rows = [("a0", 0, 100, OPS, 60, 0), ("a_bad", 0, 200, OPS, 60, 0), ("a2", 0, 300, OPS, 60, 0),
            ("b0", 1, 100, OPS, 60, 0), ("b_bad", 1, 200, OPS, 60, 0), ("b2", 1, 300, OPS, 60, 0),
            ("c0", 2, 100, OPS, 60, 0), ("c_big", 2, 200, [(60000, M)], 60, 0),
            ("d0", 3, 100, OPS, 60, 0), ("d_high", 4, 50, OPS, 60, 0), ("d_never", 3, 300, OPS, 60, 0),
            ("e0", 5, 100, OPS, 60, 0), ("e_skip", 5, 2000, OPS, 60, 0), ("e1", 5, 5000, OPS, 60, 0),
            ("k0", 6, 100, OPS, 60, 0), ("k1", 6, 260, [(500, M)], 60, 0), ("k2", 6, 400, OPS, 60, 0)]
    sorted_path = str(d / "sorted.bam")
    SC.write_rows(sorted_path, REFS, rows, block_size=0xFF00)
    raw = open(sorted_path, "rb").read()
    whole = b"".join(zlib.decompress(raw[o + 12 + x:o + bz - 8], -15) for o, bz, x in TB._blocks(raw))
    starts = GD._record_starts(sorted_path)
    head = whole[:starts[0][0]]
    blob = {name: bytearray(whole[q:q + 4 + struct.unpack_from("<i", whole, q)[0]]) for q, name in starts}
    struct.pack_into("<i", blob["a_bad"], 0, 20)                                        # (a) block_size 20
    struct.pack_into("<i", blob["b_bad"], 4 + 16, len(blob["b_bad"]) - 4)               # (b) l_seq = block_size: the fields exceed it
    rng = np.random.default_rng(11)                                                     # (c) bases and qualities that do not compress
    big = blob["c_big"]
    at = 4 + 32 + len("c_big") + 1 + 4
    big[at:at + 90000] = rng.integers(0, 256, size=90000, dtype=np.uint8).tobytes()
    assert len(big) > 90000
    stream, where = bytearray(head), {}
    for name, _t, _p, _o, _q, _f in rows:               # (in the order of `rows`: d_high lies between the two records of contig 3)
        where[name] = (len(stream), len(stream) + len(blob[name]))
        stream += blob[name]
    coff, out = [], b""
    for o in range(0, len(stream), BLOCK):
        coff.append(len(out))
        out += bamio._bgzf_block(bytes(stream[o:o + BLOCK]))
    coff.append(len(out))
    out += bamio._BGZF_EOF
    path = str(d / "walk.bam")
    open(path, "wb").write(out)

    def voff(u):
        return (coff[u // BLOCK] << 16) | (u % BLOCK)
    span = lambda first, last: (voff(where[first][0]), voff(where[last][1]))            # noqa: E731
    regions = {"a": (0, [span("a0", "a2")]), "b": (1, [span("b0", "b2")]),
               "c": (2, [(voff(where["c0"][0]), voff(where["c_big"][0] + 1))]),
               "d": (3, [span("d0", "d_never")]), "e": (5, [span("e0", "e0"), span("e1", "e1")]), "ok": (6, [span("k0", "k2")])}
    return path, regions


class Handle:
    """A native reader handle of the file, without an index."""
    def __init__(self, path):
        self.lib = L.load()
        self.h = ctypes.c_void_p()
        assert self.lib.vapor_bam_open(path.encode(), ctypes.byref(self.h)) == 0

    def close(self):
        self.lib.vapor_bam_close(self.h)


DEPTH = (0, 150, 450, W3)
SIG = (0, W3, 100, 770, 50, 10, 0, SC.NCAP, 63)
LINK = (0, W3, 100, 5000, 50, 10, 0, 0, 0, 0, len(PARTNER))
SUP = SIG[:8] + (255, 50, 20)


def device(eng, h, picks):
    """The five raw entries over the same regions: {entry: (words per region, status per region)}."""
    tids = [t for t, _ch in picks]
    chunk_first, flat = [0], []
    for _t, ch in picks:
        for c in ch:
            flat += list(c)
        chunk_first.append(len(flat) // 2)
    flat = np.asarray(flat, dtype=np.uint64)
    n = len(picks)
    got = {}
    kept_first, _addr, _q0, _miss, status, batch = eng.bam_chop_device(h.h, tids, [1] * n, [W3] * n, [100000] * n, chunk_first, flat)
    batch.close()
    got["chop"] = (kept_first.tolist(), status.tolist())
    for name, fn, fields, more in (("depth", eng.bam_depth_device, DEPTH, ()), ("sig", eng.bam_signature_device, SIG, ()),
                                   ("links", eng.bam_links_device, LINK, (PARTNER,)), ("sup", eng.bam_support_device, SUP, ())):
        out, status = fn(h.h, tids, np.asarray([fields] * n, dtype=np.int64), chunk_first, flat, *more)
        got[name] = ([[int(x) for x in o] for o in out], status.tolist())
    return got


def host(h, tid, chunks):
    """The host readers' answers for one region: {entry: words}."""
    flat = np.asarray(chunks, dtype=np.uint64).reshape(-1)
    got = {}
    for name, fn, fields, n_out, dtype, more in (("depth", h.lib.vapor_bam_depth, DEPTH, 3, np.uint64, ()), ("sig", h.lib.vapor_bam_signature, SIG, 10, np.int64, ()),
                                                 ("links", h.lib.vapor_bam_links, LINK, 5, np.int64, (PARTNER, len(PARTNER))),
                                                 ("sup", h.lib.vapor_bam_support, SUP, 7, np.int64, ())):
        f = np.asarray(fields, dtype=np.int64)
        out = np.zeros(n_out, dtype=dtype)
        rc = fn(h.h, tid, f.ctypes.data, *more, len(flat) // 2, flat.ctypes.data, out.ctypes.data)
        assert rc == 0, (name, h.lib.vapor_bam_last_error().decode())
        got[name] = [int(x) for x in out]
    return got


@pytest.mark.parametrize("case, want", [("a", REG_MALFORMED), ("b", REG_MALFORMED), ("c", REG_BEYOND), ("d", 0), ("e", 0)])
def test_the_evidence_entries_refuse_and_end_a_region_as_the_chop_entry_does(eng, world, case, want):
    path, regions = world
    h = Handle(path)
    try:
        got = device(eng, h, [regions[case], regions["ok"]])
        neighbour = host(h, *regions["ok"])
        assert any(neighbour["depth"]) and any(neighbour["sig"][:6]) and neighbour["links"][0] > 0 and any(neighbour["sup"])
        assert got["chop"][1] == [want, 0], (case, got["chop"])
        for name in ("depth", "sig", "links", "sup"):
            words, status = got[name]
            assert status == got["chop"][1], (case, name, status)
            assert words[1] == neighbour[name], (case, name, words[1], neighbour[name])
            if want:
                assert words[0] == [0] * len(words[0]), (case, name, words[0])
        if not want:
            mine = host(h, *regions[case])
            for name in ("depth", "sig", "links", "sup"):
                assert got[name][0][0] == mine[name], (case, name, got[name][0][0], mine[name])
            # the third interval, [450, W3): 280 bases of a record at 100, 600 of one behind 450.  (d): d0 alone - d_never lies
            # behind the record of a higher contig; (e): e0 and e1, a span each, e_skip in neither
            assert mine["depth"][2] == (280 + 600 if case == "e" else 280), (case, mine)
    finally:
        h.close()
