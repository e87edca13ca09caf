"""The sequence planes (p2, e1, x4) and the counters of every producer - pack_kernel, the host staging in front of it,
derive_kernel, bam_expand_kernel + pack_kernel - against tests/plane_model.py, a numpy statement of the format that is no
kernel.  Every comparison is exact and against the model; no producer is compared with another.

The bodies take an engine, so tests/test_planes_cpu.py runs them on the CPU twin as well (all but the one that needs the bases
of a BAM file on the device)."""
import ctypes

import numpy as np
import pytest

import plane_model as M
from vapor_amd import _lib as L

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193)
ALPHABET = b"ACGTacgtNnRrYyKkMmXx-=*"
# the library stages an upload on several host threads when its ASCII layout (every sequence in whole 32-byte chunks) holds
# STAGE_SWITCH_BYTES or more and the set STAGE_SWITCH_SEQS sequences or more (the constants of these names in
# vapor_amd/csrc/vapor_seqset_plan.h)
STAGE_SWITCH_BYTES = 4 << 20
STAGE_SWITCH_SEQS = 8
STAGE_THREADS = (1, 2, 3, 5, 12, 13, 64)
STAGE_THREADS_DEFAULT = 3


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def draw(rng, n, alphabet=ALPHABET):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def n_chunks(seq):
    return (len(seq) + 31) // 32


def read_planes(ss):
    """The planes of all sequences of a set in one pass, one behind the other."""
    got = [ss.planes(t) for t in range(ss.n)]
    return tuple(np.concatenate([g[w] for g in got]) if got else np.zeros(0, np.uint32) for w in range(3))


def assert_set(ss, texts, upper=None, tag=""):
    """Planes, lengths and both counters of every sequence of `ss` equal the model of `texts`."""
    assert ss.n == len(texts), tag
    assert ss.lens.tolist() == [len(t) for t in texts], tag
    p2, e1, x4, n_exc, n_inv = M.set_planes(texts, upper)
    got = read_planes(ss)
    if not all(np.array_equal(a, b) for a, b in zip(got, (p2, e1, x4))):
        for t in range(ss.n):                                           # (name the first sequence that differs)
            want = M.planes(texts[t], bool(upper[t]) if upper is not None else False)
            for a, b, what in zip(ss.planes(t), want, ("p2", "e1", "x4")):
                assert np.array_equal(a, b), (tag, t, what, len(texts[t]), np.flatnonzero(a != b)[:4].tolist())
    for a, b, what in zip(got, (p2, e1, x4), ("p2", "e1", "x4")):
        assert np.array_equal(a, b), (tag, what)
    assert ss.n_exc.tolist() == n_exc.tolist(), tag
    assert ss.n_invalid.tolist() == n_inv.tolist(), tag


def check_set(eng, texts, upper=None, tag=""):
    ss = eng.seqset(texts, upper=upper)
    try:
        assert_set(ss, texts, upper, tag)
    finally:
        ss.close()
    return ss


# ---- a. pack_kernel at its edges ----------------------------------------------------------------------------------------
def edge_sequences():
    rng = np.random.default_rng(4101)
    seqs = [b"", bytes(range(256))]
    for t, n in enumerate(LENGTHS):
        seqs += [rng.integers(0, 256, n, dtype=np.uint8).tobytes(), draw(rng, n)]
        if t == len(LENGTHS) // 2:
            seqs += [b"", b""]
    return seqs + [b""]


def check_pack_edges(eng):
    seqs = edge_sequences()
    assert seqs[0] == b"" and seqs[-1] == b"" and any(a == b"" and b == b"" for a, b in zip(seqs[1:-1], seqs[2:-1]))
    assert sorted(set(map(len, seqs))) == sorted(set(LENGTHS + (256,)))
    check_set(eng, seqs + seqs, [False] * len(seqs) + [True] * len(seqs), "edges")


def check_workgroup_boundaries(eng):
    """ASCII chunk c is thread c % 256 of workgroup c // 256: sequences that end and begin exactly at chunk 256, and sequences
    that lie across chunks 256 and 512."""
    rng = np.random.default_rng(4102)
    for tag, lens, at, across in (("ends at 256", (256 * 32, 33, 300 * 32 + 5, 2 * 32, 7), {256}, {512}),
                                  ("across 256 and 512", (200 * 32 - 5, 100 * 32 + 1, 300 * 32 - 7, 17), set(), {256, 512})):
        seqs = [draw(rng, n) for n in lens]
        first = np.concatenate([[0], np.cumsum([n_chunks(s) for s in seqs])])
        assert at <= set(first.tolist())                              # a sequence begins there (and its neighbour ends there)
        for b in across:
            assert any(first[t] < b < first[t + 1] for t in range(len(seqs))), (tag, b)      # (it holds chunks b - 1 and b)
        for upper in (False, True):
            check_set(eng, seqs, [upper] * len(seqs), tag)


def check_counters_over_many_chunks(eng):
    """70 001 symbols outside upper-case ACGT, 1 000 of them invalid: the counters are sums over about 2 200 threads."""
    rng = np.random.default_rng(4103)
    n = 70001
    s = bytearray(draw(rng, n, b"acgtn"))
    for p in rng.choice(n, 1000, replace=False):
        s[p] = ord("X")
    s = bytes(s)
    seqs = [draw(rng, 100), s, draw(rng, 50)]
    for upper in (False, True):
        ss = check_set(eng, seqs, [upper] * 3, "counters")
        if not upper:
            assert ss.n_exc[1] == 70001
        assert ss.n_invalid[1] == 1000


# ---- b. every creating entry gives the same planes -------------------------------------------------------------------------
def _adopt(eng, handle, lens, info):
    """A SeqSet around a handle the library has just returned."""
    from vapor_amd.engine import SeqSet
    ss = SeqSet.__new__(SeqSet)
    ss.engine = eng
    ss.n_lit = ss.n = len(lens)
    ss.lens = np.asarray(lens, dtype=np.int32)
    ss._h = handle
    eng._live.add(ss)
    ss.n_exc = info[0::2][:ss.n].copy()
    ss.n_invalid = info[1::2][:ss.n].copy()
    return ss


def check_entries(eng):
    from vapor_amd.engine import SeqSet
    rng = np.random.default_rng(4104)
    seqs = [bytes(range(256)), b"", draw(rng, 33), rng.integers(0, 256, 95, dtype=np.uint8).tobytes(), draw(rng, 64), b"", draw(rng, 1000), b"n"]
    n = len(seqs)
    # a blob with other bytes between the sequences, so that an offset that is off by one shows
    blob, off = b"", []
    for s in seqs:
        blob += b"*" * 3
        off.append(len(blob))
        blob += s
    blob += b"*" * 5
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    off = np.asarray(off, dtype=np.int64)
    lens = np.asarray([len(s) for s in seqs], dtype=np.int32)
    for upper in (None, [t % 2 == 0 for t in range(n)]):
        # vapor_seqset_create: the blob and offsets
        flags = None if upper is None else np.asarray(upper, dtype=np.uint8) * np.uint8(L.SEQ_UPPER)
        info = np.zeros(2 * n, dtype=np.int32)
        h = ctypes.c_void_p()
        L.check(L.load().vapor_seqset_create(eng._ctx, n, L.ptr(buf, ctypes.c_uint8), L.ptr(off, ctypes.c_int64), L.ptr(lens, ctypes.c_int32),
                                             None if flags is None else L.ptr(flags, ctypes.c_uint8), L.ptr(info, ctypes.c_int32), ctypes.byref(h)))
        ss = _adopt(eng, h, lens, info)
        try:
            assert_set(ss, seqs, upper, "vapor_seqset_create")
        finally:
            ss.close()
        # vapor_seqset_create_ptrs: one pointer per sequence
        check_set(eng, seqs, upper, "vapor_seqset_create_ptrs")
    # SeqSet.from_addresses (it passes no flags)
    ss = SeqSet.from_addresses(eng, np.uint64(buf.ctypes.data) + off.astype(np.uint64), lens, keepalive=buf)
    try:
        assert_set(ss, seqs, None, "from_addresses")
    finally:
        ss.close()


# ---- c. the threaded staging path ----------------------------------------------------------------------------------------
def _cut(blob, lens):
    at = np.concatenate([[0], np.cumsum(lens)])
    assert at[-1] <= len(blob)
    return [blob[int(at[t]):int(at[t + 1])] for t in range(len(lens))]


def staging_layouts():
    """name -> the lengths of a set whose ASCII layout is at least one chunk past the switch, in at least STAGE_SWITCH_SEQS
    sequences."""
    rng = np.random.default_rng(4105)
    need = STAGE_SWITCH_BYTES + 32
    out = {}
    out["8 equal"] = [need // STAGE_SWITCH_SEQS + 13] * STAGE_SWITCH_SEQS
    short = [int(x) for x in rng.integers(need // 400, need // 200, 14)]                       # (14 of about 1/280: 5 % in all)
    out["one of 95 %"] = short[:7] + [need - sum(32 * ((x + 31) // 32) for x in short) - 3] + short[7:]
    long9 = [need // 9 + 101 + 32 * t for t in range(9)]
    z = []
    for t in range(9):
        z += [0] * 4 + [long9[t]]
    out["40 of length 0"] = z + [0] * 4
    many = [int(x) for x in rng.integers(1, 4001, 3000)]
    many[-1] += max(0, need - sum(32 * ((x + 31) // 32) for x in many))
    out["3 000 of 1 to 4 000"] = many
    return out


STAGING_LAYOUTS = ("8 equal", "one of 95 %", "40 of length 0", "3 000 of 1 to 4 000")


def _staging_texts(lens, seed):
    rng = np.random.default_rng(seed)
    return _cut(draw(rng, int(sum(lens))), lens)


def check_staging(eng, name, threads=STAGE_THREADS):
    lens = staging_layouts()[name]
    texts = _staging_texts(lens, 4106)
    assert len(texts) >= STAGE_SWITCH_SEQS and sum(map(n_chunks, texts)) * 32 >= STAGE_SWITCH_BYTES + 32     # (the sliced path)
    if name == "40 of length 0":
        assert lens.count(0) == 40 and len(lens) == 49 and lens[0] == 0 and lens[-1] == 0
    upper = [t % 5 == 2 for t in range(len(texts))]
    want = M.set_planes(texts, upper)
    try:
        for v in threads:
            eng.set_param("stage_threads", v)
            ss = eng.seqset(texts, upper=upper)
            try:
                assert ss.lens.tolist() == lens, (name, v)
                got = read_planes(ss)
                for a, b, what in zip(got, want[:3], ("p2", "e1", "x4")):
                    assert np.array_equal(a, b), (name, v, what, np.flatnonzero(a != b)[:4].tolist() if len(a) == len(b) else (len(a), len(b)))
                assert ss.n_exc.tolist() == want[3].tolist() and ss.n_invalid.tolist() == want[4].tolist(), (name, v)
            finally:
                ss.close()
    finally:
        eng.set_param("stage_threads", STAGE_THREADS_DEFAULT)


def check_single_thread_staging(eng):
    """One sequence fewer than the switch asks for, the same bytes in all: the single-thread path."""
    lens = [(STAGE_SWITCH_BYTES + 32) // (STAGE_SWITCH_SEQS - 1) + 13] * (STAGE_SWITCH_SEQS - 1)
    texts = _staging_texts(lens, 4106)
    assert len(texts) < STAGE_SWITCH_SEQS and sum(map(n_chunks, texts)) * 32 >= STAGE_SWITCH_BYTES + 32
    check_set(eng, texts, [t % 5 == 2 for t in range(len(texts))], "7 sequences")


# ---- d. derive_kernel against the spelled text -------------------------------------------------------------------------------
def derive_case():
    """(literals, [(segments, upper)]): parents and descriptors at the places where an assembling kernel goes wrong."""
    rng = np.random.default_rng(4107)

    def dna(n):
        return draw(rng, n, b"ACGT")
    w = bytearray(dna(4000))
    for a, b in ((300, 420), (1500, 1531), (3990, 4000)):                 # soft-masked stretches
        w[a:b] = bytes(w[a:b]).lower()
    w[800:807] = b"N" * 7
    w[1903:1906] = b"n" * 3
    w[1520:1524] = b"nnNN"
    lits = [bytes(w), dna(333), (b"acgtNn" * 130)[:777], dna(4000)[:2000] + dna(300).lower() + dna(1800), b"acgtNn"]
    W, P, Q, R, S = range(5)                                               # window, payload, two parents behind others, acgtNn
    der = []
    # a segment boundary at every dst % 32
    for r in range(32):
        der.append(([(W, 5 + r, 32 * 3 + r, False), (W, 1000 + 3 * r, 70, r % 2 == 1), (P, r, 40, False)], False))
    # source offsets off % 8 = 0..7, forward and reversed, from the first parent and from one behind others
    for o in range(8):
        for rc in (False, True):
            der.append(([(W, 296 + o, 77, rc)], False))
            der.append(([(Q, 104 + o, 45, rc), (R, 1992 + o, 70, not rc)], False))
    # sixteen segments of length 1 inside one chunk; sixteen of lengths 31, 32, 33
    assert L.MAX_SEGMENTS == 16
    der.append(([(W, 296 + 7 * j, 1, j % 2 == 1) for j in range(16)], False))
    der.append(([(R if j % 4 == 3 else W, 1400 + 29 * j, (31, 32, 33)[j % 3], j % 3 == 1) for j in range(16)], False))
    # segments of length 0 first, last and between others; derived sequences of length 0
    der.append(([(W, 10, 0, False), (W, 10, 50, False), (P, 5, 0, True), (W, 60, 50, True), (Q, 0, 0, False)], False))
    der.append(([], False))
    der.append(([(W, 5, 0, False)], False))
    # total lengths that are whole chunks
    der.append(([(W, 100, 32, False)], False))
    der.append(([(W, 100, 20, False), (P, 7, 44, True)], False))
    der.append(([(W, 0, 4000, False), (W, 0, 4000, True), (R, 8, 192, False)], False))
    # an upper twin over lower case and n; the same segments as they are
    twin = [(W, 290, 200, False), (W, 1890, 30, True), (Q, 3, 60, True), (R, 1990, 320, False)]
    der += [(twin, True), (twin, False)]
    # a reversed segment over acgtNn: n stays n, a becomes t, case survives
    der += [([(S, 0, 6, True)], False), ([(Q, 0, 777, True)], False), ([(S, 0, 6, True)], True)]
    # overlapping and repeated slices
    der.append(([(W, 100, 300, False), (W, 250, 300, False), (W, 100, 300, True), (W, 100, 300, False)], False))
    return lits, der


def check_derive(eng):
    lits, der = derive_case()
    texts = [M.spell(lits, sg, up) for sg, up in der]
    assert M.spell(lits, [(4, 0, 6, True)]) == b"nNacgt" and M.spell(lits, [(4, 0, 6, True)], True) == b"NNACGT"
    assert sum(map(n_chunks, texts)) > 256                                # more than one workgroup of derive_kernel
    assert {len(t) for t in texts} >= {0, 32, 64, 8192}
    assert {(len(M.spell(lits, sg[:1], up))) % 32 for sg, up in der[:32]} == set(range(32))
    ss = eng.seqset(lits, derived=der)
    try:
        assert_set(ss, lits + texts, None, "derived")
    finally:
        ss.close()


# ---- e. n_nocomp, exactly ------------------------------------------------------------------------------------------------------
def check_nocomp(eng):
    """A reverse-complemented segment is refused iff its parent holds a byte complementary() drops - for every byte value, in
    the middle, at the end and at the start of the parent; a forward segment is taken for every one."""
    flank = b"ACGT" * 10
    n_refused = 0
    for where in ("middle", "last", "first"):
        parents = []
        for b in range(256):
            one = bytes([b])
            parents.append({"middle": flank + one + flank, "last": flank + flank + one, "first": one + flank + flank}[where])
        for b, par in enumerate(parents):
            segs = [(0, 0, len(par), True)]
            if M.complementary_keeps(b):
                assert M.n_nocomp(par) == 0
                ss = eng.seqset([par], derived=[(segs, False)])
                try:
                    assert_set(ss, [par, M.spell([par], segs)], None, ("reversed", where, b))
                finally:
                    ss.close()
            else:
                assert M.n_nocomp(par) == 1
                with pytest.raises(L.VaporHipError) as ei:
                    eng.seqset([par], derived=[(segs, False)])
                assert ei.value.code == L.E_ARG, (where, b)
                n_refused += 1
        # forward segments over all of them, in one set
        fw = [([(b, 0, len(parents[b]), False)], False) for b in range(256)]
        ss = eng.seqset(parents, derived=fw)
        try:
            assert_set(ss, parents + parents, None, ("forward", where))
        finally:
            ss.close()
    assert n_refused == 3 * (256 - len(M.KEPT_BY_COMPLEMENTARY))


# ---- the tests ---------------------------------------------------------------------------------------------------------------
def test_pack_kernel_at_its_edges(eng):
    check_pack_edges(eng)


def test_sequences_at_workgroup_boundaries(eng):
    check_workgroup_boundaries(eng)


def test_counters_summed_over_thousands_of_chunks(eng):
    check_counters_over_many_chunks(eng)


def test_every_creating_entry_gives_the_models_planes(eng):
    check_entries(eng)


@pytest.mark.parametrize("layout", STAGING_LAYOUTS)
def test_threaded_staging(eng, layout):
    check_staging(eng, layout)


def test_single_thread_staging_of_a_large_upload(eng):
    check_single_thread_staging(eng)


def test_derive_kernel_against_the_spelled_text(eng):
    check_derive(eng)


def test_n_nocomp_for_every_byte_value(eng):
    check_nocomp(eng)


def test_device_held_reads_against_the_nibble_model(eng, tmp_path):
    """bam_expand_kernel + pack_kernel: the planes of sources of src_kind 1 and 2 over one 3 001-base read of all sixteen
    nibbles equal the model's planes of the text decoded from the read's own nibbles - no host text is uploaded."""
    from vapor_amd import bamio, seqio
    rng = np.random.default_rng(12)
    nib = rng.integers(0, 16, 3001)
    assert set(nib.tolist()) == set(range(16))
    p = str(tmp_path / "one.bam")
    bamio.write_bam(p, [("c", 9000)], [("r", 0, 100, "3001M", "".join(M.BAM_NIBBLES[j] for j in nib))])
    kf, addr, q0, _miss, status, batches = seqio.InProcessBam().chop_many_device(eng, p, ["c"], [101], [700], [100])
    try:
        assert int(kf[-1]) == 1 and int(q0[0]) == 0 and status.tolist() == [0]
        # (last base, length) of tests/test_gpu_both_ends.py's reverse-complemented sources, and whole chunks at even and odd bases
        spans = [(0, 1), (1, 1), (1, 2), (31, 32), (32, 33), (63, 64), (64, 33), (999, 1000), (1000, 1000), (2999, 777), (3000, 3001),
                 (3000, 31), (2001, 1025), (2002, 1025), (131, 32), (132, 32), (163, 64), (164, 64)]
        cases = [(2, last, n) for last, n in spans] + [(1, last - n + 1, n) for last, n in spans]      # (src_kind, first, length)
        assert {(k, f % 2) for k, f, n in cases if n in (32, 64)} == {(1, 0), (1, 1), (2, 0), (2, 1)}
        dev = eng.seqset_raw(np.full(len(cases), addr[0], dtype=np.uint64), np.asarray([c[2] for c in cases], dtype=np.int64), None,
                             src_kind=np.asarray([c[0] for c in cases], dtype=np.uint8), src_first=np.asarray([c[1] for c in cases], dtype=np.int64))
        try:
            assert_set(dev, [M.bam_text(nib, f, n, k) for k, f, n in cases], None, "device-held reads")
        finally:
            dev.close()
    finally:
        for bt in batches:
            bt.close()
