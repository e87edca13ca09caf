"""The host plan of a sequence set's creation (vapor_amd/csrc/vapor_seqset_plan.h) on the four real entries, on the paths the other
tests of the planes do not reach: every refusal that needs no large input, with its code and the text vapor_last_error gives, each
followed by a good call of the same entry on the same context whose planes equal tests/plane_model.py; the empty set, a set of
sequences of no symbols, a derived sequence of no symbols, and a mixed call that names no device-held source, which is an ordinary
derived call.  A refused call reads nothing it is given: the device source "outside every live batch" is an address nobody owns.
The arithmetic behind these answers is what tests/test_seqset_cpu.py holds to its rules on the host."""
import ctypes

import numpy as np
import pytest

import plane_model as M
from test_gpu_planes import ALPHABET, _adopt, assert_set, draw
from vapor_amd import _lib as L

pytestmark = pytest.mark.gpu

ENTRIES = ("vapor_seqset_create", "vapor_seqset_create_ptrs", "vapor_seqset_create_derived", "vapor_seqset_create_mixed")
BLOB, PTRS, DERIVED, MIXED = ENTRIES
MOST_SEQS = 0x7FFFFFF0
REVCOMP_DROPS = ("vapor_seqset_create_derived: a reverse-complemented segment's parent holds characters complementary() drops "
                 "(outside ATGCN/atgcn, SF:471-478); upload that allele as bytes")
OUTSIDE = "vapor_seqset_create_derived: segment outside its parent"
COUNT = "vapor_seqset_create_derived: bad segment count"
BAD_SOURCE = "vapor_seqset_create_mixed: bad source description"


@pytest.fixture(scope="module")
def eng():
    from vapor_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


class Args:
    """The arguments of a good call: eight literals (one upper-cased, one of no symbols) and, for the entries that take them, three
    derived sequences (one of no symbols).  A test spoils a field, then calls."""

    def __init__(self, texts=None, derived=None, upper=None):
        rng = np.random.default_rng(4201)
        # (literal 5 is reversed by a derived sequence: nothing in it that complementary() drops)
        self.texts = [draw(rng, n, b"ACGTacgtNn" if n == 1000 else ALPHABET) for n in (95, 0, 33, 64, 1, 1000, 31, 32)] if texts is None else texts
        n = len(self.texts)
        self.derived = [([(0, 3, 40, False), (5, 100, 64, True)], False), ([], False), ([(2, 0, 33, False), (3, 1, 0, True)], True)] if derived is None else derived
        self.upper = [t == 2 for t in range(n)] if upper is None else upper
        self.ctx_there = self.out_there = True
        self.n = n
        self.blob = np.frombuffer(b"*" + b"**".join(self.texts) + b"*", dtype=np.uint8).copy()
        self.off = np.asarray([1 + sum(len(t) + 2 for t in self.texts[:i]) for i in range(n)] + [0], dtype=np.int64)
        self.lens = np.asarray([len(t) for t in self.texts] + [0], dtype=np.int32)
        self.bufs = [np.frombuffer(t + b"*", dtype=np.uint8).copy() for t in self.texts]
        self.ptrs = np.asarray([b.ctypes.data for b in self.bufs] + [0], dtype=np.uint64)
        self.flags = np.asarray([L.SEQ_UPPER if u else 0 for u in self.upper] + [0], dtype=np.uint8)
        self.kind = np.zeros(n + 1, dtype=np.uint8)
        self.first = np.zeros(n + 1, dtype=np.int64)
        self.n_derived = len(self.derived)
        self.seg_first = np.concatenate([[0], np.cumsum([len(sg) for sg, _u in self.derived])]).astype(np.int32)
        self.segs = np.zeros(max(int(self.seg_first[-1]), 1), dtype=L.SEG_DTYPE)
        for w, (par, off, ln, rc) in enumerate(x for sg, _u in self.derived for x in sg):
            self.segs[w] = (par, off, ln, L.SEG_REVCOMP if rc else 0)
        self.dflags = np.asarray([L.SEQ_UPPER if u else 0 for _sg, u in self.derived] + [0], dtype=np.uint8)
        self.no = set()                                      # the arrays handed over as NULL

    def texts_of(self, entry):
        """What the set of a good call holds."""
        if entry in (BLOB, PTRS):
            return self.texts, self.upper
        lits = [t.upper() if u else t for t, u in zip(self.texts, self.upper)]          # (a parent's planes hold what was packed)
        return self.texts + [M.spell(lits, sg, up) for sg, up in self.derived], self.upper + [False] * len(self.derived)

    def call(self, eng, entry):
        """(status, vapor_last_error's text, handle, seq_info)"""
        def arr(name, ctype=None):
            a = getattr(self, name)
            if name in self.no:
                return None
            return a.ctypes.data_as(ctypes.c_void_p) if ctype is None else L.ptr(a, ctype)
        lib = L.load()
        nd = self.n_derived if entry in (DERIVED, MIXED) else 0
        info = np.full(2 * max(self.n + max(nd, 0), 1) + 2, -7, dtype=np.int32) if 0 <= self.n < 1000 and nd < 1000 else np.zeros(2, np.int32)
        h = ctypes.c_void_p()
        ctx = eng._ctx if self.ctx_there else ctypes.c_void_p()
        out = ctypes.byref(h) if self.out_there else None
        ip = L.ptr(info, ctypes.c_int32)
        ptrs = None if "ptrs" in self.no else ctypes.cast(self.ptrs.ctypes.data, ctypes.POINTER(ctypes.c_void_p))
        if entry == BLOB:
            rc = lib.vapor_seqset_create(ctx, self.n, arr("blob", ctypes.c_uint8), arr("off", ctypes.c_int64), arr("lens", ctypes.c_int32),
                                         arr("flags", ctypes.c_uint8), ip, out)
        elif entry == PTRS:
            rc = lib.vapor_seqset_create_ptrs(ctx, self.n, ptrs, arr("lens", ctypes.c_int32), arr("flags", ctypes.c_uint8), ip, out)
        elif entry == DERIVED:
            rc = lib.vapor_seqset_create_derived(ctx, self.n, ptrs, arr("lens", ctypes.c_int32), arr("flags", ctypes.c_uint8), self.n_derived,
                                                 arr("seg_first", ctypes.c_int32), arr("segs"), arr("dflags", ctypes.c_uint8), ip, out)
        else:
            rc = lib.vapor_seqset_create_mixed(ctx, self.n, None if "ptrs" in self.no else self.ptrs.ctypes.data_as(ctypes.c_void_p), arr("lens"), arr("flags"),
                                               arr("kind"), arr("first"), self.n_derived, arr("seg_first"), arr("segs"), arr("dflags"), ip, out)
        return rc, lib.vapor_last_error().decode(), h, info


def good_call(eng, entry, a=None):
    a = a or Args()
    rc, msg, h, info = a.call(eng, entry)
    assert rc == 0, (entry, msg)
    texts, upper = a.texts_of(entry)
    ss = _adopt(eng, h, [len(t) for t in texts], info)
    try:
        assert_set(ss, texts, upper, entry)
        assert len(info) > 2 * len(texts) and (info[2 * len(texts):] == -7).all(), entry      # (seq_info ends with the caller's sequences)
    finally:
        ss.close()


def _set(name, index, value):
    def spoil(a):
        getattr(a, name)[index] = value
    return spoil


def _attr(name, value):
    def spoil(a):
        setattr(a, name, value)
    return spoil


def _null(*names):
    def spoil(a):
        a.no |= set(names)
    return spoil


def _seg(d, field, value):
    def spoil(a):
        a.segs[field][int(a.seg_first[d])] = value
    return spoil


def _all(*spoils):
    def spoil(a):
        for s in spoils:
            s(a)
    return spoil


def _seventeen(a):
    a.n_derived = 1
    a.seg_first = np.asarray([0, 17], dtype=np.int32)
    a.segs = np.zeros(17, dtype=L.SEG_DTYPE)
    a.segs["len"] = 1


def _device_source(kind, first, addr=0x1000, length=None):
    """Literal 3 as a device-held source at an address nobody owns."""
    def spoil(a):
        a.kind[3], a.first[3], a.ptrs[3] = kind, first, addr
        if length is not None:
            a.lens[3] = length
    return spoil


EVERY, NOT_BLOB, DER = ENTRIES, ENTRIES[1:], ENTRIES[2:]
# (what is spoilt, the entries that can make the refusal, its text - "{}:" the entry's own name)
REFUSALS = [
    ("no context", _attr("ctx_there", False), EVERY, "{}: null argument"),
    ("no output", _attr("out_there", False), EVERY, "{}: null argument"),
    ("a count below 0", _attr("n", -1), EVERY, "{}: null argument"),
    ("no sources", _null("blob", "ptrs"), EVERY, "{}: null argument"),
    ("no offsets", _null("off"), (BLOB,), "{}: null argument"),
    ("no lengths", _null("lens"), EVERY, "{}: null argument"),
    ("a derived count below 0", _attr("n_derived", -1), DER, "{}: null argument"),
    ("no seg_first", _null("seg_first"), DER, "{}: null argument"),
    ("no segments", _null("segs"), DER, "{}: null argument"),
    ("too many sequences", _attr("n_derived", MOST_SEQS - 8 + 1), DER, "{}: too many sequences"),
    ("a null sequence", _set("ptrs", 5, 0), NOT_BLOB, "{}: null sequence"),
    ("a negative length", _set("lens", 4, -1), EVERY, "negative sequence length"),
    ("a negative length before a null sequence", _all(_set("ptrs", 6, 0), _set("lens", 2, -3)), (MIXED,), "negative sequence length"),
    ("a null sequence whatever the lengths", _all(_set("ptrs", 6, 0), _set("lens", 2, -3)), (PTRS, DERIVED), "{}: null sequence"),
    ("source kind 3", _set("kind", 3, 3), (MIXED,), BAD_SOURCE),
    ("no first bases", _all(_device_source(1, 0), _null("first")), (MIXED,), BAD_SOURCE),
    ("a first base below 0", _device_source(1, -1), (MIXED,), BAD_SOURCE),
    ("a first base too far", _device_source(1, MOST_SEQS + 1), (MIXED,), BAD_SOURCE),
    ("a reversed source that begins below base 0", _device_source(2, 62), (MIXED,), BAD_SOURCE),
    ("a device source nobody owns", _device_source(1, 10), (MIXED,), "{}: a device source outside every live batch"),
    ("a reversed device source nobody owns", _device_source(2, 63), (MIXED,), "{}: a device source outside every live batch"),
    ("segment lists that descend", _all(_attr("n_derived", 1), _set("seg_first", 1, -1)), DER, COUNT),
    ("seventeen segments", _seventeen, DER, COUNT),
    ("a parent below 0", _seg(0, "parent", -1), DER, OUTSIDE),
    ("a parent that is no literal", _seg(2, "parent", 8), DER, OUTSIDE),
    ("a segment offset below 0", _seg(0, "off", -1), DER, OUTSIDE),
    ("a segment length below 0", _seg(2, "len", -1), DER, OUTSIDE),
    ("a segment that ends behind its parent", _seg(0, "len", 93), DER, OUTSIDE),
    ("not upper-cased over an upper-cased parent", _set("dflags", 2, 0), DER,
     "vapor_seqset_create_derived: a derived sequence without VAPOR_SEQ_UPPER over a parent uploaded with it"),
]
CASES = [pytest.param(entry, spoil, text, id="%s-%s" % (entry[len("vapor_seqset_"):], name.replace(" ", "_")))
         for name, spoil, entries, text in REFUSALS for entry in entries]


@pytest.mark.parametrize("entry,spoil,text", CASES)
def test_a_refusal_says_what_it_is_and_the_next_call_is_good(eng, entry, spoil, text):
    a = Args()
    assert a.texts[0] and len(a.texts[0]) == 95 and len(a.texts[3]) == 64             # (what the segment and source cases lean on)
    spoil(a)
    rc, msg, h, _info = a.call(eng, entry)
    assert (rc, msg) == (L.E_ARG, text.format(entry)) and not h.value
    good_call(eng, entry)


@pytest.mark.parametrize("entry", DER)
def test_a_reversed_segment_over_a_dropped_character_is_refused_after_the_counts(eng, entry):
    a = Args()
    a.texts[5] = a.texts[5][:120] + b"R" + a.texts[5][121:]                           # (derived sequence 0 reverses 100 .. 164 of literal 5)
    rc, msg, h, _info = Args(texts=a.texts).call(eng, entry)
    assert (rc, msg) == (L.E_ARG, REVCOMP_DROPS) and not h.value
    good_call(eng, entry)


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_empty_set(eng, entry):
    good_call(eng, entry, Args(texts=[], derived=[], upper=[]))
    if entry in DER:
        good_call(eng, entry, Args(texts=[], derived=[([], False), ([], True)], upper=[]))


@pytest.mark.parametrize("entry", ENTRIES)
def test_sequences_of_no_symbols_only(eng, entry):
    good_call(eng, entry, Args(texts=[b""] * 5, derived=[([], False), ([(3, 0, 0, True)], False)], upper=[False, True] * 2 + [False]))


@pytest.mark.parametrize("entry", DER)
def test_a_derived_sequence_of_no_symbols_among_others(eng, entry):
    a = Args()
    assert a.derived[1] == ([], False) and a.derived[2][0][1][2] == 0
    good_call(eng, entry, a)
    good_call(eng, entry, Args(derived=[([(1, 0, 0, False), (0, 5, 0, True)], False)]))     # (the only one, over the literal of no symbols too)


def test_a_mixed_call_without_device_sources_is_a_derived_call(eng):
    """src_kind all 0: no mixed block, one copy of ASCII and map, the planes of vapor_seqset_create_derived."""
    a = Args()
    assert not a.kind.any()
    good_call(eng, MIXED, a)
    a.no.add("first")                                                                 # (nobody reads first bases then)
    good_call(eng, MIXED, a)
    got = []
    for entry in DER:
        rc, msg, h, info = Args().call(eng, entry)
        assert rc == 0, msg
        texts, _upper = Args().texts_of(entry)
        ss = _adopt(eng, h, [len(t) for t in texts], info)
        try:
            got.append([ss.planes(t) for t in range(ss.n)] + [info.tolist()])
        finally:
            ss.close()
    assert all(np.array_equal(x, y) for p, q in zip(got[0][:-1], got[1][:-1]) for x, y in zip(p, q)) and got[0][-1] == got[1][-1]
