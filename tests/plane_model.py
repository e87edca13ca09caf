"""The sequence planes, stated once in numpy.  TEST INFRASTRUCTURE: it imports no kernel and nothing of vapor_amd; it is
written from the format's description (the comments at the top of vapor_amd/csrc/vapor_kernels.h), not from a
kernel's body, so that a plane a kernel writes can be compared with something that is not a kernel.

Symbol code of a byte: A C G T = 0..3, a c g t = 4..7, N and the IUPAC letters R Y S W K M B D H V = 8, their lower-case forms
= 9, everything else = 15; with the sequence's VAPOR_SEQ_UPPER flag a lower-case letter takes its upper-case letter's code.

Planes of a sequence of n symbols, ceil(n / 32) chunks:
    x4  4 words per chunk   symbol i is the nibble at bit 4 * (i % 8) of word i // 8
    p2  2 words per chunk   code & 3 for codes below 8, else 0, at bit 2 * (i % 16) of word i // 16
    e1  1 word per chunk    bit i % 32 of word i // 32 is set iff code >= 4
every bit behind symbol n - 1 is 0.  Counters: n_exc = codes of 4 or more, n_invalid = codes equal to 15, n_nocomp = bytes
that complementary() does not keep (it keeps ATGCNatgcn).

The vectorised functions (a 256-entry table and reshapes; one test packs more than 4 MiB) are what the tests use; the scalar_*
functions restate the same sentences one symbol at a time and are their self-check (tests/test_planes_cpu.py)."""
import numpy as np

IUPAC = "NRYSWKMBDHV"
KEPT_BY_COMPLEMENTARY = b"ATGCNatgcn"
BAM_NIBBLES = "=ACMGRSVTWYHKDBN"


def _code_table(upper):
    t = np.full(256, 15, dtype=np.uint32)
    for v, ch in enumerate("ACGT"):
        t[ord(ch)] = v
        t[ord(ch.lower())] = v if upper else v + 4
    for ch in IUPAC:
        t[ord(ch)] = 8
        t[ord(ch.lower())] = 8 if upper else 9
    return t


_TABLE = (_code_table(False), _code_table(True))
_KEPT = np.zeros(256, dtype=bool)
_KEPT[np.frombuffer(KEPT_BY_COMPLEMENTARY, dtype=np.uint8)] = True


def codes(seq, upper=False):
    """The symbol codes of a bytes sequence (uint32, one per byte)."""
    return _TABLE[1 if upper else 0][np.frombuffer(bytes(seq), dtype=np.uint8)]


def complementary_keeps(b):
    """Whether complementary() keeps byte value `b` (it drops what is not ATGCN / atgcn)."""
    return bool(_KEPT[b])


def n_nocomp(seq):
    return int((~_KEPT[np.frombuffer(bytes(seq), dtype=np.uint8)]).sum())


def _planes_of_padded(c):
    """p2, e1, x4 of codes laid out in whole 32-symbol chunks (the places behind a sequence's last symbol hold 0)."""
    x4 = (c.reshape(-1, 8) << (4 * np.arange(8, dtype=np.uint32))).sum(axis=1, dtype=np.uint32)
    two = np.where(c < 8, c & 3, 0).astype(np.uint32)
    p2 = (two.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint32)
    e1 = ((c >= 4).astype(np.uint32).reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)
    return p2, e1, x4


def planes(seq, upper=False):
    """(p2, e1, x4, n_exc, n_invalid) of one sequence."""
    c = codes(seq, upper)
    pad = np.zeros((len(c) + 31) // 32 * 32, dtype=np.uint32)
    pad[:len(c)] = c
    return _planes_of_padded(pad) + (int((c >= 4).sum()), int((c == 15).sum()))


def set_planes(seqs, upper=None):
    """The planes of every sequence of a set, one behind the other as a pass over the set reads them (sequence s owns
    ceil(len / 32) chunks; a sequence of length 0 owns nothing): (p2, e1, x4, n_exc[], n_invalid[])."""
    n = len(seqs)
    up = np.zeros(n, dtype=bool) if upper is None else np.asarray(upper, dtype=bool)
    lens = np.fromiter(map(len, seqs), dtype=np.int64, count=n)
    chunks = (lens + 31) // 32
    first = np.concatenate([[0], np.cumsum(chunks)])                     # first chunk of every sequence
    start = np.concatenate([[0], np.cumsum(lens)])                       # first byte of every sequence in the blob
    blob = np.frombuffer(b"".join(bytes(s) for s in seqs), dtype=np.uint8)
    owner = np.repeat(np.arange(n), lens)
    c = np.where(up[owner], _TABLE[1][blob], _TABLE[0][blob])
    pad = np.zeros(int(first[-1]) * 32, dtype=np.uint32)
    pad[first[owner] * 32 + (np.arange(len(blob)) - start[owner])] = c
    n_exc = np.bincount(owner, weights=c >= 4, minlength=n).astype(np.int64)
    n_inv = np.bincount(owner, weights=c == 15, minlength=n).astype(np.int64)
    return _planes_of_padded(pad) + (n_exc, n_inv)


def _complementary(s):
    """seqio.complementary's rule, restated: ATGCN / atgcn are complemented, everything else is dropped."""
    return bytes(s).translate(bytes.maketrans(b"ATGCNatgcn", b"TACGNtacgn"),
                              bytes(b for b in range(256) if b not in KEPT_BY_COMPLEMENTARY))


def spell(literals, segments, upper=False):
    """The text a descriptor list stands for: segments = [(parent, off, len, revcomp), ...] over the bytes of `literals`."""
    out = b""
    for par, off, ln, rc in segments:
        piece = bytes(literals[par])[off:off + ln]
        out += _complementary(piece)[::-1] if rc else piece
    return out.upper() if upper else out


def _rev4(nib):
    return ((nib & 1) << 3) | ((nib & 2) << 1) | ((nib & 4) >> 1) | ((nib & 8) >> 3)


def bam_text(nibbles, first, length, src_kind):
    """The text of a device-held read: `nibbles` the read's 4-bit bases (one per entry), src_kind 1 = the `length` bases from
    base `first` on, 2 = the complements (the nibble with its bits reversed) of base `first` and the bases before it."""
    nib = np.asarray(nibbles, dtype=np.uint8)
    t = np.arange(length)
    if src_kind == 1:
        got = nib[first + t]
    else:
        assert src_kind == 2
        got = _rev4(nib[first - t])
    return np.frombuffer(BAM_NIBBLES.encode(), dtype=np.uint8)[got].tobytes()


# ---- the same, one symbol at a time -------------------------------------------------------------------------------------
def scalar_code(b, upper=False):
    ch = chr(b)
    if not ("A" <= ch <= "Z" or "a" <= ch <= "z"):
        return 15
    lower = ch.islower()
    u = ch.upper()
    if u in "ACGT":
        base = "ACGT".index(u)
    elif u in IUPAC:
        base = 8
    else:
        return 15
    if lower and not upper:
        return base + 4 if base < 4 else 9
    return base


def scalar_planes(seq, upper=False):
    seq = bytes(seq)
    ch = (len(seq) + 31) // 32
    p2, e1, x4 = [0] * (2 * ch), [0] * ch, [0] * (4 * ch)
    n_exc = n_inv = 0
    for i, b in enumerate(seq):
        code = scalar_code(b, upper)
        x4[i // 8] |= code << (4 * (i % 8))
        if code < 8:
            p2[i // 16] |= (code & 3) << (2 * (i % 16))
        if code >= 4:
            e1[i // 32] |= 1 << (i % 32)
            n_exc += 1
        if code == 15:
            n_inv += 1
    return np.asarray(p2, dtype=np.uint32), np.asarray(e1, dtype=np.uint32), np.asarray(x4, dtype=np.uint32), n_exc, n_inv


def scalar_n_nocomp(seq):
    return sum(1 for b in bytes(seq) if chr(b) not in "ATGCNatgcn")


def scalar_spell(literals, segments, upper=False):
    comp = {"A": "T", "T": "A", "G": "C", "C": "G", "N": "N", "a": "t", "t": "a", "g": "c", "c": "g", "n": "n"}
    out = []
    for par, off, ln, rc in segments:
        piece = [chr(b) for b in bytes(literals[par])[off:off + ln]]
        if rc:
            piece = [comp[ch] for ch in piece if ch in comp]
            piece.reverse()
        out += piece
    text = "".join(out)
    if upper:
        text = "".join(chr(ord(ch) - 32) if "a" <= ch <= "z" else ch for ch in text)
    return text.encode("latin-1")


def scalar_bam_text(nibbles, first, length, src_kind):
    out = []
    for t in range(length):
        if src_kind == 1:
            nib = int(nibbles[first + t])
        else:
            nib = int("{:04b}".format(int(nibbles[first - t]))[::-1], 2)
        out.append(BAM_NIBBLES[nib])
    return "".join(out).encode()
