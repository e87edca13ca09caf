"""A free-form DEFLATE writer (RFC 1951) for the decoders' tests: the caller chooses the token list and every code length, so
the streams are legal forms that zlib's encoder never writes - codes of 15 bits together with the widest extra fields, code
lengths in any order, alphabets padded to 286 / 30 symbols, code-length codes of 7 bits with or without the run symbols,
length 258 as symbol 284 + extra 31, a lone one-bit distance code, no distance code at all, empty stored blocks anywhere.
Every stream handed out has been inflated by zlib (zlib.decompressobj(-15)) and compared with the bytes it was made from:
the reference is zlib, never a decoder of this project.  A helper module: no tests in it.

  forms(seed) / all_forms(seed)  the named families (a) .. (f), seeded, in a fixed order: (family, stream, data) triples
  encode(data, rng, family)      *given* bytes (FASTA text, BAM records) as one stream of that family
  bgzf_block_maker(seed, fams)   a replacement for bamio._bgzf_block that encodes block after block, round-robin over fams
  write_records(path, items)     the streams as the record file `tools/bamdev_emu.cpp --forms` reads"""
import bisect
import random
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FAMILIES = ("long_codes", "headers", "match_queue", "stored", "size_edge", "mixed")
CHAIN = list(range(1, 16)) + [15]                      # the 16 leaves of the deepest code: 1, 2, .. 14, 15, 15


class BitWriter:
    """Bits go out least significant first; Huffman codes are handed in already reversed (canonical_codes does that)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, k):
        self.acc |= value << self.n
        self.n += k
        if self.n >= 512:
            whole = self.n >> 3
            self.out += (self.acc & ((1 << (whole * 8)) - 1)).to_bytes(whole, "little")
            self.acc >>= whole * 8
            self.n -= whole * 8

    def bitpos(self):
        return len(self.out) * 8 + self.n

    def align(self):
        self.bits(0, -self.n & 7)

    def raw(self, data):
        self.align()
        self.out += self.acc.to_bytes(self.n >> 3, "little")
        self.acc = self.n = 0
        self.out += data

    def getvalue(self):
        self.align()
        return bytes(self.out) + self.acc.to_bytes(self.n >> 3, "little")


def canonical_codes(lengths):
    """[(code with its bits reversed, length)] per symbol, RFC 1951 3.2.2; (0, 0) for a symbol without a code."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if not l:
            out.append((0, 0))
            continue
        c = nxt[l]
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def kraft_complete(lengths):
    return sum(1 << (15 - l) for l in lengths if l) == 1 << 15


def split_shape(rng, leaves, max_len=15, bias=2.0):
    """The leaf depths of a complete binary code with `leaves` >= 2 leaves, none deeper than max_len, by splitting a random leaf
    again and again; a leaf of depth d is chosen with weight bias^d (bias 1: any leaf alike; a large bias: the deepest, which ends
    in the chain 1, 2, 3 .. while leaves last).  Sorted, deepest first."""
    assert 2 <= leaves <= 1 << max_len
    cnt = [0] * (max_len + 1)
    cnt[1] = 2
    for _ in range(leaves - 2):
        ws = [cnt[d] * bias ** d for d in range(max_len)]
        x = rng.random() * sum(ws)
        d = 0
        for d in range(max_len):
            x -= ws[d]
            if x < 0 and cnt[d]:
                break
        else:
            d = max(d for d in range(max_len) if cnt[d])
        cnt[d] -= 1
        cnt[d + 1] += 2
    return [d for d in range(max_len, 0, -1) for _ in range(cnt[d])]


def assign_lengths(rng, size, used, shape, pinned=None):
    """Code lengths for an alphabet of `size` symbols: the depths of `shape` dealt at random to the symbols of `used`, except
    that pinned[symbol] = depth is honoured where the shape has such a leaf; leaves left over go to symbols outside `used`
    (padding symbols: they have a code and never occur)."""
    used = list(dict.fromkeys(used))
    assert len(used) <= len(shape) <= size, (len(used), len(shape), size)
    pool = list(shape)
    lengths = [0] * size
    rest = []
    for s in used:
        want = (pinned or {}).get(s)
        if want is not None and want in pool:
            pool.remove(want)
            lengths[s] = want
        else:
            rest.append(s)
    rng.shuffle(pool)
    for s in rest:
        lengths[s] = pool.pop()
    spare = [s for s in range(size) if not lengths[s]]
    rng.shuffle(spare)
    for s in spare[:len(pool)]:
        lengths[s] = pool.pop()
    assert not pool and kraft_complete(lengths)
    return lengths


def length_symbol(length, alt258=False):
    if length == 258:
        return (284, 5, 31) if alt258 else (285, 0, 0)
    i = bisect.bisect_right(LEN_BASE, length) - 1
    if i == 28:
        i = 27
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_symbol(dist):
    i = bisect.bisect_right(DIST_BASE, dist) - 1
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def symbolize(tokens, rng=None, alt258=False):
    """Tokens ('L', byte) / ('M', len, dist) as (ll symbol, extra bits, extra value, dist symbol, extra bits, extra value)
    (dist symbol -1 for a literal); with alt258 a length of 258 is written as 284 + 31 now and then."""
    out = []
    for t in tokens:
        if t[0] == "L":
            out.append((t[1], 0, 0, -1, 0, 0))
        else:
            assert 3 <= t[1] <= 258 and 1 <= t[2] <= 32768, t
            out.append(length_symbol(t[1], alt258 and rng.random() < 0.6) + dist_symbol(t[2]))
    return out


def expand(tokens, prefix=b""):
    """What the tokens spell behind `prefix` (the module's own LZ77 expansion; zlib has the last word in checked())."""
    out = bytearray(prefix)
    for t in tokens:
        if t[0] == "L":
            out.append(t[1])
        else:
            _m, length, dist = t
            assert dist <= len(out)
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
    return bytes(out[len(prefix):])


# ---- blocks -----------------------------------------------------------------------------------------------------------------
def stored_block(w, data, final=False):
    assert len(data) <= 65535
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.raw(struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + bytes(data))


_FIXED_LL = canonical_codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_D = canonical_codes([5] * 32)


def _body(w, syms, ll, dc):
    for s, xb, xv, d, dxb, dxv in syms:
        c, l = ll[s]
        assert l, ("no code for literal / length symbol", s)
        w.bits(c, l)
        if d >= 0:
            if xb:
                w.bits(xv, xb)
            c, l = dc[d]
            assert l, ("no code for distance symbol", d)
            w.bits(c, l)
            if dxb:
                w.bits(dxv, dxb)
    c, l = ll[256]
    w.bits(c, l)


def fixed_block(w, tokens, final=False, rng=None, alt258=False):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    _body(w, symbolize(tokens, rng, alt258), _FIXED_LL, _FIXED_D)


def cl_symbols(seq, rng, runs):
    """The code-length sequence as symbols of the code-length alphabet: (symbol, extra bits, extra value).  With runs, symbols
    16 / 17 / 18 of random reach wherever a run allows one (a run does not stop where the distance lengths begin)."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        j = i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if runs and v == 0 and run >= 3 and rng.random() < 0.9:
            rep = rng.randint(3, min(run, 138)) if rng.random() < 0.5 else min(run, 138)
            out.append((17, 3, rep - 3) if rep <= 10 else (18, 7, rep - 11))
            i += rep
        elif runs and i > 0 and seq[i - 1] == v and run >= 3 and rng.random() < 0.9:
            rep = rng.randint(3, min(run, 6))
            out.append((16, 2, rep - 3))
            i += rep
        else:
            out.append((v, 0, 0))
            i += 1
    return out


def dynamic_block(w, tokens, ll_len, d_len, rng, final=False, runs=True, cl_bias=2.0, cl_leaves=None, wide=False, alt258=False,
                  hclen=None):
    """One dynamic block.  ll_len / d_len: the code lengths (the caller's choice; only the symbols the tokens use must have one).
    wide: HLIT 286 and HDIST 30 whatever the last symbol with a code is.  The code-length code is complete, of cl_leaves
    leaves (all 19 when None) and up to 7 bits, its longest codes on the symbols the header uses.  Returns the header's bits."""
    syms = symbolize(tokens, rng, alt258)
    hlit = 286 if wide else max(257, max(i for i, l in enumerate(ll_len) if l) + 1)
    hdist = 30 if wide else max([1] + [i + 1 for i, l in enumerate(d_len) if l])
    ll_len = (list(ll_len) + [0] * 286)[:hlit]
    d_len = (list(d_len) + [0] * 30)[:hdist]
    cls = cl_symbols(ll_len + d_len, rng, runs)
    used = list(dict.fromkeys(s for s, _b, _v in cls))
    leaves = max(cl_leaves or 19, len(used), 2)
    shape = split_shape(rng, leaves, 7, cl_bias)          # (deepest first: assign_lengths pops from the end, so reverse)
    pl = [0] * 19
    order = used + rng.sample([s for s in range(19) if s not in used], leaves - len(used))
    for s, d in zip(order, shape):
        pl[s] = d
    assert kraft_complete(pl)
    n_cl = max(4, max(i for i, s in enumerate(CL_ORDER) if pl[s]) + 1)
    if hclen is not None:
        n_cl = max(n_cl, hclen)
    start = w.bitpos()
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(n_cl - 4, 4)
    for s in CL_ORDER[:n_cl]:
        w.bits(pl[s], 3)
    pc = canonical_codes(pl)
    for s, xb, xv in cls:
        w.bits(pc[s][0], pc[s][1])
        if xb:
            w.bits(xv, xb)
    header_bits = w.bitpos() - start
    _body(w, syms, canonical_codes(ll_len), canonical_codes(d_len))
    return header_bits


def used_symbols(tokens):
    ll, dd = {256}, set()
    for t in tokens:
        if t[0] == "L":
            ll.add(t[1])
        else:
            ll.add(length_symbol(t[1])[0])
            if t[1] == 258:
                ll.add(284)                                # (either way of writing 258 must have a code)
            dd.add(dist_symbol(t[2])[0])
    return sorted(ll), sorted(dd)


def choose_lengths(tokens, rng, style="random", bias=2.0, pad=None, pinned_ll=None, pinned_d=None):
    """Code lengths for the tokens' symbols.  style: 'random' (leaf splitting with the depth bias), 'chain' (the deepest code;
    symbols beyond its 16 leaves force random splitting of the deepest leaves instead), 'flat' (bias 1).  pad: how many
    padding symbols get a code too (None: a random few; 'all': every symbol of 286 / 30)."""
    ul, ud = used_symbols(tokens)

    def one(size, used, pinned, least):
        if len(used) == 1 and least == 1:
            return [1 if s == used[0] else 0 for s in range(size)]      # (the lone one-bit code zlib accepts)
        extra = size - len(used) if pad == "all" else (pad if pad is not None else rng.choice([0, 0, 1, 3, 20]))
        n = max(min(len(used) + extra, size), 2)
        if style == "chain" and n <= 16:
            shape = sorted(CHAIN[:n - 1] + [CHAIN[n - 2]], reverse=True) if n < 16 else sorted(CHAIN, reverse=True)
        else:
            shape = split_shape(rng, n, 15, {"flat": 1.0, "chain": 64.0}.get(style, bias))
        return assign_lengths(rng, size, used, shape, pinned)
    ll = one(286, ul, pinned_ll, 2)
    dl = one(30, ud, pinned_d, 1) if ud else ([0] * 30 if rng.random() < 0.5 else one(30, [rng.randrange(30)], None, 1))
    return ll, dl


# ---- a tokenizer for given data --------------------------------------------------------------------------------------------
class Tokenizer:
    """Free token choices for given bytes: at each position a literal, or any earlier occurrence of the next three bytes (found
    through an index of all 3-grams) cut to a random length; biased towards distance 1, distances below the length, lengths
    3 / 64 / 65 / 257 / 258 and distances up to 32 768."""

    def __init__(self, data, rng, p_literal=0.25):
        self.data, self.rng, self.p_literal = bytes(data), rng, p_literal
        self.index = {}                                    # 3-gram -> its positions in the whole of data, ascending
        d, ix = self.data, self.index
        for p in range(len(d) - 2):
            ix.setdefault(d[p:p + 3], []).append(p)

    def tokens(self, start, end):
        """Tokens that spell data[start:end) (a match may reach back before start, into other blocks)."""
        d, rng = self.data, self.rng
        out, i = [], start
        while i < end:
            if end - i < 3 or rng.random() < self.p_literal:
                out.append(("L", d[i]))
                i += 1
                continue
            lst = self.index[d[i:i + 3]]
            hi = bisect.bisect_left(lst, i)                # (the occurrences in front of i, no more than 32 768 back: lst[lo:hi])
            lo = bisect.bisect_left(lst, i - 32768, 0, hi)
            if lo == hi:
                out.append(("L", d[i]))
                i += 1
                continue
            r = rng.random()
            if r < 0.3 and d[i - 1:i + 2] == d[i:i + 3]:
                src = i - 1
            elif r < 0.55:
                src = lst[hi - 1]                          # the nearest (periodic data: distance below the length)
            elif r < 0.8:
                src = lst[lo]                              # the farthest inside the window
            else:
                src = lst[rng.randrange(lo, hi)]
            cap = min(258, end - i)
            m = 3
            while m < cap and d[src + m] == d[i + m]:
                m += 1
            r = rng.random()
            if r < 0.4:
                length = m
            elif r < 0.7:
                length = rng.choice([x for x in (3, 64, 65, 257, 258) if x <= m])
            else:
                length = rng.randint(3, m)
            out.append(("M", length, i - src))
            i += length
        return out


# ---- checking ---------------------------------------------------------------------------------------------------------------
def checked(stream, data):
    """The stream, once zlib has inflated it to exactly `data` and found its end."""
    z = zlib.decompressobj(-15)
    got = z.decompress(stream)
    assert z.eof and not z.unused_data and got == bytes(data), "deflate_forms wrote a stream zlib reads otherwise (%d bytes for %d)" % (len(got), len(data))
    return stream


def _random_dynamic(w, tokens, rng, final, style=None, **kw):
    style = style or rng.choice(["random", "random", "chain", "flat"])
    ll, dl = choose_lengths(tokens, rng, style, bias=rng.choice([1.3, 2.0, 4.0, 16.0]), pad=rng.choice([None, None, 0, "all"]))
    return dynamic_block(w, tokens, ll, dl, rng, final=final, runs=kw.pop("runs", rng.random() < 0.6), cl_bias=rng.choice([1.0, 2.0, 64.0]),
                         cl_leaves=rng.choice([None, None, 2, 8]), wide=kw.pop("wide", rng.random() < 0.4), alt258=kw.pop("alt258", rng.random() < 0.5), **kw)


def final_match(data):
    """(258, distance) where the last 258 bytes of data stand earlier in it, no more than 32 768 back (the nearest such place);
    else the same for the last 3 bytes; else None."""
    n = len(data)
    for length in (258, 3):
        if n > length:
            src = data.rfind(data[n - length:], max(0, n - length - 32768), n - 1)
            if src >= 0:
                return length, n - length - src
    return None


def encode(data, rng, family="mixed"):
    """Given bytes as one stream of a family: 'long_codes' (one dynamic block, chain or strongly depth-biased codes with the widest
    length and distance symbols on 15 bits where the data has such matches), 'match_queue' (match-heavy dynamic blocks with the
    header change right behind matches), 'stored' (stored blocks - empty ones too - between Huffman blocks), 'headers' (a
    fixed-code block, then the widest header), 'size_edge' (one dynamic block whose last token is final_match(data): a match
    that ends with the data; 'mixed' where the data has none), 'mixed' (1 - 6 blocks of all kinds)."""
    data = bytes(data)
    n = len(data)
    w = BitWriter()
    if family == "long_codes":
        tk = Tokenizer(data, rng, p_literal=0.35)
        tokens = tk.tokens(0, n)
        ul, ud = used_symbols(tokens)
        freq = {}
        for t in tokens:
            if t[0] == "L":
                freq[t[1]] = freq.get(t[1], 0) + 1
        common = sorted(freq, key=lambda s: -freq[s])
        pin_ll = {s: 15 for s in (281, 282, 283, 284)}
        for s, l in zip(common, (8, 9, 3, 5, 4, 6)):
            pin_ll[s] = l
        shape_n = min(286, max(len(ul) + 4, 24))
        ll = assign_lengths(rng, 286, ul, split_shape(rng, shape_n, 15, 3.0), pin_ll)
        dl = assign_lengths(rng, 30, ud, split_shape(rng, min(30, max(len(ud) + 2, 18)), 15, 64.0), {28: 15, 29: 15}) if ud else [0] * 30
        dynamic_block(w, tokens, ll, dl, rng, final=True, runs=rng.random() < 0.5, cl_bias=64.0, wide=rng.random() < 0.5, alt258=True)
        return checked(w.getvalue(), data)
    if family == "size_edge" and final_match(data):
        length, dist = final_match(data)
        tokens = Tokenizer(data, rng, p_literal=0.2).tokens(0, n - length) + [("M", length, dist)]
        _random_dynamic(w, tokens, rng, True, alt258=True)
        return checked(w.getvalue(), data)
    tk = Tokenizer(data, rng, p_literal={"match_queue": 0.05, "stored": 0.3}.get(family, rng.choice([0.1, 0.3, 0.6])))
    if family == "headers":
        k = rng.randrange(0, min(n, 1500) + 1)
        fixed_block(w, [("L", c) for c in data[:k]], final=False)
        if rng.random() < 0.3:
            stored_block(w, b"")
        _random_dynamic(w, tk.tokens(k, n), rng, True, style="random", runs=False, wide=True)
        return checked(w.getvalue(), data)
    pieces = rng.randint(1, 6)
    cuts = sorted(rng.randrange(0, n + 1) for _ in range(pieces - 1)) + [n]
    pos = 0
    for bi, cut in enumerate(cuts):
        final = bi == len(cuts) - 1
        kind = rng.choice({"stored": ["stored", "stored", "dynamic", "fixed"], "match_queue": ["dynamic", "dynamic", "fixed"]}.get(
            family, ["stored", "fixed", "dynamic", "dynamic"]))
        if kind == "stored":
            while cut - pos > 65535:                       # (LEN is 16 bits)
                stored_block(w, data[pos:pos + 65535])
                pos += 65535
            stored_block(w, data[pos:cut], final)
        elif kind == "fixed":
            fixed_block(w, tk.tokens(pos, cut), final, rng, alt258=rng.random() < 0.5)
        else:
            _random_dynamic(w, tk.tokens(pos, cut), rng, final)
        pos = cut
        if family == "stored" and not final and rng.random() < 0.5:
            stored_block(w, b"")
    return checked(w.getvalue(), data)


def bgzf_block_maker(seed, families=FAMILIES, log=None):
    """A stand-in for bamio._bgzf_block: block k is encoded by families[k % len(families)] (seeded; zlib-checked like every
    stream of this module).  A stream too long for BSIZE is written again by the next family.  log, a list, gets (family,
    compressed length) per block."""
    rng = random.Random(seed)
    state = {"k": 0}

    def block(data):
        data = bytes(data)
        for attempt in range(len(families) + 1):
            fam = families[(state["k"] + attempt) % len(families)] if attempt < len(families) else "zlib"
            cdata = encode(data, rng, fam) if fam != "zlib" else zlib.compress(data, 6)[2:-4]
            if len(cdata) + 26 <= 65536:
                break
        state["k"] += 1
        if log is not None:
            log.append((fam, len(cdata)))
        return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25)
                + cdata + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))
    return block


# ---- the named families -----------------------------------------------------------------------------------------------------
def _stream(blocks, rng):
    """blocks: (kind, tokens or bytes, options) in order -> (stream, data); the last block is final."""
    w = BitWriter()
    data = bytearray()
    for bi, (kind, what, opt) in enumerate(blocks):
        final = bi == len(blocks) - 1
        if kind == "stored":
            stored_block(w, what, final)
            data += what
        else:
            piece = expand(what, bytes(data))
            if kind == "fixed":
                fixed_block(w, what, final, rng, **opt)
            elif "ll" in opt:
                o = dict(opt)
                dynamic_block(w, what, o.pop("ll"), o.pop("dl"), rng, final=final, **o)
            else:
                _random_dynamic(w, what, rng, final, **opt)
            data += piece
    return checked(w.getvalue(), data), bytes(data)


def _lits(rng, n, alphabet=b"ACGTN\n"):
    return [("L", c) for c in rng.choices(alphabet, k=n)]


def long_codes(rng):
    """(a) Both codes the chain 1, 2 .. 14, 15, 15 or depth-biased random; a literal of 8 - 9 bits (or two of 8 - 15 together),
    then a match whose length symbol has 5 extra bits and whose distance symbol has 13, a few hundred times: every alignment
    of the bit buffer in front of a 48-bit symbol."""
    lit_a, lit_b, lit_c, lit_d = rng.sample(range(256), 4)
    prefix = [("L", rng.choice([lit_a, lit_b, lit_c, lit_d])) for _ in range(300)]
    tokens = list(prefix)
    # 16 500 bytes of matches first, so that distances of 16 385 and more exist
    size = 300
    while size < 16700:
        tokens.append(("M", 258, rng.choice([1, 2, 3, 300])))
        size += 258
    reps = rng.randint(150, 230)
    for _ in range(reps):
        r = rng.random()
        lits = [("L", lit_a)] if r < 0.35 else [("L", lit_b)] if r < 0.6 else [("L", lit_c), ("L", lit_d)] if r < 0.85 else [("L", lit_d), ("L", lit_a)]
        tokens += lits
        size += len(lits)
        if size + 258 > 65536:
            break
        length = rng.randint(131, 258)
        tokens.append(("M", length, rng.randint(16385, min(size, 32768))))
        size += length
    ul, ud = used_symbols(tokens)
    if rng.random() < 0.5:
        # the chain itself: one leaf of every depth, two of 15 - the widest length and distance symbols on those
        pair = rng.choice([(3, 5), (2, 6), (4, 7), (5, 10), (6, 7), (4, 11)])
        pin_ll = {lit_a: 8, lit_b: 9, lit_c: pair[0], lit_d: pair[1], 284: 15, 283: 15, 282: 14, 281: 13, 285: 12}
        ll = assign_lengths(rng, 286, ul, sorted(CHAIN, reverse=True), pin_ll)
        dl = assign_lengths(rng, 30, ud, sorted(CHAIN, reverse=True), {28: 15, 29: 15})
    else:
        pin_ll = {lit_a: 8, lit_b: 9, 281: 15, 282: 15, 283: 15, 284: 15}
        ll = assign_lengths(rng, 286, ul, split_shape(rng, rng.randint(max(len(ul), 20), 286), 15, rng.choice([2.0, 3.0, 8.0])), pin_ll)
        dl = assign_lengths(rng, 30, ud, split_shape(rng, rng.randint(max(len(ud), 16), 30), 15, rng.choice([3.0, 64.0])), {28: 15, 29: 15})
    return _stream([("dynamic", tokens, dict(ll=ll, dl=dl, runs=rng.random() < 0.5, cl_bias=rng.choice([2.0, 64.0]), alt258=True))], rng)


def header_at(k, rng):
    """(b) The widest dynamic header - 286 / 30 symbols, no run symbols, every code length in use written with 7 bits - behind
    a fixed-code block of k literals (an empty stored block in between for every third k)."""
    blocks = [("fixed", _lits(rng, k, bytes(range(144))), {})]           # (8-bit codes: k bytes of stream)
    if k % 3 == 2:
        blocks.append(("stored", b"", {}))
    body = _lits(rng, rng.randint(0, 40)) + [("M", rng.choice([3, 4, 258]), 1)] * (1 if k else 0) + _lits(rng, rng.randint(0, 5))
    ul, ud = used_symbols(body)
    ll = assign_lengths(rng, 286, ul, split_shape(rng, 286, 15, 1.6), None)
    dl = assign_lengths(rng, 30, ud, split_shape(rng, 30, 15, 1.6), None)
    blocks.append(("dynamic", body, dict(ll=ll, dl=dl, runs=False, cl_bias=1e6, wide=True)))
    if k % 5 == 0:
        blocks.append(("fixed", _lits(rng, 3), {}))
    return _stream(blocks, rng)


def match_queue(rng, which):
    """(c) 63 / 64 / 65 matches right in front of an end-of-block and a new header; distance 1 behind a double literal, a match,
    stored bytes; runs of short matches whose sources overlap earlier destinations."""
    lead = _lits(rng, rng.randint(20, 400))
    if which < 3:
        n = (63, 64, 65)[which]
        blocks, size = [], len(lead)
        for rep in range(rng.randint(1, 3)):
            toks = lead if rep == 0 else _lits(rng, rng.randint(0, 3))
            for _ in range(n):
                length = rng.choice([3, 4, 5, 8, 30, 64, 65])
                toks = toks + [("M", length, rng.randint(1, size))]
                size += length
            blocks.append((rng.choice(["dynamic", "fixed"]), toks, {}))
        blocks.append(rng.choice([("dynamic", _lits(rng, 5), {}), ("fixed", _lits(rng, 5), {}), ("stored", b"tail", {})]))
        return _stream(blocks, rng)
    if which == 3:                                         # distance 1 after a double literal, after a match, after stored bytes
        toks = list(lead)
        for _ in range(rng.randint(30, 120)):
            r = rng.random()
            if r < 0.4:
                toks += _lits(rng, 2, b"AC") + [("M", rng.choice([3, 10, 64, 65, 258]), 1)]
            elif r < 0.7:
                toks += [("M", rng.randint(3, 40), rng.randint(2, 20)), ("M", rng.randint(3, 300) % 256 + 3, 1)]
            else:
                toks += _lits(rng, 1) + [("M", rng.randint(3, 258), 1), ("M", rng.randint(3, 258), 1)]
        blocks = [("stored", bytes(rng.randrange(256) for _ in range(rng.randint(1, 50))), {}),
                  (rng.choice(["dynamic", "fixed"]), [("M", rng.choice([3, 258]), 1)] + toks, {}),
                  ("stored", b"xy", {}), ("dynamic", [("M", 7, 1), ("L", 65), ("L", 65), ("M", 9, 1)], {})]
        return _stream(blocks, rng)
    toks, size = list(lead), len(lead)                      # short matches reading what the matches just before them wrote
    for _ in range(rng.randint(100, 400)):
        length = rng.randint(3, 64)
        r = rng.random()
        dist = rng.randint(1, 8) if r < 0.2 else rng.randint(length, length + 70) if r < 0.8 else rng.randint(1, size)
        toks.append(("M", length, min(dist, size)))
        size += length
        if rng.random() < 0.15:
            k = rng.randint(1, 3)
            toks += _lits(rng, k)
            size += k
    return _stream([(rng.choice(["dynamic", "fixed"]), toks, {})], rng)


def stored_forms(rng, which):
    """(d) Length 0 as the first, a middle and the last block; several stored blocks in a row; a stored block behind a Huffman
    block that ends at each of the eight bit offsets; stored bytes as the source of matches."""
    some = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 3000)))
    if which == 0:
        where = rng.randrange(3)
        blocks = [("dynamic", _lits(rng, rng.randint(0, 50)), {}), ("fixed", _lits(rng, rng.randint(1, 50)), {})]
        blocks.insert((0, 1, 2)[where], ("stored", b"", {}))
        if rng.random() < 0.5:
            blocks.insert(rng.randrange(len(blocks) + 1), ("stored", b"", {}))
        return _stream(blocks, rng)
    if which == 1:
        return _stream([("stored", some[i:i + rng.randint(0, 700)], {}) for i in range(0, len(some), 700)] + [("stored", b"", {})] * rng.randint(0, 2), rng)
    if which == 2:
        # fixed codes: 3 header bits, 8-bit literals 0 .. 143, 9-bit literals 144 .. 255, a 7-bit end of block: j nine-bit literals
        # move the end of the block over every offset in a byte
        j = rng.randrange(8)
        toks = _lits(rng, rng.randint(1, 30)) + [("L", rng.randrange(144, 256)) for _ in range(j)]
        return _stream([("fixed", toks, {}), ("stored", some[:rng.randint(0, 40)], {}), ("dynamic", _lits(rng, j) + [("M", 3 + j, 1)], {}),
                        ("stored", some[:j], {})], rng)
    toks, size = [], len(some)
    for _ in range(rng.randint(1, 80)):
        length = rng.randint(3, 258)
        toks.append(("M", length, rng.randint(1, size)))
        size += length
    return _stream([("stored", some, {}), (rng.choice(["dynamic", "fixed"]), toks, {})], rng)


def size_edge(rng, which):
    """(e) Exactly 65 536 bytes: the last token a match of 258 that ends at 65 536; a match that starts at 65 535 - 2."""
    toks = _lits(rng, 300)
    size = 300
    tail = 258 if which == 0 else 3
    while size < 65536 - tail:
        if rng.random() < 0.1:
            toks += _lits(rng, 1)
            size += 1
            continue
        length = min(rng.choice([258, 258, 200, 64, 3]), 65536 - tail - size)
        if length < 3:
            toks += _lits(rng, length)
        else:
            toks.append(("M", length, rng.randint(1, min(size, 32768))))
        size += length
    toks.append(("M", tail, rng.choice([1, 2, 258, 32768])))
    stream, data = _stream([(rng.choice(["dynamic", "fixed"]), toks, dict(alt258=True))], rng)
    assert len(data) == 65536
    return stream, data


def _some_data(rng, n):
    kind = rng.randrange(5)
    if kind == 0:
        return rng.randbytes(n)
    if kind == 1:
        return bytes(rng.choices(b"ACGT", k=n))
    if kind == 2:
        unit = bytes(rng.choice(b"ACGTN") for _ in range(rng.randint(1, 90)))
        return (unit * (n // len(unit) + 1))[:n]
    if kind == 3:
        out = bytearray()
        while len(out) < n:
            out += bytes([rng.randrange(256)]) * rng.randint(1, 600)
        return bytes(out[:n])
    out = bytearray(rng.randrange(256) for _ in range(min(n, 200)))
    while len(out) < n:
        if rng.random() < 0.7:
            a = rng.randrange(len(out))
            out += out[a:a + rng.randint(3, 500)]
        else:
            out += bytes(rng.randrange(17, 60) for _ in range(rng.randint(1, 40)))
    return bytes(out[:n])


def mixed(rng):
    """(f) 1 - 6 blocks of all kinds over data of 0 .. 65 536 bytes (most of them small: the large ones cost the writer time)."""
    r = rng.random()
    n = rng.choice([0, 1, 2, 3, 65536, 65535, 65280]) if r < 0.06 else rng.randint(0, 65536) if r < 0.12 else rng.randint(0, 6000)
    data = _some_data(rng, n)
    return encode(data, rng, rng.choice(["mixed", "mixed", "stored", "match_queue", "headers"])), data


def forms(seed=1, n_long=330, n_mixed=820, header_ks=range(1500)):
    """The families in a fixed order, seeded: yields (family, stream, data).  About 3 000 streams with the defaults."""
    rng = random.Random(seed)
    for _ in range(n_long):
        yield ("long_codes",) + long_codes(rng)
    for k in header_ks:
        yield ("headers",) + header_at(k, rng)
    for i in range(150):
        yield ("match_queue",) + match_queue(rng, i % 5)
    for i in range(160):
        yield ("stored",) + stored_forms(rng, i % 4)
    # the lone one-bit distance code, a block with no distance code, an empty dynamic block whose only code is the end of block
    for i in range(30):
        w = BitWriter()
        toks = _lits(rng, rng.randint(1, 30)) + ([("M", rng.randint(3, 258), 1)] * rng.randint(1, 4) if i % 3 == 0 else [])
        ll, _dl = choose_lengths(toks, rng, "random", pad=0)
        dl = [0] * 30
        if i % 3 == 0:
            dl[0] = 1
        elif i % 3 == 1:
            dynamic_block(w, [], [0] * 256 + [1], [0] * 30, rng, runs=i % 2 == 0)
        dynamic_block(w, toks, ll, dl, rng, final=True, runs=rng.random() < 0.5, wide=i % 2 == 1)
        data = expand(toks)
        yield "headers", checked(w.getvalue(), data), data
    # a run of symbol 16 that goes on from the literal / length lengths into the distance lengths
    for i in range(20):
        toks = _lits(rng, 40) + [("M", 3, 1), ("M", 4, 2)]
        ul, ud = used_symbols(toks)
        sl, sd = split_shape(rng, 286, 15, 1.2), split_shape(rng, 30, 15, 1.2)
        common = [v for v in set(sl) if sl.count(v) >= 3 and sd.count(v) >= 3]
        v = rng.choice(common) if common else None
        ll = assign_lengths(rng, 286, ul + [283, 284, 285], sl, {283: v, 284: v, 285: v} if v else None)
        dl = assign_lengths(rng, 30, ud + [2, 3], sd, {0: v, 1: v, 2: v} if v else None)
        w = BitWriter()
        dynamic_block(w, toks, ll, dl, rng, final=True, runs=True, wide=True)
        data = expand(toks)
        yield "headers", checked(w.getvalue(), data), data
    for i in range(4):
        yield ("size_edge",) + size_edge(rng, i % 2)
    for _ in range(n_mixed):
        s, d = mixed(rng)
        yield "mixed", s, d


_cache = {}


def all_forms(seed=1):
    """forms(seed) as a list, made once a process (the test modules share it)."""
    if seed not in _cache:
        _cache[seed] = list(forms(seed))
    return _cache[seed]


def write_records(path, items):
    """The record file tools/bamdev_emu.cpp reads: per stream u32 number, u32 c_len, u32 u_len, the stream, the expected bytes."""
    with open(path, "wb") as f:
        for k, (_fam, stream, data) in enumerate(items):
            f.write(struct.pack("<III", k, len(stream), len(data)) + stream + data)
