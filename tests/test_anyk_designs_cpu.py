"""The designed pairs of the any-k route (anyk_designs) without a GPU: every design has the property it is named for, every
mutant of the statement is told from the right one by a named design, the distances of the planted keys hold against the
plain dynamic programme, and the restatement equals the C oracle on every k <= 40 design with inversions."""
import numpy as np

import anyk_designs as ad
import anyk_model as model
from conftest import load_golden


def _set(hits):
    return set(map(tuple, hits.tolist()))


def test_sort_sizes():
    ps = {p.name: p for p in ad.sort_sizes()}
    for forward, sizes in ((True, ad.SORT_FWD_N), (False, ad.SORT_INV_N)):
        for n in sizes:
            for k in (3, 33):
                p = ps["%s_n%d_k%d" % ("fwd" if forward else "inv", n, k)]
                assert (p.n, p.forward, p.k) == (n, forward, k) and len(p.hits()) > 0, p.name
    got = {(p.n, p.np) for p in ps.values()}
    # no padding entry, one, and a full array but one; the first array above the tile alone (np = 1024: no global step)
    assert {(512, 512), (1024, 1024), (2048, 2048), (511, 512), (1023, 1024), (2047, 2048), (513, 1024), (1025, 2048), (2049, 4096),
            (4097, 8192), (1, 512), (2, 512), (1026, 2048)} <= got
    for p in ps.values():
        table = model.lookup(p.s1, p.k, not p.forward)
        longest = max(len(v) for v in table.values())
        if p.name.endswith("_k3"):
            # eight 3-mers over two letters (and their eight reverse complements): runs of about n / 8, longer than a tile from 4097
            assert len(table) <= (8 if p.forward else 16) and longest >= p.n // 16, p.name
            assert set(p.allele[j:j + 3] for j in range(p.nk2)) >= set(table), p.name      # every run is emitted
        elif p.k == 33 and p.n >= 511:
            assert longest >= 6 and len(table) > p.n // 2 - 100, p.name                 # planted repeats between unique k-mers
    for name, sign in (("fwd_ascending", 1), ("fwd_descending", -1)):
        p = ps[name]
        keys = [ad.comparator_key(p.s1[i:i + p.k]) for i in range(p.n)]
        assert (p.n, p.np) == (1024, 1024) and all(sign * (a < b) - sign * (a > b) >= 0 for a, b in zip(keys, keys[1:])), name
        assert len(set(keys)) == 10 and set(p.allele[j:j + 3] for j in range(p.nk2)) >= set(model.lookup(p.s1, 3, False))
    big = ps["fwd_n4097_k3"]
    assert max(len(v) for v in model.lookup(big.s1, 3, False).values()) > ad.TILE


def test_every_k():
    ps = ad.every_k()
    base = [p for p in ps if p.off2 == 0]
    assert sorted((p.k, p.forward) for p in base) == sorted((k, f) for k in range(1, 65) for f in (False, True))
    rd, al = base[0].s1, base[0].s2
    assert (len(rd), len(al)) == (400, 500)
    assert any(c.islower() for c in rd) and "NNNNNN" in rd and "R" in rd and ad.revcomp(rd[165:200]) in al and rd[165:200] not in al
    for p in base:
        assert len(p.hits()) > 0, p.name
        if p.forward:          # symbols outside the alphabet on both sides, some matched byte for byte
            assert "XUX" in p.s1 and "XUX" in p.s2 and "Z" in p.s1 and p.s2.endswith("RYU")
        else:
            assert p.refused == 0
    fwd1 = [p for p in base if p.forward and p.k == 3][0]
    assert (fwd1.s2.index("XUX"), fwd1.s1.index("XUX")) in _set(fwd1.hits())
    off = [p for p in ps if p.off2]
    assert {p.off2 for p in off} == {1, 8, 13}                    # odd, a whole word of the 4-bit plane, both
    for o in ad.EVERY_OFF2:
        for forward in (False, True):
            ks = [p.k for p in off if p.off2 == o and p.forward == forward]
            assert {k % 4 for k in ks if k <= 40} == {0, 1, 2, 3} == {k % 4 for k in ks if k > 40}
    for p in off:
        twin = [q for q in base if q.k == p.k and q.forward == p.forward][0]
        assert p.allele == twin.s2 and np.array_equal(p.hits(), twin.hits()) and p.s2[p.off2 - 1:] != twin.s2
    assert {p.flags for p in ps} == {3, 7}


def test_last_symbol():
    ps = ad.last_symbol()
    assert sorted((p.k, p.forward) for p in ps) == sorted((k, f) for k in ad.LAST_K for f in (False, True))
    for p in ps:
        hits = _set(p.hits())
        k = p.k
        for j, i, dot in p.planted:
            a, b = p.s1[i:i + k], p.s2[j:j + k]
            assert ((j, i) in hits) == dot, (p.name, j, i)
            if dot:          # equal, and followed by different symbols (or by the end of both buffers)
                assert a == b and (p.s1[i + k:i + k + 1] != p.s2[j + k:j + k + 1] or i + k == len(p.s1))
            else:            # they differ in symbol k - 1 alone
                assert a[:-1] == b[:-1] and a[-1] != b[-1]
        for dot in (True, False):
            inner = [(j % 4, i % 4) for j, i, d in p.planted if d == dot and i + k < len(p.s1)]
            assert len(set(inner)) == 16, p.name                    # all four byte alignments of both sequences
        assert (len(p.s2) - k, len(p.s1) - k, True) in p.planted     # the last k-mer of each buffer: the word into the padding
        assert any(i + k == len(p.s1) and not d for _j, i, d in p.planted)


def test_edit_rounds():
    ps = {p.name: p for p in ad.edit_rounds()}
    for k in ad.ROUND_K:
        t = k // 10
        for D in ad.ROUND_D:
            p = ps["fwd_k%d_D%d" % (k, D)]
            names, lists, dist = p.keys()
            assert p.D == D == len(names) and p.forward and [len(x) for x in lists] == [2] * 3 + [1] * (D - 3) if D > 3 else p.D == D
            hits = _set(p.hits())
            ranks = set()
            for j, r, e in p.planted:
                q = p.allele[j:j + k]
                assert names[r] == p.s1[r:r + k] and lists[r][0] == r           # rank = order of first insertion
                assert model.lev_dp(q, names[r]) == e == dist[r, j], (p.name, j, r, e)
                assert model.lev_many(q.encode(), model._rows([names[r]], k)).tolist() == [e]
                assert all(((j, i) in hits) == (e <= t) for i in lists[r]), (p.name, j, r, e)
                ranks.add(r)
            assert ranks == {r for r in (0, 63, 64, D - 1) if r < D} and {e for _j, _r, e in p.planted} == {0, t, t + 1}
        # the low-complexity read: one all-A allele k-mer, most lanes of a round, lists of different lengths, the carry into the next round
        p = ps["fwd_k%d_lowcomplexity" % k]
        j = p.info["query"]
        assert p.allele[j:j + k] == "A" * k
        rounds = ad.contributing(p, j)
        assert max(len(r) for r in rounds) >= 32 and sum(1 for r in rounds if r) >= 2, (p.name, [len(r) for r in rounds])
        assert any(len(r) >= 32 and len(set(r)) >= 2 for r in rounds), p.name
        assert any(r and rounds[q + 1] for q, r in enumerate(rounds[:-1]))
        # the same with inversions: a tandem read, every list longer than one
        p = ps["inv_k%d_tandem" % k]
        names, lists, dist = p.keys()
        assert not p.forward and min(len(x) for x in lists) > 1 and len(names) == 46
        rounds = [ad.contributing(p, j)[0] for j in range(p.nk2)]
        assert max(len(r) for r in rounds) >= 2 and len(p.hits()) > 100


def test_edit_split():
    ps = {p.name: p for p in ad.edit_split()}
    for per in ad.SPLIT_PER:
        for tag in ("fwd", "inv"):
            p = ps["%s_per%d" % (tag, per)]
            assert p.k == 50 and p.n in (251, 252) and p.per == per and p.nk2 == 351 and p.n_launches == -(-351 // per) > 1
            js = set(p.hits()[:, 0].tolist())
            assert {per - 1, per, 2 * per - 1, 2 * per} <= js and max(js) >= 300, (p.name, sorted(js))
            assert ad.per_of(p.n) > p.nk2                       # one launch at the default
    p = ps["inv_default_3launches"]
    assert p.edit_pairs is None and (p.n, p.per, p.D, p.n_launches, p.np) == (399902, 5368, 200, 3, 1 << 19)
    js = set(p.hits()[:, 0].tolist())
    assert {p.per - 1, p.per, 2 * p.per - 1, 2 * p.per} <= js and len(p.hits()) > 100000
    assert min(len(x) for x in p.keys()[1]) >= 1999


def test_batch_state():
    ps = ad.batch_state()
    big, small, exact, fwd, none, bad, again = ps
    assert big.k == small.k > 40 and not big.forward and not small.forward and small.n < big.n and small.D < big.D
    assert big.np == 2048 and small.np == 512
    assert exact.k <= 40 and not exact.forward and fwd.forward and fwd.k > 40
    assert none.n == 0 and none.refused == 0 and len(none.hits()) == 0
    assert bad.refused == ad.E_KEYERROR and bad.expected()[0][:3] == [0, -1, -1]
    assert again.k > 40 and not again.forward
    assert all(len(p.hits()) > 0 for p in (big, small, exact, fwd, again))
    assert all(p.D % 64 != 1 for p in (big, small, fwd, again))


# the mutant that only this group tells from the right statement
ONLY = {"sort_sizes": "n1_empty", "every_k": "off2_even", "edit_rounds": "one_lane_round", "edit_split": "restart_j0",
        "batch_state": "stale_isfirst"}


def test_mutants():
    """Every mutant is killed by a named design; every group but last_symbol has a mutant that it alone kills.  last_symbol has
    none and cannot have one beside every_k: a read of 400 symbols against its own allele at k = 1 .. 64 holds k-mers that differ
    in their last symbol alone and equal k-mers followed by different symbols at every k, by volume.  What last_symbol adds is
    that both happen at every k of LAST_K in both modes at all sixteen alignments (test_last_symbol) - so it must kill the two
    comparison mutants on every one of its pairs."""
    table = {m: {g: ad.kills(g, m) for g in ad.GROUPS} for m in ad.MUTANTS}
    for m, row in table.items():
        assert any(row.values()), m
    for g, m in ONLY.items():
        assert [x for x in ad.GROUPS if table[m][x]] == [g], (g, m, table[m])
    assert set(ONLY) | {"last_symbol"} == set(ad.GROUPS)
    for p in ad.last_symbol():
        for m in ("cmp_k_minus_1", "cmp_round_up4"):
            if m == "cmp_round_up4" and p.k % 4 == 0:
                continue
            assert not np.array_equal(ad.mutant_hits(p, m), p.hits()), (p.name, m)


def test_edit_pairs_parameter_is_restated():
    """"anyk_edit_pairs": in the header's list of parameters, in DESIGN.md, and taken (from 1 up) by the CPU twin."""
    import ctypes
    import os
    from conftest import ROOT
    from oracle import oracle as orc
    from vapor_amd import _lib as L
    for name in (os.path.join("include", "vapor_hip.h"), "DESIGN.md", os.path.join("vapor_amd", "csrc", "vapor_hip.hip")):
        with open(os.path.join(ROOT, name)) as f:
            assert '"anyk_edit_pairs"' in f.read(), name
    lib = ctypes.CDLL(orc.build_twin())
    lib.vapor_set_param.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]
    ctx = ctypes.c_void_p()
    assert lib.vapor_init(0, ctypes.byref(ctx)) == 0
    try:
        assert lib.vapor_set_param(ctx, b"anyk_edit_pairs", 1) == 0 and lib.vapor_set_param(ctx, b"anyk_edit_pairs", 1 << 31) == 0
        assert lib.vapor_set_param(ctx, b"anyk_edit_pairs", 0) == L.E_ARG and lib.vapor_set_param(ctx, b"anyk_edit_pairs", -5) == L.E_ARG
    finally:
        lib.vapor_destroy.argtypes = [ctypes.c_void_p]
        lib.vapor_destroy(ctx)


def test_key_major_equals_query_major():
    """lev_matrix row by row is lev_many; kmerhits_array (key-major) is kmerhits (query-major) on designs of every group at k > 40."""
    rng = np.random.default_rng(9)
    for k in (41, 50, 63, 64):
        keys = rng.choice(np.frombuffer(b"ACGTNn", dtype=np.uint8), size=(70, k))
        qs = rng.choice(np.frombuffer(b"ACGTNn", dtype=np.uint8), size=(30, k))
        m = model.lev_matrix(keys, qs)
        assert m.tolist() == [model.lev_many(bytes(r), qs).tolist() for r in keys]
        assert m[:5, :5].tolist() == [[model.lev_dp(bytes(r), bytes(q)) for q in qs[:5]] for r in keys[:5]]
    picks = [ad.edit_rounds()[1], ad.edit_rounds()[-1], ad.edit_rounds()[-4], ad.edit_split()[1], ad.batch_state()[1], ad.every_k()[2 * 40]]
    for p in picks:
        assert p.k > 40
        assert [tuple(h) for h in p.hits().tolist()] == model.kmerhits(p.s1, p.allele, p.k, not p.forward), p.name


def test_model_equals_oracle(oracle):
    """k <= 40 with inversions: the dots are oracle.dotdata_array's, order included, and words 0-9 oracle.pair_stats'."""
    n = 0
    for make in ad.GROUPS.values():
        for p in make():
            if p.k > 40 or p.forward or p.refused:
                continue
            assert np.array_equal(p.hits(), oracle.dotdata_array(p.k, p.s1, p.allele)), p.name
            want = oracle.pair_stats(p.k, p.s1, p.allele)[:10].tolist()
            assert p.expected(3)[0][:10] == want, p.name
            n += 1
    assert n >= 40 + 12 + 8 + 8 + 1


def test_designed_goldens_present():
    """The reference's own answers (tools/gen_anyk_golden.py --designs): every k from 1 to 40 in both modes, the last_symbol
    designs and the eight golden_rounds pairs; test_anyk_cpu.test_model_equals_golden holds the model against each."""
    cases = {c["name"]: c for c in load_golden("kmerhits_anyk.json.gz")["cases"]}
    for k in range(1, 41):
        for tag in ("inv", "fwd"):
            assert "exact_k%d_%s" % (k, tag) in cases
    for p in ad.last_symbol() + ad.golden_rounds():
        c = cases[p.name if p.group == "golden_rounds" else "last_symbol_" + p.name]
        assert (c["s1"], c["s2"], c["k"], c["inversions"]) == (p.s1, p.s2, p.k, not p.forward)
        assert model.matches(c["out"]["ok"], p.hits().tolist()), p.name
    for p in ad.golden_rounds():
        assert max(len(p.s1), len(p.s2)) <= 200 and p.D == (1 if p.forward else 2) * int(p.why.split()[2]), p.name
