"""tests/plane_model.py kept honest without a GPU: the vectorised model against its scalar restatement, and the check bodies of
tests/test_gpu_planes.py on the CPU twin (oracle/cpu_twin.cpp, which builds its sequences as texts the way the reference does
and restates the symbol codes) - all but the one that needs a BAM file's bases on the device."""
import ctypes

import numpy as np
import pytest

import plane_model as M
import test_gpu_planes as G


@pytest.fixture(scope="module")
def twin(oracle):
    """vapor_amd._lib bound to the CPU twin for the duration of this module."""
    from vapor_amd import _lib
    so = oracle.build_twin()
    saved = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(so))
    yield so
    _lib._lib = saved


@pytest.fixture()
def eng(twin):
    from vapor_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a[:3], b[:3])) and tuple(a[3:]) == tuple(b[3:])


def test_code_of_every_byte_value():
    every = bytes(range(256))
    for upper in (False, True):
        assert M.codes(every, upper).tolist() == [M.scalar_code(b, upper) for b in range(256)]
    c = M.codes(every).tolist()
    assert [c[ord(ch)] for ch in "ACGTacgt"] == list(range(8))
    assert {c[ord(ch)] for ch in "NRYSWKMBDHV"} == {8} and {c[ord(ch)] for ch in "nryswkmbdhv"} == {9}
    assert c.count(15) == 256 - 8 - 22 and c[0] == 15 and c[ord("X")] == 15 and c[ord("=")] == 15 and c[0xC1] == 15
    u = M.codes(every, True).tolist()
    assert all(u[b] == (c[b - 32] if ord("a") <= b <= ord("z") else c[b]) for b in range(256))
    assert [b for b in range(256) if M.complementary_keeps(b)] == sorted(b"ATGCNatgcn")
    assert M.n_nocomp(every) == M.scalar_n_nocomp(every) == 246


def test_model_equals_its_scalar_restatement():
    rng = np.random.default_rng(4100)
    seqs = [bytes(range(256))]
    for n in (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000):
        seqs += [rng.integers(0, 256, n, dtype=np.uint8).tobytes(), G.draw(rng, n), G.draw(rng, n, b"ACGTacgtNnRyXx-=")]
    for upper in (False, True):
        for s in seqs:
            assert _same(M.planes(s, upper), M.scalar_planes(s, upper)), (len(s), upper)
            assert M.n_nocomp(s) == M.scalar_n_nocomp(s)
    # a set's planes are its sequences' planes, one behind the other
    flags = [t % 3 == 1 for t in range(len(seqs))]
    each = [M.scalar_planes(s, f) for s, f in zip(seqs, flags)]
    p2, e1, x4, n_exc, n_inv = M.set_planes(seqs, flags)
    for w, got in enumerate((p2, e1, x4)):
        assert got.dtype == np.uint32 and np.array_equal(got, np.concatenate([e[w] for e in each]))
    assert n_exc.tolist() == [e[3] for e in each] and n_inv.tolist() == [e[4] for e in each]
    empty = M.set_planes([])
    assert [len(x) for x in empty] == [0] * 5


def test_last_chunk_holds_nothing_behind_the_last_symbol():
    for n in (1, 31, 33):
        p2, e1, x4, n_exc, n_inv = M.planes(b"x" * n)
        assert n_exc == n_inv == n
        assert int(e1[-1]) == (1 << ((n - 1) % 32 + 1)) - 1
        bits = sum(bin(int(v)).count("1") for v in x4)
        assert bits == 4 * n and not p2.any()
    p2, e1, x4, _a, _b = M.planes(b"T" * 17)
    assert p2.tolist() == [0xFFFFFFFF, 3] and e1.tolist() == [0] and x4.tolist() == [0x33333333, 0x33333333, 3, 0]


def test_spelled_texts_and_nibble_texts():
    lits, der = G.derive_case()
    for sg, up in der:
        assert M.spell(lits, sg, up) == M.scalar_spell(lits, sg, up)
    assert M.spell([b"acgtNn"], [(0, 0, 6, True)]) == b"nNacgt"
    assert M.spell([b"ACRGT-a"], [(0, 0, 7, True)]) == b"tACGT"          # complementary() drops what it does not know
    assert M.spell([b"acgtn", b"GG"], [(0, 1, 3, False), (1, 0, 2, True), (0, 0, 0, True)], True) == b"CGTCC"
    rng = np.random.default_rng(4108)
    nib = rng.integers(0, 16, 200)
    for kind, first, n in ((1, 0, 200), (1, 7, 33), (2, 199, 200), (2, 32, 33), (2, 0, 1), (1, 199, 1), (1, 5, 0)):
        assert M.bam_text(nib, first, n, kind) == M.scalar_bam_text(nib, first, n, kind)
    every = np.arange(16)
    assert M.bam_text(every, 0, 16, 1) == b"=ACMGRSVTWYHKDBN"
    assert M.bam_text(every, 15, 16, 2) == b"NVHMDRWABSYCKGT="           # (A <-> T, C <-> G, M <-> K ...: the read backwards)


def test_pack_edges_on_the_twin(eng):
    G.check_pack_edges(eng)
    G.check_workgroup_boundaries(eng)
    G.check_counters_over_many_chunks(eng)


def test_creating_entries_on_the_twin(eng):
    G.check_entries(eng)


def test_large_uploads_on_the_twin(eng):
    """The twin has one way to stage (it ignores stage_threads), so one setting per layout says all it can say here."""
    for name in G.STAGING_LAYOUTS:
        G.check_staging(eng, name, threads=(G.STAGE_THREADS_DEFAULT,))
    G.check_single_thread_staging(eng)


def test_derived_planes_on_the_twin(eng):
    G.check_derive(eng)


def test_n_nocomp_on_the_twin(eng):
    G.check_nocomp(eng)
