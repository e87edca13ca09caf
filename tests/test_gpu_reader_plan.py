"""The host plan of the device readers (vapor_amd/csrc/vapor_readplan.h) on the real entries, on the paths the other reader tests do
not reach: a call with no regions on each of the four vapor_bam_chop_device* entries; regions the host refuses before anything is
sent, among good ones, whose answers must be those of a call with the good ones alone (numbers, groups and the bases themselves);
and one vapor_fasta_windows_device call that holds a reversed window, an empty one and a text buffer one byte short.  The
arithmetic behind these answers is what tests/test_readplan_cpu.py holds to its rules on the host."""
import numpy as np
import pytest

from vapor_amd import _lib as L
from vapor_amd import seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu

MODES = {"plain": {}, "right": {"right": True}, "tagged": {"tagged": True}}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = synth.make_world(seed=17, n_loci=6, read_len=2000, n_reads=8)
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    _fa, bam = synth.write_world_files(w, str(tmp_path_factory.mktemp("readplan")), block_size=1500)
    return w, bam


@pytest.fixture()
def handle(world):
    """(the open file, its native handle): what seqio.chop_many_device hands Engine.bam_chop_device."""
    be = seqio.InProcessBam()
    b = be._open(world[1])
    with b.handle(L.load()) as tl:
        yield b, tl["native"]
    b.close()


def _empty_sites():
    dt = np.dtype([("pos", "<i4"), ("a1", "u1"), ("a2", "u1"), ("idx", "u1"), ("pad", "u1")])
    return np.zeros(1, dtype=np.int32), np.zeros(0, dtype=dt), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int64)


@pytest.mark.parametrize("more", [{}, {"right": True}, {"tagged": True}, {"tagged": True, "sites": _empty_sites()}],
                         ids=["plain", "right", "tagged", "haplotag"])
def test_a_call_with_no_regions(eng, handle, more):
    _b, native = handle
    got = eng.bam_chop_device(native, [], [], [], [], [0], [], 20, **more)
    assert got[0].tolist() == [0]
    assert [len(x) for x in got[1:5]] == [0, 0, 0, 0]
    if "tagged" in more:
        assert [len(x) for x in got[6:]] == [0, 0, 0]
    got[5].close()


def _region_arrays(b, regions):
    """The arrays of seqio.chop_many_device for (chrom, start, end, flank, chunks or None: the index's)."""
    tids, flat, chunk_first = [], [], [0]
    for chrom, start, end, _flank, chunks in regions:
        t = b.tid[chrom]
        tids.append(t)
        for c in (b.index.chunks(t, max(start - 1, 0), end) if chunks is None else chunks):
            flat += [c[0], c[1]]
        chunk_first.append(len(flat) >> 1)
    return (np.asarray(tids, dtype=np.int32), np.asarray([r[1] for r in regions], dtype=np.int64), np.asarray([r[2] for r in regions], dtype=np.int64),
            np.asarray([r[3] for r in regions], dtype=np.int64), np.asarray(chunk_first, dtype=np.int32), np.asarray(flat, dtype=np.uint64))


@pytest.mark.parametrize("mode", list(MODES))
def test_refused_regions_among_good_ones(eng, world, handle, mode):
    w, _bam = world
    b, native = handle
    good = [(l.chrom, max(l.start - 400, 1), l.start + 900, 400, None) for l in w.loci[:3]]
    first = b.index.chunks(b.tid[good[0][0]], good[0][1] - 1, good[0][2])[0]
    refused = [(good[1][0], 5, 2 ** 31, 400, []),                                        # positions are 32-bit in a BAM file
               (good[2][0], good[2][1], good[2][2], 400, [(first[1] + 1, first[1])])]    # a chunk that ends before it starts
    mixed = [good[0], refused[0], good[1], refused[1], good[2]]
    alone = eng.bam_chop_device(native, *_region_arrays(b, good), 20, **MODES[mode])
    both = eng.bam_chop_device(native, *_region_arrays(b, mixed), 20, **MODES[mode])
    try:
        assert alone[4].tolist() == [0, 0, 0] and both[4].tolist() == [0, 2, 0, 2, 0]
        kf_a, kf_b = alone[0].tolist(), both[0].tolist()
        assert kf_b[1] == kf_b[2] and kf_b[3] == kf_b[4]                                 # a refused region has no entries
        assert kf_a[3] > 0
        sel = np.concatenate([np.arange(kf_b[g], kf_b[g + 1]) for g in (0, 2, 4)])
        assert [kf_b[g + 1] - kf_b[g] for g in (0, 2, 4)] == np.diff(kf_a).tolist() and len(sel) == kf_b[5]
        for k in (2, 3) + ((6,) if mode == "tagged" else ()):                            # q0, miss, member
            assert both[k][sel].tolist() == alone[k].tolist(), k
        if mode == "tagged":
            assert both[7][[0, 2, 4]].tolist() == alone[7].tolist() and both[8][[0, 2, 4]].tolist() == alone[8].tolist()
            assert both[7][[1, 3]].tolist() == [-2 ** 63] * 2 and both[8][[1, 3]].tolist() == [0, 0]
        # the bases themselves, as tests/test_gpu_bamdev.py compares them: the bit planes of sets made from the device addresses
        span = np.repeat(np.asarray([r[2] - r[1] for r in good], dtype=np.int64), np.diff(kf_a))
        lens = span - alone[3]
        kind = np.full(len(lens), 2 if mode == "right" else 1, dtype=np.uint8)
        sa = eng.seqset_raw(alone[1], lens, None, src_kind=kind, src_first=alone[2])
        sb = eng.seqset_raw(both[1][sel], lens, None, src_kind=kind, src_first=both[2][sel])
        try:
            for t in range(len(lens)):
                assert all(np.array_equal(x, y) for x, y in zip(sa.planes(t), sb.planes(t))), t
            assert np.array_equal(sa.n_exc, sb.n_exc) and np.array_equal(sa.n_invalid, sb.n_invalid)
        finally:
            sa.close()
            sb.close()
    finally:
        alone[5].close()
        both[5].close()


def test_fasta_reversed_empty_and_one_byte_short(eng, tmp_path):
    rng = np.random.default_rng(5)
    gz = seqio.write_bgzf_fasta(str(tmp_path / "ref.fa.gz"), {"chrA": synth.random_dna(rng, 9000), "chrB": synth.random_dna(rng, 4001)}, 60, 1500)
    bz = seqio.BgzfFasta(gz)
    wins = [("chrA", 100, 2100), ("chrB", 7, 1900), ("chrA", 3000, 8100), ("chrB", 2000, 4001)]
    rng_raw = [bz.raw_range(*x) for x in wins]
    vb = [int(bz.virtual(np.asarray([r[0]]))[0]) for r in rng_raw]
    ve = [int(bz.virtual(np.asarray([r[1]]))[0]) for r in rng_raw]
    # window 0 reversed, window 1 empty, then the four ordinary ones; room for all their raw bytes but one
    vbeg = [ve[0], vb[1]] + vb
    vend = [vb[0], vb[1]] + ve
    texts, _traits, status = eng.fasta_windows_device(bz._fd, vbeg, vend, sum(r[1] - r[0] for r in rng_raw) - 1)
    assert status.tolist() == [L.FASTA_RANGE, 0, 0, 0, 0, L.FASTA_ROOM]
    assert texts[0] is None and texts[1] == "" and texts[5] is None
    for q in range(3):
        assert texts[2 + q] == bz.fetch(*wins[q]), wins[q]
