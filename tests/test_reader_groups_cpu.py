"""The scheduler of the device readers' calls (vapor_amd/seqio.py: _flat_chunks, _size_groups, _run_groups - what
InProcessBam.chop_many_device and ._evidence_many share) on made-up chunk lists, without a library: the arrays of a call, the
groups at the cap's edges, and the order of the calls under a pattern of refusals.  A region's size is stated here as the rule
has it: (end >> 16) - (begin >> 16) + 65600 compressed bytes a chunk."""
import numpy as np
import pytest

from vapor_amd import _lib, seqio

MB = 1 << 20
LAST = 65600                    # what a chunk counts beside its file range: a last block


def region(*sizes):
    """A region whose chunks count `sizes` bytes each, one behind the other in the file (within-block offsets that do not count)."""
    out, at = [], 1000
    for k, s in enumerate(sizes):
        out.append(((at << 16) | (17 * k), ((at + s - LAST) << 16) | 4321))
        at += s
    return out


def groups_of(regions, cap_mb, monkeypatch):
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", str(cap_mb))
    return seqio._size_groups(*seqio._flat_chunks(regions))


def test_the_arrays_of_a_call():
    lists = [[(5 << 16, 9 << 16 | 3)], [], [(1 << 40, 1 << 41), (7, 8)], ()]
    chunk_first, flat_a = seqio._flat_chunks(lists)
    assert chunk_first.dtype == np.int32 and chunk_first.tolist() == [0, 1, 1, 3, 3]         # a region without chunks: an empty range
    assert flat_a.dtype == np.uint64 and flat_a.shape == (3, 2)
    assert flat_a.tolist() == [[5 << 16, 9 << 16 | 3], [1 << 40, 1 << 41], [7, 8]]
    chunk_first, flat_a = seqio._flat_chunks([])
    assert chunk_first.dtype == np.int32 and chunk_first.tolist() == [0]
    assert flat_a.dtype == np.uint64 and flat_a.shape == (0, 2)
    assert seqio._size_groups(chunk_first, flat_a) == []
    chunk_first, flat_a = seqio._flat_chunks([[], []])                                        # regions, and not one chunk
    assert chunk_first.tolist() == [0, 0, 0] and flat_a.shape == (0, 2)
    assert seqio._size_groups(chunk_first, flat_a) == [(0, 2)]


def test_groups_at_the_edges_of_the_cap(monkeypatch):
    half = MB // 2
    # cap 0: every region with a chunk is alone
    assert groups_of([region(LAST), region(LAST, 3 * MB), region(LAST + 1)], 0, monkeypatch) == [(0, 1), (1, 2), (2, 3)]
    # a cap that admits exactly two: two halves of it are a group, the third region opens the next
    assert groups_of([region(half)] * 5, 1, monkeypatch) == [(0, 2), (2, 4), (4, 5)]
    assert groups_of([region(half // 2, half // 2)] * 5, 1, monkeypatch) == [(0, 2), (2, 4), (4, 5)]       # (the chunks of a region add up)
    # one byte more in the second, and it no longer fits
    assert groups_of([region(half), region(half + 1), region(half - 1), region(half)], 1, monkeypatch) == [(0, 1), (1, 3), (3, 4)]
    # a first region that alone is over the cap is still taken, alone
    assert groups_of([region(3 * MB), region(LAST), region(LAST)], 1, monkeypatch) == [(0, 1), (1, 3)]
    assert groups_of([region(LAST), region(3 * MB), region(LAST)], 1, monkeypatch) == [(0, 1), (1, 2), (2, 3)]
    # a region without chunks counts nothing: it goes with the group before it where that is within the cap, and only there
    assert groups_of([region(MB), [], [], region(LAST)], 1, monkeypatch) == [(0, 3), (3, 4)]
    assert groups_of([region(MB + 1), [], region(LAST)], 1, monkeypatch) == [(0, 1), (1, 3)]
    assert groups_of([[], region(LAST), []], 0, monkeypatch) == [(0, 1), (1, 2), (2, 3)]


def test_the_cap_is_read_at_the_call_and_is_192_mb_without_the_variable(monkeypatch):
    regions = [region(96 * MB), region(96 * MB), region(96 * MB), region(96 * MB + 1), region(96 * MB)]
    arrays = seqio._flat_chunks(regions)
    monkeypatch.delenv("VAPOR_BAM_DEVICE_BATCH_MB", raising=False)
    assert seqio._size_groups(*arrays) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "1000")
    assert seqio._size_groups(*arrays) == [(0, 5)]
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "95")
    assert seqio._size_groups(*arrays) == [(k, k + 1) for k in range(5)]


def too_big(what="vapor_bam_depth_device: more than 1.5 GB of blocks in one call (use smaller batches)"):
    return _lib.VaporHipError(_lib.E_ARG, what)


def test_the_order_of_the_calls_under_refusals():
    calls = []

    def call(a, e):
        calls.append((a, e))
        if e - a > 2 or a <= 7 < e:                # more than two regions; and whatever holds region 7, down to itself
            raise too_big()
        return "r%d-%d" % (a, e)
    groups = [(0, 5), (5, 6), (6, 9)]
    got = list(seqio._run_groups(groups, call))
    # a refused group's halves come next, cut at (a + e) // 2, before the groups behind it
    assert calls == [(0, 5), (0, 2), (2, 5), (2, 3), (3, 5), (5, 6), (6, 9), (6, 7), (7, 9), (7, 8), (8, 9)]
    # what went through in order, a single refused region - in the middle of the others - as None: the host route's
    assert got == [(0, 2, "r0-2"), (2, 3, "r2-3"), (3, 5, "r3-5"), (5, 6, "r5-6"), (6, 7, "r6-7"), (7, 8, None), (8, 9, "r8-9")]
    assert groups == [(0, 5), (5, 6), (6, 9)]                  # (the caller's list is left as it was)
    assert list(seqio._run_groups([], call)) == []
    # the calls are made as the answers are taken: nothing runs ahead of its consumer
    calls.clear()
    it = seqio._run_groups([(0, 2), (2, 4)], call)
    assert next(it) == (0, 2, "r0-2") and calls == [(0, 2)]
    assert next(it) == (2, 4, "r2-4") and calls == [(0, 2), (2, 4)]


@pytest.mark.parametrize("err", [ValueError("a damaged file"), MemoryError(), KeyboardInterrupt(),
                                 _lib.VaporHipError(_lib.E_ARG, "vapor_bam_depth_device: bad argument")])
def test_another_error_passes_through_untouched(err):
    calls = []

    def call(a, e):
        calls.append((a, e))
        if len(calls) == 2:
            raise err
        return a
    got = []
    with pytest.raises(type(err)) as info:
        for item in seqio._run_groups([(0, 3), (3, 6), (6, 7)], call):
            got.append(item)
    assert info.value is err
    assert got == [(0, 3, 0)] and calls == [(0, 3), (3, 6)]        # no halves, no further call
