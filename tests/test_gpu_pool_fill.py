"""No answer may depend on what a block held before the call got it.

The library recycles device and pinned blocks through a per-context pool (vapor_amd/csrc/vapor_pool.h): a small
call routinely receives a block that a larger call of another entry has just written full, and nothing clears it.  In the other GPU
modules a kernel that reads a word before anything wrote it is right all the same: fresh device memory arrives zeroed, and every
module opens its own engine and runs calls of one family.  Here the engine runs with the test parameter pool_fill: every block the
pool hands out, fresh or recycled, device or pinned, is filled with one byte over its whole capacity before the call goes on, and
so are the staging buffers of the sequence set uploads (tests/test_pool_cpu.py holds the pool to that on the host).  The bodies
are the other modules' own - their check_ functions and the test_ functions that take an engine, called as the plain functions
they are - so every expected value stays the independent model's: each test is the kernel against its model, on dirty blocks.

Two fill bytes.  0xFF is a start value the library itself uses (the wide route's list heads): under it a missing zeroing shows
and a missing 0xFF start does not.  0x5A is neither start value and gives small positive words where 0xFF gives negative ones.
0x00 is what fresh memory holds anyway and is left out.

The last test is the one the fill alone does not give: a large call, then a small call of another entry whose blocks fall into
the pool's window for the large call's blocks, against the same small call on a fresh engine with the parameter off."""
import numpy as np
import pytest

import dot_designs as D
import junction_model as JM
import test_gpu_anyk_designs as TA
import test_gpu_bamdev as TB
import test_gpu_bgzf_fasta as TFA
import test_gpu_dedup as TDD
import test_gpu_depth as TDP
import test_gpu_dot_designs as TD
import test_gpu_finish as TF
import test_gpu_haplotag as TH
import test_gpu_join_designs as TJ
import test_gpu_junction as TGJ
import test_gpu_links as TL
import test_gpu_phase as TPH
import test_gpu_planes as TP
import test_gpu_polish as TGP
import test_gpu_realign as TG
import test_gpu_refine as TR
import test_gpu_revote as TGR
import test_gpu_signature as TS
import test_gpu_support as TSU
import test_gpu_trace as TT
import test_gpu_wide as TW
# the files of the readers' designed regions: the home modules' fixtures, each under a name of its own
from test_gpu_dedup import files as dedup_files                     # noqa: F401
from test_gpu_depth import designed as depth_designed               # noqa: F401
from test_gpu_links import designed as links_designed               # noqa: F401
from test_gpu_signature import designed as signature_designed       # noqa: F401
from test_gpu_support import designed as support_designed           # noqa: F401

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x5A)
FILL_IDS = ["fill_ff", "fill_5a"]


def filled_engine(fill):
    from vapor_amd.engine import Engine
    e = Engine(0)
    e.set_param("pool_fill", fill)
    e.pool_fill = fill
    return e


def unfilled_and_closed(e):
    e.set_param("pool_fill", -1)
    e.close()


@pytest.fixture(scope="module", params=FILLS, ids=FILL_IDS)
def eng(request):
    e = filled_engine(request.param)
    yield e
    unfilled_and_closed(e)


@pytest.fixture(params=FILLS, ids=FILL_IDS)
def own_eng(request):
    """An engine per test, for the bodies whose home module gives them one (tests/test_gpu_join_designs.py: its first plan runs at
    the engine's own join_tasks)."""
    e = filled_engine(request.param)
    yield e
    unfilled_and_closed(e)


@pytest.fixture(params=FILLS, ids=FILL_IDS)
def make_engine(request):
    """A source of filled engines, for the bodies that open and close their own (the budget at its floor against the default)."""
    return lambda: filled_engine(request.param)


def test_the_parameter_takes_a_byte_or_minus_one(eng):
    from vapor_amd import _lib as L
    for bad in (-2, 256, 1 << 40):
        with pytest.raises(L.VaporHipError) as ei:
            eng.set_param("pool_fill", bad)
        assert ei.value.code == L.E_ARG
    # (a refused value leaves the fill as it was: the next body still runs on dirty blocks - the staging test below would tell)


def test_the_fill_is_what_an_unwritten_word_of_a_device_block_holds(eng):
    """vapor_realign_trace copies its run block back whole; a pair's runs are the last n_runs words of its row and what stands in
    front of them is unspecified (include/vapor_hip.h) - no kernel writes it.  Under the parameter it is the fill: the one place
    where a caller sees the bytes of a pool block nothing wrote, and so the sign that the fill is live on the device."""
    ss = eng.seqset(["ACGTACGTAC", "ACGTACGTAC", "ACGTAGGTAC"])
    try:
        head, runs = eng.realign_trace(ss, eng.make_pairs([(0, 1, 0, 0, 0), (0, 2, 0, 0, 0)]), 4, 16)
    finally:
        ss.close()
    assert head[:, 1].tolist() == [0, 0] and head[:, 4].tolist() == [1, 3]
    word = eng.pool_fill * 0x01010101
    assert runs[0, :15].tolist() == [word] * 15 and runs[1, :13].tolist() == [word] * 13
    assert runs[0, 15] == 10 << 2 and runs[1, 13:].tolist() == [5 << 2, 1 << 2 | 1, 4 << 2]


# ---- planes and staging (tests/test_gpu_planes.py against tests/plane_model.py) ---------------------------------------------------
def test_planes_pack_kernel_at_its_edges(eng):
    TP.check_pack_edges(eng)


def test_planes_at_workgroup_boundaries(eng):
    TP.check_workgroup_boundaries(eng)


def test_planes_of_every_creating_entry(eng):
    TP.check_entries(eng)


def test_planes_of_derived_sequences(eng):
    TP.check_derive(eng)


def test_staging_after_a_larger_upload(eng):
    """The staging buffers' case: they are kept by the context and grown, never fresh after the first upload.  A larger upload of
    0xFF-free text first, then the threaded layout whose last sequences are short: the tail bytes of every last 32-byte chunk and
    the chunk map behind the shorter ASCII lie where the larger upload (and the fill) wrote."""
    name = "3 000 of 1 to 4 000"
    lens = TP.staging_layouts()[name]
    big = TP._staging_texts([2 * sum(lens) // 16 + 7] * 16, 4111)
    assert sum(map(TP.n_chunks, big)) > 1.5 * sum((n + 31) // 32 for n in lens)
    TP.check_set(eng, big, None, "the larger upload")
    TP.check_staging(eng, name, threads=(TP.STAGE_THREADS_DEFAULT, 1))


# ---- dot designs (tests/test_gpu_dot_designs.py against dot_designs.expected()) --------------------------------------------------
@pytest.mark.parametrize("band", [0, 1, 2])
def test_dot_designs_small_lists(eng, band):
    TD.check_small_lists(eng, band, n_random=40)


def test_dot_designs_big_lists(eng):
    TD.check_big_lists(eng)


def test_dot_designs_wide_lists(eng):
    TD.check_wide_lists(eng, 0)


def test_dot_designs_sequences_on_the_plan_and_wide_routes(eng):
    TD.check_sequences(eng, wide=True)


@pytest.mark.parametrize("route", [0, 2])
def test_dot_designs_served_group(eng, route):
    TD.check_served_group(eng, route)


# ---- join designs (tests/test_gpu_join_designs.py against join_designs / anyk_model) ----------------------------------------------
def test_join_designs_tiles(own_eng):
    TJ.test_tiles(own_eng)


def test_join_designs_ends(own_eng):
    TJ.test_ends(own_eng)


def test_join_designs_runs(own_eng):
    TJ.test_runs(own_eng)


def test_join_designs_strands(own_eng):
    TJ.test_strands(own_eng)


# ---- any-k designs (tests/test_gpu_anyk_designs.py against anyk_model) ------------------------------------------------------------
def test_anyk_designs_sort_sizes(eng):
    TA.test_sort_sizes(eng)


def test_anyk_designs_last_symbol(eng):
    TA.test_last_symbol(eng)


def test_anyk_designs_edit_rounds(eng):
    TA.test_edit_rounds(eng)


def test_anyk_designs_batch_state(eng):
    TA.test_batch_state(eng)


# ---- finish (tests/test_gpu_finish.py against tests/finish_model.py) ------------------------------------------------------------
def test_finish_gate_tables(eng):
    TF.check_gate_tables(eng)


def test_finish_second_run(eng):
    TF.check_second_run(eng)


def test_finish_async_steps(eng):
    TF.check_async_steps(eng)


# ---- refine (grid_pick_kernel against refine.pick) --------------------------------------------------------------------------------
def test_refine_grid_pick_kernel(eng):
    TR.test_grid_pick_kernel_against_refine_pick(eng)


# ---- wide route (tests/test_gpu_wide.py against the C oracle) ---------------------------------------------------------------------
def test_wide_hits_equal_dotdata(eng, oracle):
    TW.test_hits_equal_dotdata(eng, oracle)


def test_wide_mixed_batch_overflow_then_rerun(eng, oracle):
    """(the rerun takes the first call's blocks back)"""
    TW.test_mixed_batch_overflow_then_rerun(eng, oracle)


# ---- the realign chain (realign, trace, polish, junction and revote kernels against their plain-integer models) ---------------------
def test_realign_designed_pairs(eng):
    TG.test_designed_pairs_equal_the_model(eng)


def test_realign_edge_bands(eng):
    TG.test_bands_on_both_sides_of_every_lane_width_equal_the_model(eng)


def test_trace_designed_pairs(eng):
    TT.test_designed_pairs_equal_the_model_run_for_run(eng)


def test_trace_edge_bands(eng):
    TT.test_bands_on_both_sides_of_every_lane_width_equal_the_model_run_for_run(eng)


def test_trace_budget_at_its_floor(make_engine):
    TT.check_budget_at_its_floor_and_several_groups(make_engine)


def test_polish_designed_loci(eng):
    TGP.test_designed_loci_equal_the_model(eng)


def test_polish_budget_at_its_floor(make_engine):
    TGP.check_budget_at_its_floor(make_engine)


@pytest.mark.parametrize("band", JM.BANDS)
def test_junction_designed_pairs(eng, band):
    TGJ.test_designed_pairs_equal_the_model_at_every_band(eng, band)


def test_junction_edge_bands(eng):
    TGJ.test_bands_on_both_sides_of_every_lane_width_equal_the_model(eng)


def test_junction_tables_beyond_the_budget(make_engine):
    TGJ.check_tables_beyond_the_budget_refuse_the_call(make_engine)


def test_revote_designed_loci(eng):
    TGR.test_designed_loci_equal_the_model(eng)


def test_revote_budget_at_its_floor(make_engine):
    TGR.check_budget_at_its_floor(make_engine)


# ---- the device readers (against the host readers, the Python statements and the closed forms of their home modules) ---------------
def test_readers_bam_chop_on_a_small_world(eng, tmp_path):
    from vapor_amd import synth
    w = synth.make_world(seed=62, n_loci=10, svtypes=("DEL", "INV", "INS", "TANDUP"), span_range=(80, 3000), read_len=7000, n_reads=26)
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    _fa, bam = synth.write_world_files(w, str(tmp_path), block_size=1500)
    regions = [(l.chrom, max(l.start - 400, 1), l.start + 900, 400) for l in w.loci] + [("no_such_contig", 5, 900, 100), (w.loci[0].chrom, 1, 40, 10)]
    status, n = TB.compare(eng, bam, regions)
    assert status.tolist() == [0] * len(regions) and n > 60, (status.tolist(), n)


def test_readers_fasta_windows(eng, tmp_path):
    assert TFA.check_device_windows(eng, tmp_path, 70, 1000, False, 150) >= 150


def test_readers_depth_designed_regions(eng, depth_designed):
    TDP.test_every_designed_region_equals_host_statement_and_model(eng, depth_designed)


def test_readers_signature_designed_regions(eng, signature_designed):
    TS.test_every_designed_region_equals_host_statement_and_model(eng, signature_designed)


def test_readers_links_designed_regions(eng, links_designed):
    TL.test_every_designed_region_equals_host_statement_and_model(eng, links_designed)


def test_readers_support_designed_regions(eng, support_designed):
    TSU.test_every_designed_region_equals_host_statement_and_model(eng, support_designed)


def test_readers_haplotag_hand_written_table(eng, tmp_path):
    TH.test_the_hand_written_table(eng, tmp_path)


def test_readers_haplotag_tile_boundaries(eng, tmp_path):
    TH.test_tile_boundaries_of_operations_and_of_sites(eng, tmp_path)


def test_readers_dedup_designed_regions(eng, dedup_files):
    TDD.test_device_with_the_option_is_the_host_with_it_and_the_device_on_the_file_without_the_dropped_records(eng, dedup_files, "haplotag")


def test_readers_phase_groups_above_the_cap(eng, tmp_path):
    TPH.test_groups_above_the_cap_two_phase_sets_and_a_full_slot(eng, tmp_path)


# ---- big, then small ---------------------------------------------------------------------------------------------------------------------
KiB, MiB = 1 << 10, 1 << 20


def pool_round(n):
    """vapor_pool.h's rounding, restated: 256, powers of two below 64 KiB, 64 KiB steps above."""
    if n <= 256:
        return 256
    if n < 64 * KiB:
        return 1 << (n - 1).bit_length()
    return -(-n // (64 * KiB)) * 64 * KiB


def serves(block, request):
    """A free block of this capacity serves the request: the pool's window."""
    cap = pool_round(request)
    return cap <= block <= 2 * cap + MiB


def wide_join_blocks(k, len1, len2):
    """The capacities of the blocks vapor_wide_batch's join takes for one pair (vapor_dots_plan.h wide_join: keys, bucket heads,
    chain links, counts per allele position and their prefix) - each written over all its bytes by the table and count passes."""
    nk1, nk2 = len1 - k + 1, len2 - k + 1
    ne = 2 * nk1
    buckets = 1 << (2 * ne - 1).bit_length()
    return sorted(pool_round(b) for b in (ne * 4 * ((4 * k + 31) // 32), 4 * buckets, 4 * ne, 4 * nk2, 8 * (nk2 + 1)))


def clean_lists_requests(lists):
    """What vapor_clean_hits asks the pool for (vapor_clean_plan.h ListPack: every list's slot padded to four records): the overflow
    words, the big list, the pairs, the counts, the records, their flag bytes, the statistics."""
    n = len(lists)
    records = max(sum((len(h) + 3) // 4 * 4 for h in lists), 4)
    return [16, 4 * n, 40 * n, 8 * n, 8 * records, records, 128 * n]


def small_lists_answers(e):
    lists = [c.hits for c in D.small_cases(0, 40)]
    return lists, [e.clean_hits(lists, flags=[fl] * len(lists)) for fl in D.FLAG_SETS]


def test_big_then_small_of_another_entry(make_engine):
    """A score_wide pair of 70 kb, then vapor_clean_hits on the small designed lists, on one filled engine: every block the small
    call asks for lies in the pool's window of blocks the large call's join has just written full and given back: the pool hands it
    the smallest free block in that window, one of the large call's whichever it is.  The small call's answers are those of a fresh engine with the parameter off, and the model's."""
    from vapor_amd.engine import Engine
    rng = np.random.default_rng(17)
    al = TW._rand(rng, 70000)
    rd = TW._mutate(rng, al)
    lists = [c.hits for c in D.small_cases(0, 40)]
    # the sizes: each request of the small call finds a block of the large call's join of its own in its window
    free = wide_join_blocks(10, len(rd), len(al))
    assert free == [320 * KiB, 576 * KiB, 576 * KiB, 1152 * KiB, 2 * MiB], free
    requests = clean_lists_requests(lists)
    assert len(requests) == 7 and max(requests) < free[0]
    for r in requests:                                           # (a request of 16 bytes is served by a block of up to 1 MiB + 512)
        assert any(serves(b, r) for b in free), (r, free)
    # ... and the records, the largest request, by all of them but the bucket heads, whose window begins at requests of 512 KiB
    assert [serves(b, max(requests)) for b in free] == [True, True, True, True, False] and serves(free[4], 512 * KiB) and not serves(free[4], 512 * KiB - 64 * KiB)
    clean = Engine(0)
    try:
        _lists, want = small_lists_answers(clean)
    finally:
        clean.close()
    e = make_engine()
    try:
        ss = e.seqset([rd, al])
        try:
            st = e.score_wide(ss, e.make_pairs([(0, 1, 0, 10, 3)]))
        finally:
            ss.close()
        assert st[0, 15] == 0 and st[0, 0] > 60000               # (the large call did its work: a dot per k-mer of the read and more)
        _lists, got = small_lists_answers(e)
        for (st_a, hf_a), (st_b, hf_b) in zip(got, want):
            assert np.array_equal(st_a, st_b)
            assert all(np.array_equal(a, b) for a, b in zip(hf_a, hf_b))
        TD.check_small_lists(e, 0, n_random=40)
    finally:
        unfilled_and_closed(e)
