"""Breakpoint refinement (`--refine M[:T]`, vapor_amd/refine.py, drivers.vapor_refine) without a GPU: the candidate model, the
pick rule, the identity at M = 0 on the committed bed worlds, the recovery of moved breakpoints, the CLI's columns and INFO
keys.  Everything here runs the brute-force route (one Score request per candidate, host finish, pick in Python) on the
tests' stand-in engine or on the CPU twin of the C ABI, which has no refinement kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from fake_engine import FakeEngine

from vapor_amd import cli, drivers, modes, pipeline, refine, seqio, synth
from vapor_amd import _lib as L


@pytest.fixture()
def fake(oracle):
    e = FakeEngine(oracle)
    pipeline.set_engine(e)
    yield e
    pipeline.set_engine(None)
    seqio.set_backend(None)


@pytest.fixture()
def twin_eng(oracle):
    """The real Engine on the CPU twin of the C ABI (test infrastructure), as pipeline's engine."""
    from vapor_amd.engine import Engine
    saved = L._lib
    L._lib = L.bind(ctypes.CDLL(oracle.build_twin()))
    e = Engine(0)
    pipeline.set_engine(e)
    yield e
    pipeline.set_engine(None)
    seqio.set_backend(None)
    e.close()
    L._lib = saved


# ------------------------------------------------------------------------------------------
# enumeration
# ------------------------------------------------------------------------------------------

def test_counts_default_step_and_cap():
    assert refine.MAX_CANDIDATES == L.MAX_CANDIDATES == 128
    for spec, n in (("0", 1), ("10:10", 9), ("20:10", 25), ("50", 121)):
        m, t = refine.parse(spec)
        assert len(refine.candidates(m, t, 1000, 2000)) == n, spec
    assert refine.parse("50") == (50, 10) and refine.parse("0") == (0, 1) and refine.parse("5") == (5, 1)
    assert refine.parse("50:25") == (50, 25) and refine.parse("50:9") == (50, 9)          # (an explicit step: the cap alone)
    for m in range(0, 200):
        t = refine.default_step(m)
        assert (2 * (m // t) + 1) ** 2 <= 128 and len(refine.candidates(m, t, 1000, 5000)) <= 128
        assert t == 1 or (2 * -(-m // (t - 1)) + 1) ** 2 > 128
    for bad in ("50:8", "6:1", "200:10"):
        with pytest.raises(ValueError, match="at most 128"):
            refine.parse(bad)
    for bad in ("-1", "10:0", "x", "10:5:2", "", "1.5"):
        with pytest.raises(ValueError):
            refine.parse(bad)


def test_order_of_the_candidates():
    c = refine.candidates(20, 10, 1000, 2000)
    assert c[0] == (0, 0) and len(set(c)) == 25
    assert c[:5] == [(0, 0), (0, -10), (0, 10), (-10, 0), (10, 0)]
    keys = [(abs(ds) + abs(de), abs(ds), ds, de) for ds, de in c]
    assert keys == sorted(keys)
    assert set(c) == {(ds, de) for ds in (-20, -10, 0, 10, 20) for de in (-20, -10, 0, 10, 20)}


def test_cipos_and_ciend_clip_the_grid_and_zero_stays():
    c = refine.candidates(50, 10, 1000, 2000, cipos=(-20, 10), ciend=(0, 35))
    assert {ds for ds, _ in c} == {-20, -10, 0, 10} and {de for _, de in c} == {0, 10, 20, 30} and c[0] == (0, 0)
    # bounds that exclude 0, or the whole margin: 0 is kept
    c = refine.candidates(50, 10, 1000, 2000, cipos=(15, 45), ciend=(-400, -300))
    assert {ds for ds, _ in c} == {0, 20, 30, 40} and {de for _, de in c} == {0}
    # wider than the margin: the margin holds
    assert len(refine.candidates(10, 10, 1000, 2000, cipos=(-500, 500), ciend=(-500, 500))) == 9


def test_candidates_that_leave_no_span_are_dropped():
    c = refine.candidates(20, 10, 1000, 1015)                # b - a = 15 + de - ds
    assert (0, 0) in c and all(15 + de - ds >= 1 for ds, de in c)
    assert (10, -10) not in c and (20, 0) not in c and (10, 0) in c and len(c) < 25


# ------------------------------------------------------------------------------------------
# the pick rule
# ------------------------------------------------------------------------------------------

def _row(qs, gs, n, npos=None):
    return [qs, gs, 1.0, 3.0, n, n if npos is None else npos, 0.0, 0.0]


NA = [np.nan, np.nan, np.nan, np.nan, 0.0, np.nan, np.nan, np.nan]


def test_pick_rule_on_hand_made_tables():
    # the largest GS
    assert refine.pick([_row(.5, .5, 10), _row(.4, .8, 10), _row(.9, .7, 10)]) == 1
    # GS ties broken by QS
    assert refine.pick([_row(.5, .8, 10), _row(.4, .8, 10), _row(.9, .8, 10), _row(.7, .8, 10)]) == 2
    # full ties broken by index (candidate 0 keeps a full tie)
    assert refine.pick([_row(.5, .8, 10), _row(.5, .8, 10), _row(.5, .8, 10)]) == 0
    assert refine.pick([_row(.5, .7, 10), _row(.5, .8, 10), _row(.5, .8, 10)]) == 1
    # fewer scored reads than candidate 0: loses despite a higher GS; more reads are fine
    assert refine.pick([_row(.5, .5, 10), _row(.9, 1.0, 9), _row(.5, .6, 10), _row(.5, .55, 12)]) == 2
    # candidate 0 without a scored read: anything that scored one is eligible
    assert refine.pick([NA, _row(.1, .1, 1), _row(.1, .2, 2)]) == 2
    # an all-NA locus
    assert refine.pick([NA, NA, NA]) == 0 and refine.pick([NA]) == 0
    # a candidate that scored nothing never wins
    assert refine.pick([_row(.0, .0, 10, 0), NA, _row(0., 0., 10, 0)]) == 0


def test_pick_rule_nan_handling_is_finish_pys():
    """vapor_amd.finish tests numbers with `>` and `>=`, which a NaN never passes (rounded_nonpositive, locus_summary): here a
    NaN GS or QS never beats a number, a NaN read count makes a candidate ineligible, and -0.0 ties with 0.0."""
    nan = np.nan
    assert refine.pick([_row(.5, .5, 10), _row(.9, nan, 10), _row(nan, .5, 10)]) == 0
    assert refine.pick([_row(nan, .5, 10), _row(.1, .5, 10)]) == 1
    assert refine.pick([_row(.5, nan, 10), _row(.1, -1.0, 10)]) == 1
    assert refine.pick([_row(.5, .5, 10), _row(.9, .9, nan)]) == 0
    assert refine.pick([_row(.5, .5, nan), _row(.9, .9, 10)]) == 0              # (nothing is >= NaN: no candidate is eligible)
    assert refine.pick([_row(0.0, .5, 10), _row(-0.0, .5, 10)]) == 0 and refine.pick([_row(-0.0, .5, 10), _row(0.0, .5, 10)]) == 0
    from vapor_amd import finish
    assert bool(finish.rounded_nonpositive(np.asarray([nan]))[0])


def test_record_is_the_finish_of_the_scores():
    from vapor_amd import finish
    rng = np.random.default_rng(5)
    assert np.array_equal(refine.record([]), np.asarray(NA), equal_nan=True) and refine.record([None, None])[4] == 0
    for n in (1, 3, 8, 20, 40):
        sc = [None if rng.random() < .2 else float(rng.normal(.3, .5)) for _ in range(n)]
        kept = [x for x in sc if x is not None]
        rec = refine.record(sc)
        if not kept:
            assert rec[4] == 0
            continue
        qs, gs, idx, gq = finish.locus_summary(kept)
        assert rec[:4].tolist() == [float(qs), gs, float(idx), gq] and rec[4] == len(kept)
        assert rec[5] == sum(1 for x in kept if x > 0) and rec[6] == sum(1 for x in kept if not round(x, 2) > 0)


# ------------------------------------------------------------------------------------------
# identity at M = 0 on the committed bed worlds
# ------------------------------------------------------------------------------------------
LOCUS = load_golden("locus_bed.json.gz")["cases"] + load_golden("locus_long.json.gz")["cases"]
_SHORT_KIND = {"DEL": "del", "INV": "s1", "TANDUP": "s3"}


def _scored_on_the_short_branch(job) -> bool:
    """Whether the type's own driver scores this locus on its short branch: it sends the Score request of that branch (a DEL
    below 10 kb: 'del'; INV: 's1', its junction branch sends 's2'; TANDUP: 's3', its junction branch 's2')."""
    name = job.key.split(":")[-1]
    c, s, e = job.key.split(":")[0], int(job.key.split(":")[1]), int(job.key.split(":")[2])
    if name not in _SHORT_KIND or e - s >= drivers.default_max_sv_test or s - seqio.flank_length_calculate([c, s, e]) < 1:
        return False
    seen = []
    gen = job.make()
    eng = pipeline.get_engine()
    try:
        req = next(gen)
        while True:
            if isinstance(req, drivers.Score):
                seen.append(req.kind)
            ans = pipeline._answer(eng, [req], None)[0]
            req = gen.throw(ans) if isinstance(ans, BaseException) else gen.send(ans)
    except StopIteration:
        pass
    return _SHORT_KIND[name] in seen


@pytest.mark.parametrize("case", LOCUS, ids=lambda c: c["name"])
def test_refine_0_is_the_unrefined_row_and_its_own_numbers(fake, case, tmp_path):
    world = synth.world_from_json(case["world"])
    seqio.set_backend(seqio.MemorySamtools(world))
    bed = tmp_path / "in.bed"
    bed.write_text(case["bed"])
    tables = {}
    for name, more in (("plain", []), ("refined", ["--refine", "0"])):
        out = tmp_path / (name + ".vapor")
        assert cli.main(["bed", "--sv-input", str(bed), "--reference", "ref.fa", "--pacbio-input", "x.bam", "--output-path",
                         str(tmp_path / "figs"), "--output-file", str(out), "--no-figures"] + more) == 0
        tables[name] = out.read_text().splitlines()
    plain, refined = tables["plain"], tables["refined"]
    assert len(plain) == len(refined) and refined[0] == plain[0] + "\tVaPoR_RPOS\tVaPoR_REND\tVaPoR_QS0\tVaPoR_GS0"
    jobs = cli.bed_jobs(cli.bed_info_readin(str(bed), str(tmp_path / "figs")), 3, "x.bam", "ref.fa", str(tmp_path / "figs") + "/", "in")
    assert len(jobs) == len(plain) - 1
    n_refined = 0
    for job, a, b in zip(jobs, plain[1:], refined[1:]):
        f = a.split("\t")
        if _scored_on_the_short_branch(job):
            assert b == a + "\t" + "\t".join([f[1], f[2], f[5], f[6]]), job.key
            n_refined += 1
        else:
            assert b == a + "\t.\t.\t.\t.", job.key
    if case["name"] == "bed_hom_alt":
        assert n_refined >= 3                 # (the comparison above is not made of fall-backs alone)


def test_without_the_option_the_jobs_are_todays(fake, tmp_path):
    """No --refine: the jobs keep their array-route description (fastpath) and the drivers' own generators."""
    case = LOCUS[0]
    bed = tmp_path / "in.bed"
    bed.write_text(case["bed"])
    info = cli.bed_info_readin(str(bed), str(tmp_path / "figs"))
    plain = cli.bed_jobs(info, 3, "x.bam", "ref.fa", "o/", "in")
    ref = cli.bed_jobs(info, 3, "x.bam", "ref.fa", "o/", "in", modes.refine(50, 10))
    assert [j.key for j in plain] == [j.key for j in ref]
    for a, b in zip(plain, ref):
        name = a.key.split(":")[-1]
        assert a.spec is not None and a.extra is None
        if name in _SHORT_KIND:
            assert b.spec is None and b.cost > a.cost           # fastpath leaves it alone; its cost counts the candidates
        else:
            assert b.spec == a.spec and b.cost == a.cost
    assert cli.job_cost("DEL", 800, candidates=121) > 20 * cli.job_cost("DEL", 800) - 20 * cli.COST_HOST_US - 20 * cli.COST_PER_KBASE_US * 30
    assert cli.job_cost("INV", 800, candidates=1) == cli.job_cost("INV", 800)


# ------------------------------------------------------------------------------------------
# recovery of moved breakpoints
# ------------------------------------------------------------------------------------------
MOVES = [(30, -20), (-20, 30), (40, 0), (-30, -30), (0, 20), (20, 20)]


def _recovery_world():
    return synth.make_world(seed=11, n_loci=6, svtypes=("DEL", "INV", "TANDUP"), spans=[400, 600, 500, 900, 700, 300], read_len=3200,
                            n_reads=10, alt_fraction=1.0, errors=(0.0, 0.0, 0.0))


def test_moved_breakpoints_are_recovered(twin_eng, tmp_path):
    """A world of two DEL, two INV and two TANDUP loci whose BED rows are moved off the implanted breakpoints by multiples of
    the step (10) within the margin (50): `vapor bed --refine 50`, brute-force route on the CPU twin.  On every locus the
    winner is no further from the truth (|a - s*| + |b - e*|) than the call, on at least one locus per type strictly closer,
    and every locus is refined.

    The reads are error-free and all carry the alt allele.  With the generator's default error rates (1 % substitutions, 8 %
    insertions, 4 % deletions) the same world does not meet this: every candidate near the truth has GS = 1, the choice falls
    to QS, and the reads' own indels move a scorer's distance sums by more than a 10 bp step does - three of the six winners
    then lie further from the truth than the call (measured on this world: DEL (+30, -20) -> (+50, -20), TANDUP (+40, 0) ->
    (+30, +20), INV (0, +20) -> (+10, +20)).  Error-free, the two deletions behave differently from the other types: a
    deletion allele shifted by the same amount at both ends is nearly the same sequence, so DEL (+30, -20) keeps its call
    (tie, lowest index), while DEL (-30, -30) moves its start home."""
    w = _recovery_world()
    seqio.set_backend(seqio.MemorySamtools(w))
    rows = []
    for l, (ms, me) in zip(w.loci, MOVES):
        rows.append("\t".join([l.chrom, str(l.start + ms), str(l.end + me), l.svid, {"TANDUP": "DUP"}.get(l.svtype, l.svtype)]))
    bed = tmp_path / "moved.bed"
    bed.write_text("\n".join(rows) + "\n")
    out = tmp_path / "out.vapor"
    assert cli.main(["bed", "--sv-input", str(bed), "--reference", "ref.fa", "--pacbio-input", "x.bam", "--output-path",
                     str(tmp_path / "figs"), "--output-file", str(out), "--no-figures", "--refine", "50"]) == 0
    got = [ln.split("\t") for ln in out.read_text().splitlines()[1:]]
    assert len(got) == len(w.loci)
    closer = {}
    for l, (ms, me), f in zip(w.loci, MOVES, got):
        assert f[0] == l.chrom and int(f[1]) == l.start + ms and int(f[2]) == l.end + me and f[3] == l.svtype     # POS / END: the call
        assert "." not in f[-4:], (l.svid, f[-4:])                                                       # no locus is left out
        a, b = int(f[-4]), int(f[-3])
        assert (a - int(f[1])) % 10 == 0 and (b - int(f[2])) % 10 == 0 and abs(a - int(f[1])) <= 50 and abs(b - int(f[2])) <= 50
        d_call, d_win = abs(ms) + abs(me), abs(a - l.start) + abs(b - l.end)
        print(l.svtype, "call off by", (ms, me), "winner off by", (a - l.start, b - l.end), "GS", f[6], "GS0", f[-1])
        assert d_win <= d_call, (l.svid, l.svtype, d_call, d_win)
        closer[l.svtype] = closer.get(l.svtype, False) or d_win < d_call
        assert float(f[6]) >= float(f[-1])                       # the winner's GS is at least candidate 0's
    assert closer == {"DEL": True, "INV": True, "TANDUP": True}
    # the longer rows go through concat, sort, bgzip and tabix
    from vapor_amd import workflow
    gz = workflow.merge_tables([str(out)], str(tmp_path / "merged"))
    rows_back = workflow.read_bgzf(gz).decode().splitlines()
    assert sorted(rows_back) == sorted(out.read_text().splitlines()[1:]) and all(len(r.split("\t")) == 14 for r in rows_back)
    l0 = w.loci[0]
    hit = workflow.tabix_query(gz, l0.chrom, l0.start, l0.end)
    assert len(hit) == 1 and hit[0].split("\t")[-4:] == got[0][-4:]


def test_grid_result_is_the_candidates_own_requests(twin_eng):
    """The brute-force route per candidate is pipeline.score_requests' answer for that allele, its record the host finish of
    those scores, the winner refine.pick's; the driver at M = 0 sends the allele of the type's own driver."""
    w = synth.make_world(seed=3, n_loci=3, svtypes=("DEL", "INV", "TANDUP"), spans=[300, 420, 350], read_len=2400, n_reads=7)
    seqio.set_backend(seqio.MemorySamtools(w))
    for l in w.loci:
        info = [l.chrom, l.start, l.end]
        own = {"DEL": drivers.vapor_simple_del, "INV": drivers.vapor_simple_inv, "TANDUP": drivers.vapor_simple_tandup}[l.svtype]
        base_reqs = []
        g = own(3, 1, "x.bam", "ref.fa", list(info), "f.png")
        req = next(g)
        try:
            while True:
                if isinstance(req, drivers.Score):
                    base_reqs.append(req)
                req = g.send(pipeline._answer(twin_eng, [req], None)[0])
        except StopIteration as e:
            base_scores = e.value
        g = drivers.vapor_refine(l.svtype, 3, 1, "x.bam", "ref.fa", list(info), "f.png", 0, 1)
        req = next(g)
        grids = []
        try:
            while True:
                if isinstance(req, drivers.ScoreGrid):
                    grids.append(req)
                req = g.send(pipeline._answer(twin_eng, [req], None)[0])
        except StopIteration as e:
            scores = e.value
        assert len(grids) == 1 and len(grids[0].alts) == 1 and len(base_reqs) == 1
        assert str(grids[0].alts[0]) == str(base_reqs[0].alt_seq) and grids[0].alts[0].segs == base_reqs[0].alt_seq.segs
        assert grids[0].ref_seq == base_reqs[0].ref_seq and grids[0].kind == base_reqs[0].kind and grids[0].k == base_reqs[0].k
        assert list(scores) == list(base_scores) and scores.info[:2] == (float(l.start), float(l.end))
        # a grid of 9 on the same locus
        g9 = drivers.ScoreGrid(grids[0].kind, grids[0].ref_seq,
                               [drivers.refine_allele(l.svtype, grids[0].ref_seq, seqio.flank_length_calculate(info), 0, ds, de)
                                for ds, de in refine.candidates(10, 10, l.start, l.end)], grids[0].reads, grids[0].k)
        res = pipeline.score_grids(twin_eng, [g9])[0]
        each = pipeline.score_requests(twin_eng, [drivers.Score(g9.kind, g9.ref_seq, a, g9.reads, g9.k) for a in g9.alts])
        assert res.all_scores == each and res.winner == refine.pick(res.all_recs) and res.scores == each[res.winner]
        assert np.array_equal(res.all_recs, np.stack([refine.record(v) for v in each]), equal_nan=True)
        assert np.array_equal(res.rec0, res.all_recs[0], equal_nan=True) and np.array_equal(res.rec, res.all_recs[res.winner], equal_nan=True)


# ------------------------------------------------------------------------------------------
# vapor vcf --refine: CIPOS / CIEND, INFO keys, header lines
# ------------------------------------------------------------------------------------------

def test_vcf_refine_info_keys_and_ci_bounds(twin_eng, tmp_path):
    w = synth.make_world(seed=21, n_loci=4, svtypes=("DEL", "INV", "INS", "DEL"), spans=[400, 500, 1, 30], read_len=2600, n_reads=8,
                         alt_fraction=1.0, errors=(0.0, 0.0, 0.0))
    seqio.set_backend(seqio.MemorySamtools(w))
    moves = {0: (-20, 0), 1: (0, 20)}
    ci = {0: "CIPOS=0,30;CIEND=-10,10", 1: "CIPOS=0,0;CIEND=-40,0"}
    lines = synth.vcf_text(w).splitlines()
    body = [ln for ln in lines if not ln.startswith("#")]
    for t, (ms, me) in moves.items():
        l = w.loci[t]
        f = body[t].split("\t")
        f[1] = str(l.start + ms)
        f[7] = "SVTYPE=%s;END=%d;IMPRECISE;%s" % (l.svtype, l.end + me, ci[t])
        body[t] = "\t".join(f)
    vcf = tmp_path / "calls.vcf"
    vcf.write_text("\n".join([ln for ln in lines if ln.startswith("#")] + body) + "\n")
    got_ci = cli.vcf_ci_readin(str(vcf))
    l0, l1 = w.loci[0], w.loci[1]
    assert got_ci["%s:%d:%d:DEL" % (l0.chrom, l0.start - 20, l0.end)] == ((0, 30), (-10, 10))
    assert got_ci["%s:%d:%d:INV" % (l1.chrom, l1.start, l1.end + 20)] == ((0, 0), (-40, 0))
    args = ["vcf", "--sv-input", str(vcf), "--reference", "ref.fa", "--pacbio-input", "x.bam", "--output-path", str(tmp_path / "figs"),
            "--output-file", str(tmp_path / "unused"), "--no-figures"]
    assert cli.main(args) == 0
    plain = (tmp_path / "calls.vcf.vapor").read_text().splitlines()
    assert cli.main(args + ["--refine", "50"]) == 0
    ref = (tmp_path / "calls.vcf.vapor").read_text().splitlines()
    new_meta = [ln for ln in ref if ln.startswith("##") and ln not in plain]
    assert [re.match(r"##INFO=<ID=(\w+),", ln).group(1) for ln in new_meta] == ["VaPoR_RPOS", "VaPoR_REND", "VaPoR_QS0", "VaPoR_GS0"]
    assert [ln for ln in plain if ln.startswith("#")] == [ln for ln in ref if ln.startswith("#") and ln not in new_meta]
    recs_p = [ln.split("\t") for ln in plain if not ln.startswith("#")]
    recs_r = [ln.split("\t") for ln in ref if not ln.startswith("#")]
    assert len(recs_p) == len(recs_r) == 4
    for t, (p, r) in enumerate(zip(recs_p, recs_r)):
        assert p[:7] == r[:7] and p[8:] == r[8:]
        keys_p = [x.split("=")[0] for x in p[7].split(";")]
        keys_r = [x.split("=")[0] for x in r[7].split(";")]
        assert keys_r == keys_p + ["VaPor_RPOS", "VaPor_REND", "VaPor_QS0", "VaPor_GS0"] and keys_p[-4:] == ["VaPor_GS", "VaPor_GT", "VaPor_GQ", "VaPor_REC"]
        extra = dict(x.split("=") for x in r[7].split(";")[-4:])
        if t in moves:
            l, (ms, me) = w.loci[t], moves[t]
            a, b = int(extra["VaPor_RPOS"]), int(extra["VaPor_REND"])
            lo, hi = got_ci[list(got_ci)[t]][0]
            assert lo <= a - (l.start + ms) <= hi and (a - (l.start + ms)) % 10 == 0
            lo, hi = got_ci[list(got_ci)[t]][1]
            assert lo <= b - (l.end + me) <= hi and (b - (l.end + me)) % 10 == 0
            assert abs(a - l.start) + abs(b - l.end) <= abs(ms) + abs(me)
            assert float(extra["VaPor_GS0"]) <= float(dict(x.split("=") for x in r[7].split(";") if "=" in x)["VaPor_GS"])
        else:
            assert p[7] == ";".join(r[7].split(";")[:-4]) and set(extra.values()) == {"."}       # INS, and the DEL below 50 bp


def test_usage_errors(capsys):
    base = ["--sv-input", "a.bed", "--reference", "r.fa", "--pacbio-input", "x.bam", "--output-path", "o", "--output-file", "o.vapor"]
    for mode, spec in (("bed", "50:8"), ("vcf", "x"), ("svelter", "10")):
        with pytest.raises(SystemExit) as e:
            cli.main([mode] + base + ["--refine", spec])
        assert e.value.code == 2
    assert "at most 128" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------

def test_entry_points_are_declared_optional_and_refused_by_the_twin(twin_eng, oracle):
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    for name in ("vapor_plan_set_grid", "vapor_plan_run_grid"):
        assert re.search(r"\bint %s\(" % name, h) and name in L.EXPORTS and name in L.OPTIONAL_EXPORTS
    assert "#define VAPOR_MAX_CANDIDATES 128" in h and L.ABI_VERSION == 3
    assert not twin_eng.grid_available() and not pipeline.has_grid(twin_eng) and not pipeline.has_grid(FakeEngine(None))
    ss = twin_eng.seqset(["ACGTACGTACGTTTGACCA", "ACGTACGTACGTAACGT"])
    plan = twin_eng.plan(ss, twin_eng.make_pairs([(0, 1, 0, 10, 3)]))
    with pytest.raises(NotImplementedError, match="refinement kernel"):
        plan.set_grid(np.asarray([0, 1], dtype=np.int32))
    with pytest.raises(NotImplementedError):
        pipeline.score_grids(twin_eng, [], route="batched")
    raw = ctypes.CDLL(oracle.build_twin())
    raw.vapor_plan_set_grid.restype = ctypes.c_int
    assert raw.vapor_plan_set_grid(None, 0, None) == L.E_ARG
    plan.close(); ss.close()
