"""`--phased` on the device (vapor_bam_chop_device_tagged: the tag walk in the chop kernel, bam_select_kernel) against the host
readers (vapor_bam_chop_tagged + phase.select): the union of the three group lists, the membership words, the phase set, miss_bp
and the bases as bit planes, on files with blocks of 64 KB and 1.5 KB, every tag case of tests/test_phase_cpu.py, a 70 001-
operation CG record, groups above the cap of 20, a region above its slot of 256 and records with a malformed aux area (their
regions go to the host route, their neighbours do not); then `vapor bed --phased` from files on the device route against the
host-reader route, the drivers' route and the CPU twin's table."""
import copy
import ctypes
import os

import numpy as np
import pytest

import test_phase_cpu as TP
from vapor_amd import _lib as L
from vapor_amd import bamio, cli, phase, pipeline, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def compare(eng, bam, regions, max_keep=20):
    """regions: (chrom, start, end, flank).  Returns the device's status per region, the reads compared and the selections
    (tagged, P, member words) of the regions it answered; for every such region the union, the member words, the phase set,
    miss_bp and the bases are the host's."""
    be = seqio.InProcessBam()
    b = be._open(bam)
    chroms = [r[0] for r in regions]
    st = np.asarray([r[1] for r in regions], dtype=np.int64)
    en = np.asarray([r[2] for r in regions], dtype=np.int64)
    fl = np.asarray([r[3] for r in regions], dtype=np.int64)
    dkf, daddr, dq0, dmiss, dstatus, batches, dmember, dps, dtagged = be.chop_many_device(eng, bam, chroms, st, en, fl, max_keep, groups=True)
    texts, lens, sel, answers = [], [], [], {}
    try:
        for g in range(len(regions)):
            if dstatus[g]:
                continue
            r = b.chop_native_raw(chroms[g], int(st[g]), int(en[g]), int(fl[g]), tagged=True)
            a, e = int(dkf[g]), int(dkf[g + 1])
            if r is None:
                assert e == a and not dtagged[g] and dps[g] == phase.PS_NONE, g
                continue
            whole, off, ln, miss, hap, ps = r
            tagged, p, order, words = phase.select_numbers(miss, hap, ps, max_keep)
            assert (bool(dtagged[g]), int(dps[g])) == (tagged, p), (g, regions[g])
            assert e - a == len(order) <= 3 * max_keep and dmiss[a:e].tolist() == miss[order].tolist(), (g, regions[g])
            assert dmember[a:e].tolist() == words, (g, regions[g])
            answers[g] = (tagged, p, words, [(int(hap[i]), int(ps[i])) for i in order])
            for t, i in enumerate(order):
                assert int(ln[i]) == int(en[g] - st[g] - miss[i])
                texts.append(whole[int(off[i]):int(off[i]) + int(ln[i])])
                lens.append(int(ln[i]))
                sel.append(a + t)
        if texts:
            sel = np.asarray(sel)
            dev = eng.seqset_raw(daddr[sel], np.asarray(lens, dtype=np.int64), None, src_kind=np.ones(len(sel), dtype=np.uint8), src_first=dq0[sel])
            ref = eng.seqset(texts)
            try:
                for t in range(len(texts)):
                    assert all(np.array_equal(x, y) for x, y in zip(dev.planes(t), ref.planes(t))), t
            finally:
                dev.close()
                ref.close()
    finally:
        for bt in batches:
            bt.close()
        b.close()
    # the host readers' groups form gives the same arrays (what the array route takes where the device leaves a region)
    hkf, _haddr, _hq0, hmiss, hstatus, _keep, hmember, hps, htagged = be.chop_many(bam, chroms, st, en, fl, max_keep, groups=True)
    for g in range(len(regions)):
        if dstatus[g] == 0 and hstatus[g] == 0:
            assert hmember[hkf[g]:hkf[g + 1]].tolist() == dmember[dkf[g]:dkf[g + 1]].tolist() and hps[g] == dps[g] and htagged[g] == dtagged[g]
            assert hmiss[hkf[g]:hkf[g + 1]].tolist() == dmiss[dkf[g]:dkf[g + 1]].tolist()
    return dstatus, len(texts), answers


def _sorted(w):
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    return w


def test_oracle_world_files_large_and_small_blocks(eng, tmp_path):
    w = _sorted(TP._oracle_world())
    for block in (0xFF00, 1500):
        d = tmp_path / ("b%d" % block)
        d.mkdir()
        fa, bam = synth.write_world_files(w, str(d), block_size=block)
        regions = [(l.chrom, max(l.start - 400, 1), l.start + 900, 400) for l in w.loci] + [("no_such_contig", 5, 900, 100), (w.loci[0].chrom, 1, 40, 10)]
        status, n, answers = compare(eng, bam, regions)
        assert status.tolist() == [0] * len(regions) and n == 938, (block, status.tolist(), n)
        for g in range(36):
            tagged, p, words, _tags = answers[g]
            assert tagged and p == 1 and 7 <= sum(1 for x in words if x & 1) <= 20 and sum(1 for x in words if x & 2) >= 1
        st = eng.bam_last_stats()
        assert 0 < st["d2h_bytes"] < len(regions) * (3 * 20 * 16 + 16 + 8) + 4 * st["blocks"] + 4096


def test_every_tag_case_a_long_cg_record_and_malformed_aux_areas(eng, tmp_path):
    cases = TP.TAG_CASES
    recs = [(name, 0, 10000 * t + 100, "4000M", "ACGT" * 1000, aux) for t, (name, aux, _sam, _exp) in enumerate(cases)]
    t_long = len(cases)
    recs.append(("long_cg", 0, 10000 * t_long + 500, "1M1I" * 35000 + "5000M", "AC" * 35000 + "G" * 5000, {"MM": "m" * 300, "HP": 2, "PS": ("I", 4000000000)}))
    for block in (0xFF00, 1500):
        bam = str(tmp_path / ("tags%d.bam" % block))
        bamio.write_bam(bam, [("c", 10000 * (t_long + 2) + 80000)], recs, block_size=block)
        regions = [("c", 10000 * t + 1000, 10000 * t + 3000, 500) for t in range(t_long + 1)]
        status, n, answers = compare(eng, bam, regions)
        bad = {t for t, c in enumerate(cases) if c[0] in ("truncated_Z", "truncated_i", "unknown_type")}
        assert {t for t in range(len(regions)) if status[t]} == bad and all(status[t] == 2 for t in bad)      # the host route's, no other
        for t, (name, _aux, _sam, exp) in enumerate(cases):
            if t not in bad:
                assert answers[t][3] == [(exp[0], phase.PS_NONE if exp[1] is None else exp[1])], name
        assert answers[t_long][3] == [(2, 4000000000)] and n == len(regions) - len(bad)
        # one region over many of them: the malformed records are inside it
        status, _n, _a = compare(eng, bam, [("c", 100, 10000 * (t_long + 1), 500), ("c", 10000 * t_long + 1000, 10000 * t_long + 2000, 500)])
        assert status.tolist() == [0, 0]                   # (no record of the first region is kept: none is walked)
    # the host readers give the malformed records the tags of the table
    be = seqio.InProcessBam()
    for t in sorted(bad):
        got = be.chop(bam, "c", 10000 * t + 1000, 10000 * t + 3000, 500, tagged=True)
        assert [(r[3], r[4]) for r in got] == [cases[t][3]]


def test_groups_above_the_cap_two_phase_sets_and_a_full_slot(eng, tmp_path):
    rng = np.random.default_rng(8)
    contig = synth.random_dna(rng, 60000)
    recs = []
    for i in range(140):
        pos = 4000 + int(rng.integers(0, 900))
        pre = int(rng.integers(0, 40))
        read, cg = synth.mutate(rng, contig[pos:pos + 6000])
        u = rng.random()
        tags = None if u < 0.15 else {"HP": int(rng.integers(1, 3)), "PS": 7 if u < 0.7 else 9} if u < 0.9 else {"HP": int(rng.integers(0, 4))}
        recs.append(("m%d" % i, 0, pos, ("%dS" % pre if pre else "") + "%dD" % int(rng.integers(1, 700)) + cg, synth.random_dna(rng, pre) + read, tags))
    p = str(tmp_path / "many.bam")
    bamio.write_bam(p, [("c", 60000)], recs, block_size=0xFF00)
    status, n, answers = compare(eng, p, [("c", 4900, 6100, 1000), ("c", 5200, 5900, 1400)])
    assert status.tolist() == [0, 0]
    for g in (0, 1):
        tagged, ps, words, tags = answers[g]
        assert tagged and ps == 7
        sizes = [sum(1 for x in words if (x >> b) & 1) for b in range(3)]
        assert sizes[0] == 20 and 1 <= sizes[1] <= 20 and 1 <= sizes[2] <= 20 and 20 < len(words) <= 60
        if g == 0:
            assert sizes == [20, 20, 20]
    for keep in (5, 64, 256):
        status, _n, answers = compare(eng, p, [("c", 4900, 6100, 1000)], max_keep=keep)
        sizes = [sum(1 for x in answers[0][2] if (x >> b) & 1) for b in range(3)]
        assert status.tolist() == [0] and sizes == {5: [5, 5, 5], 64: [64, 30, 50], 256: [137, 30, 50]}[keep]
        if keep == 64:                                      # (the other phase set's tagged reads: in list A only)
            assert any(t == (h, 9) and (w & 7) == 1 for t, w in zip(answers[0][3], answers[0][2]) for h in (1, 2))
    # 300 kept reads in one region: beyond the 256 a region's slot holds - the host route's
    big = [("b%d" % i, 0, 100 + i, "30000M", "ACGT" * 7500, {"HP": 1 + i % 2, "PS": 3}) for i in range(300)]
    p3 = str(tmp_path / "big.bam")
    bamio.write_bam(p3, [("c", 60000)], big)
    status, n, _a = compare(eng, p3, [("c", 500, 25000, 500), ("c", 150, 900, 30)])
    assert status[0] == 4 and status[1] == 0 and n == 40


def _tables(tmp_path, bed_text, fa, bam, runs, monkeypatch):
    bed = tmp_path / "in.bed"
    bed.write_text(bed_text)
    out = {}
    seqio.set_backend(seqio.InProcessBam())
    monkeypatch.setenv("VAPOR_QC_SEED", "7")
    for name, env, extra in runs:
        for k in ("VAPOR_BAM_DEVICE", "VAPOR_FAST_PATH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        o = tmp_path / (name + ".vapor")
        assert cli.main(["bed", "--sv-input", str(bed), "--reference", fa, "--pacbio-input", bam, "--output-path", str(tmp_path / "figs"),
                         "--output-file", str(o), "--no-figures"] + extra) == 0
        out[name] = o.read_text()
    for k in ("VAPOR_BAM_DEVICE", "VAPOR_FAST_PATH"):
        monkeypatch.delenv(k, raising=False)
    return out


RUNS = [("device", {}, ["--phased"]), ("host", {"VAPOR_BAM_DEVICE": "0"}, ["--phased"]), ("drivers", {"VAPOR_FAST_PATH": "0"}, ["--phased"]),
        ("unphased", {}, [])]


@pytest.mark.parametrize("which", ["oracle", "gate", "two_sets"])
def test_cli_tables_device_route_host_route_drivers_and_twin(tmp_path, which, monkeypatch, oracle):
    if which == "oracle":
        w = TP._oracle_world()
    elif which == "gate":
        w = synth.phase_world(synth.make_world(seed=73, n_loci=36, svtypes=("DEL", "INV", "INS"), span_range=(100, 3000), read_len=7000,
                                               n_reads=16), seed=1073)
    else:
        w = TP._two_set_world()
    _sorted(w)
    fa, bam = synth.write_world_files(w, str(tmp_path), block_size=0xFF00)
    bed = synth.bed_text(w)
    seen = []
    real = Engine.bam_chop_device

    def spy(self, *a, **k):
        got = real(self, *a, **k)
        seen.append((bool(k.get("tagged")), got[4].tolist()))
        return got
    monkeypatch.setattr(Engine, "bam_chop_device", spy)
    pipeline.set_engine(None)
    try:
        t = _tables(tmp_path, bed, fa, bam, RUNS, monkeypatch)
        # the device answered every region of the phased run itself
        tagged_calls = [s for s in seen if s[0]]
        assert len(tagged_calls) == 1 and set(tagged_calls[0][1]) == {0} and len(tagged_calls[0][1]) == len(w.loci)
        assert t["device"] == t["host"] == t["drivers"]
        rows = [ln.split("\t") for ln in t["device"].splitlines()]
        assert [ln.split("\t") for ln in t["unphased"].splitlines()] == [r[:10] for r in rows]
        # the CPU twin's table from the same files
        saved = L._lib
        L._lib = L.bind(ctypes.CDLL(oracle.build_twin()))
        e = Engine(0)
        pipeline.set_engine(e)
        try:
            twin = _tables(tmp_path, bed, fa, bam, [("twin", {}, ["--phased"])], monkeypatch)["twin"]
        finally:
            pipeline.set_engine(None)
            e.close()
            L._lib = saved
        assert twin == t["device"]
    finally:
        pipeline.set_engine(None)
        seqio.set_backend(None)
    if which == "oracle":
        # the subset oracle on the device route: the H_h columns are the unphased run's on the file that keeps the HP = h records
        subs = []
        for h in (1, 2):
            d = tmp_path / ("h%d" % h)
            d.mkdir()
            fa_h, bam_h = synth.write_world_files(TP._only_hap(w, h), str(d), block_size=0xFF00)
            try:
                subs.append([ln.split("\t") for ln in _tables(d, bed, fa_h, bam_h, [("sub", {}, [])], monkeypatch)["sub"].splitlines()])
            finally:
                seqio.set_backend(None)
        TP._check_subset_oracle(rows, subs[0], subs[1], [r[:10] for r in rows])
        # an unphased run from the tagged file equals the unphased run from the same file written without tags
        plain = copy.copy(w)
        plain.reads = {c: [synth.SamRecord(r.qname, r.rname, r.pos, r.cigar, r.seq, r.ref_span) for r in rs] for c, rs in w.reads.items()}
        d = tmp_path / "plain"
        d.mkdir()
        fa0, bam0 = synth.write_world_files(plain, str(d), block_size=0xFF00)
        try:
            assert _tables(d, bed, fa0, bam0, [("un", {}, [])], monkeypatch)["un"] == t["unphased"]
        finally:
            seqio.set_backend(None)
    elif which == "gate":
        assert sum(1 for r in rows[1:] for h in (0, 1) if r[13 + 3 * h:16 + 3 * h] == [".", ".", "."]) == 3
    else:
        assert {r[10] for r in rows[1:]} == {"20", "40", "."} and {r[3] for r in rows[1:] if "." not in r[11:]} == {"DEL", "INV", "TANDUP", "INS"}
