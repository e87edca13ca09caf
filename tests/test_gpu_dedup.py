"""`--dedup-qname` on the device (vapor_bam_set_dedup on the handle the four vapor_bam_chop_device* calls are made
with, bam_dedup_kernel behind their chop kernel): every call with the option against the host reader with the option AND against
the same call without it on the file written without the records rule W drops - kept reads, q0 / q1, miss_bp, member, phase set,
tagged, status and the bases behind every address; the name keys of a batch against seqio.name_key of the host route's names.
The dropped records are named by a direct statement over the QNAMEs themselves, not over keys.  Small files on purpose: reads of
400 bases, a window of 100 bp, BGZF blocks of 2 KB, a region per way the kernel could go wrong."""
import numpy as np
import pytest

from vapor_amd import _lib as L
from vapor_amd import bamio, cli, phase, pipeline, seqio, synth
from vapor_amd import simple_function as SF
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu

BLOCK = 2048
START, END, FLANK = 2000, 2100, 50
Q, F = 20, 0x400                        # the handle's read filter: one region holds records it filters
KEPT_CAP, REG_KEPT_FULL = 256, 4


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def passes(rec):
    return not (rec[6] < Q or (rec[7] & F))


def survivors(recs):
    """Rule W by its words, over the QNAMEs: of the records of one contig that pass the filter (all of them are kept by the
    window, in file order) one per name survives - the first that is neither secondary nor supplementary, else the first."""
    out = []
    by_tid = {}
    for i, r in enumerate(recs):
        if r[8] and passes(r):
            by_tid.setdefault(r[1], []).append(i)
    dropped = set()
    for idx in by_tid.values():
        for i in idx:
            same = [j for j in idx if recs[j][0] == recs[i][0]]
            prim = [j for j in same if not recs[j][7] & 0x900]
            if i != (prim[0] if prim else same[0]):
                dropped.add(i)
    for i, r in enumerate(recs):
        if i not in dropped:
            out.append(r)
    return out, dropped


def designed():
    """(refs, records with a `kept by the window` mark as ninth field, regions, sites): a contig per case; every marked record
    is a 400-base copy of its contig that starts before the window and ends behind it, POS ascending in the order given."""
    rng = np.random.default_rng(91)
    refs, recs, sites = [], [], []

    def contig(name, n=6000):
        refs.append((name, n))
        ref = synth.random_dna(rng, n)
        for p in range(1710, 2000, 23):
            r = ref[p - 1]
            alt = "ACGT"[("ACGT".index(r) + 1 + p % 3) % 4]
            sites.append((name, p, r, alt, 5) if p % 2 else (name, p, alt, r, 5 if p % 3 else 6))
        return len(refs) - 1, ref

    def put(tid, ref, rows, pos0=1700, step=1):
        """rows: (name, FLAG[, MAPQ]) in file order"""
        for i, row in enumerate(rows):
            name, flag = row[0], row[1]
            mapq = row[2] if len(row) > 2 else 60
            a = pos0 + i * step
            k = len(recs)
            recs.append((name, tid, a, "400M", ref[a:a + 400], {"HP": 1 + k % 2, "PS": 7 if k % 4 else 9} if k % 5 else None, mapq, flag, True))

    t, ref = contig("adjacent")
    put(t, ref, [("u0", 0), ("m", 0), ("m", 0x800), ("u1", 0x10)])
    t, ref = contig("apart65")           # kept entries 2 and 67 are one molecule, 3 and 69 another: the survivors shift across the tiles
    rows = [("s%d" % i, 0) for i in range(72)]
    rows[2], rows[67] = ("far", 0x100), ("far", 0)
    rows[3], rows[69] = ("far2", 0), ("far2", 0x800)
    put(t, ref, rows)
    t, ref = contig("supp_first")
    put(t, ref, [("m", 0x800), ("u0", 0), ("m", 0), ("u1", 0)])
    t, ref = contig("three")
    put(t, ref, [("m", 0x100), ("u0", 0), ("m", 0x10), ("m", 0), ("u1", 0)])
    t, ref = contig("all_one")
    put(t, ref, [("m", 0x100), ("m", 0x800), ("m", 0), ("m", 0), ("m", 0x900)])
    t, ref = contig("pairs256")
    put(t, ref, [("p%d" % (i % 128), 0x800 if (i * 7) % 3 == 0 else 0) for i in range(256)])
    t, ref = contig("full257")
    put(t, ref, [("f%d" % (i % 200), 0) for i in range(257)])
    t, ref = contig("lengths")           # names whose last byte falls on every side of a lane's four bytes
    rows = []
    for n in (1, 3, 4, 5, 63, 64, 65, 254):
        nm = "".join("ACGTNacgtn0123456789_/:"[(i * 7 + n) % 23] for i in range(n))
        rows += [(nm, 0x800), (nm[:-1] + ("x" if nm[-1] != "x" else "y"), 0), (nm, 0)]
    put(t, ref, rows)
    t, ref = contig("prefix200")         # a 200-byte prefix in common, the last byte decides
    pre = "m64011_190830_220126/" + "7" * 179
    assert len(pre) == 200
    put(t, ref, [(pre + "a", 0), (pre + "b", 0), (pre + "a", 0x100), (pre + "c", 0x800), (pre + "b", 0x800), (pre, 0), (pre, 0)])
    t, ref = contig("is_prefix")
    put(t, ref, [("abc", 0x800), ("abcd", 0), ("abc", 0), ("ab", 0), ("abcd", 0x100), ("abcde", 0)])
    t, ref = contig("straddle")          # the header of `straddle_d` lies in two BGZF blocks (fillers in front of it take the padding)
    for i in range(14):
        recs.append(("fill%02d" % i, t, 100 + i, "400M", ref[100 + i:500 + i], None, 60, 0, False))
    put(t, ref, [("u0", 0), ("straddle_d", 0x800), ("u1", 0), ("straddle_d", 0), ("u2", 0)], pos0=1750)
    t, ref = contig("long_cigar", 40000)  # a record whose 70 000 operations are in CG:B,I among the duplicates
    put(t, ref, [("cg", 0x100), ("u0", 0)])
    recs.append(("cg", t, 1900, "1M1I" * 35000, synth.random_dna(rng, 70000), {"HP": 1, "PS": 7}, 60, 0, True))
    put(t, ref, [("u1", 0), ("cg", 0x800)], pos0=1950)
    t, ref = contig("filtered")          # a filtered record between two duplicates, and a filtered would-be survivor
    put(t, ref, [("m", 0x800), ("m", 0, 5), ("m", 0x100), ("w", 0x400), ("w", 0x800), ("w", 0x100), ("u", 0)])
    t, ref = contig("none")              # records of the region, none before the window start: n_kept 0
    for i in range(3):
        recs.append(("late%d" % i, t, 2010 + i, "400M", ref[2010 + i:2410 + i], None, 60, 0, False))
    t, ref = contig("one")
    put(t, ref, [("only", 0x800)])
    regions = [(name, START, END, FLANK) for name, _n in refs]
    return refs, recs, regions, sites


def _straddle_pad(path, refs, recs):
    """Writes the file so that the header of the primary `straddle_d` crosses a block boundary: the fillers' names take the padding."""
    def where():
        b = bamio.BamFile(path)
        cur = b.bgzf.read_from(b.first_record)
        hit = 0
        while True:
            at = cur.tell()
            hdr = cur.read(4)
            if len(hdr) < 4:
                return None
            r = cur.read(int.from_bytes(hdr, "little"))
            if r[32:32 + r[8] - 1] == b"straddle_d":
                hit += 1
                if hit == 2:
                    return at & 0xFFFF
    w = [r[:8] for r in recs]
    bamio.write_bam(path, refs, w, block_size=BLOCK)
    shift = (BLOCK - 20 - where()) % BLOCK
    out = []
    for r in recs:
        if r[0].startswith("fill") and shift:
            take = min(shift, 200)
            shift -= take
            r = (r[0] + "x" * take,) + r[1:]
        out.append(r)
    assert shift == 0
    bamio.write_bam(path, refs, [r[:8] for r in out], block_size=BLOCK)
    u = where()
    assert u < BLOCK < u + 36, u                       # the 36 bytes the walk loads first lie in two blocks
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_dd")
    refs, recs, regions, sites = designed()
    x = str(d / "x.bam")
    recs = _straddle_pad(x, refs, recs)
    rest, dropped = survivors(recs)
    p = str(d / "p.bam")
    bamio.write_bam(p, refs, [r[:8] for r in rest], block_size=BLOCK)
    by = {}
    for i in dropped:
        by[refs[recs[i][1]][0]] = by.get(refs[recs[i][1]][0], 0) + 1
    assert by == {"adjacent": 1, "apart65": 2, "supp_first": 1, "three": 2, "all_one": 4, "pairs256": 128, "full257": 57, "lengths": 8,
                  "prefix200": 3, "is_prefix": 2, "straddle": 1, "long_cigar": 2, "filtered": 2}, by
    return x, p, regions, phase.Sites.from_rows(sites), recs, refs


MODES = {"plain": {}, "right": {"right": True}, "tagged": {"groups": True}, "haplotag": {"groups": True}}


def device(eng, be, bam, regions, mode, sites, max_keep=20, keys=False):
    """One device call; per region (status, [(q, miss, member, planes of the read's bases)]), and phase set / tagged per region."""
    kw = dict(MODES[mode])
    if mode == "haplotag":
        kw["sites"] = sites
    st = np.asarray([r[1] for r in regions], dtype=np.int64)
    en = np.asarray([r[2] for r in regions], dtype=np.int64)
    fl = np.asarray([r[3] for r in regions], dtype=np.int64)
    got = be.chop_many_device(eng, bam, [r[0] for r in regions], st, en, fl, max_keep, **kw)
    kf, addr, q, miss, status, batches = got[:6]
    member = got[6] if len(got) > 6 else np.zeros(len(addr), dtype=np.uint32)
    out = []
    try:
        lens = np.asarray([int(en[g] - st[g] - miss[t]) for g in range(len(regions)) for t in range(int(kf[g]), int(kf[g + 1]))], dtype=np.int64)
        planes = []
        if len(addr):
            ss = eng.seqset_raw(addr, lens, None, src_kind=np.full(len(addr), 2 if mode == "right" else 1, dtype=np.uint8), src_first=q)
            try:
                planes = [tuple(a.tobytes() for a in ss.planes(t)) for t in range(len(addr))]
            finally:
                ss.close()
        for g in range(len(regions)):
            out.append((int(status[g]), [(int(q[t]), int(miss[t]), int(member[t]), planes[t]) for t in range(int(kf[g]), int(kf[g + 1]))]))
        if keys:
            name_keys = [None if bt.name_keys is None else [int(k) for k in bt.name_keys] for bt in batches]
            return out, kf.tolist(), name_keys
    finally:
        for bt in batches:
            bt.close()
    extra = (got[7].tolist(), got[8].tolist()) if len(got) > 6 else None
    return out, extra


def host(eng, be, bam, regions, mode, sites, max_keep=20):
    """The host reader's answer in the same shape, without q (the host hands text): (status, [(miss, member, planes)])."""
    out = []
    texts = []
    if mode == "right":
        b = be._open(bam)
        for c, a, e, fl in regions:
            got = seqio.minimize_pacbio_read_list(b.chop_native(c, a, e, fl, right=True), max_keep)
            out.append([0, [(r[1], 0) for r in got]])
            texts += [r[0] for r in got]
        extra = None
    else:
        kw = dict(MODES[mode])
        if mode == "haplotag":
            kw["sites"] = sites
        import ctypes
        got = be.chop_many(bam, [r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions], [r[3] for r in regions], max_keep, **kw)
        kf, addr, q0, miss, status = got[:5]
        member = got[6] if len(got) > 6 else np.zeros(len(addr), dtype=np.uint32)
        for g, r in enumerate(regions):
            out.append([int(status[g]), [(int(miss[t]), int(member[t])) for t in range(int(kf[g]), int(kf[g + 1]))]])
            texts += [ctypes.string_at(int(addr[t]) + int(q0[t]), r[2] - r[1] - int(miss[t])).decode() for t in range(int(kf[g]), int(kf[g + 1]))]
        extra = (got[7].tolist(), got[8].tolist()) if len(got) > 6 else None
    planes = []
    if texts:
        ss = eng.seqset(texts)
        try:
            planes = [tuple(a.tobytes() for a in ss.planes(t)) for t in range(len(texts))]
        finally:
            ss.close()
    t = 0
    for g in range(len(out)):
        out[g] = (out[g][0], [(m, mem, planes[t + i]) for i, (m, mem) in enumerate(out[g][1])])
        t += len(out[g][1])
    return out, extra


def _backends():
    bx, bp, b0 = seqio.InProcessBam(), seqio.InProcessBam(), seqio.InProcessBam()
    for be in (bx, bp, b0):
        be.read_filter = (Q, F)
    bx.dedup_qname = True
    return bx, bp, b0


def _close(*bes):
    for be in bes:
        for b in be._bam.values():
            b.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_device_with_the_option_is_the_host_with_it_and_the_device_on_the_file_without_the_dropped_records(eng, files, mode):
    x, p, regions, sites, recs, refs = files
    bx, bp, b0 = _backends()
    full = [r[0] for r in regions].index("full257")
    rest = [g for g in range(len(regions)) if g != full]
    sub = [regions[g] for g in rest]
    # every kept record of a region comes back (max_keep = the slot's size), and once more under the drivers' cap of 20
    for max_keep in (KEPT_CAP, 20):
        dx, ex = device(eng, bx, x, regions, mode, sites, max_keep)
        dp, ep = device(eng, bp, p, regions, mode, sites, max_keep)
        assert [dx[g] for g in rest] == [dp[g] for g in rest]                # as if the dropped records were not in the file
        if ex is not None:
            assert [[e[g] for g in rest] for e in ex] == [[e[g] for g in rest] for e in ep]
        assert [dx[g][0] for g in rest] == [0] * len(rest)
        # 257 kept records before the rule: the region is the host route's, as without the option
        assert dx[full] == (REG_KEPT_FULL, []) and dp[full][0] == 0
        hx, eh = host(eng, bx, x, sub, mode, sites, max_keep)
        assert [(s, [r[1:] for r in rd]) for s, rd in (dx[g] for g in rest)] == hx
        if ex is not None:
            assert [[e[g] for g in rest] for e in ex] == [list(e) for e in eh]
    # the counts are the designed ones: the option decides something in every region but the last two
    if mode in ("plain", "right"):
        dx, _ = device(eng, bx, x, regions, mode, sites, KEPT_CAP)
        d0, _ = device(eng, b0, x, regions, mode, sites, KEPT_CAP)
        want, _dropped = survivors(recs)
        n_live = {name: sum(1 for r in want if r[8] and passes(r) and refs[r[1]][0] == name) for name, _n in refs}
        n_all = {name: sum(1 for r in recs if r[8] and passes(r) and refs[r[1]][0] == name) for name, _n in refs}
        for g in rest:
            name = regions[g][0]
            assert len(dx[g][1]) == n_live[name] and len(d0[g][1]) == n_all[name], name
        assert n_live["pairs256"] == 128 and n_all["pairs256"] == 256 and n_live["none"] == 0 and n_live["one"] == 1 and n_live["all_one"] == 1
    _close(bx, bp, b0)


def test_the_region_the_device_hands_back_goes_the_host_route_which_applies_the_rule(eng, files):
    x, p, regions, _sites, _recs, _refs = files
    bx, bp, _b0 = _backends()
    reg = [r for r in regions if r[0] == "full257"][0]
    seqio.set_backend(bx)
    try:
        final = seqio.chop_pacbio_read_by_pos(x, *reg)
    finally:
        seqio.set_backend(None)
    assert len(final) == 200 and final == bp.chop(p, *reg)
    _close(bx, bp)


@pytest.mark.parametrize("mode", ["plain", "right"])
def test_name_keys_of_a_batch_are_the_keys_of_the_host_routes_names(eng, files, mode):
    x, _p, regions, sites, _recs, _refs = files
    bx, _bp, b0 = _backends()
    regions = [r for r in regions if r[0] != "full257"]
    for max_keep in (KEPT_CAP, 20):
        dx, kf, keys = device(eng, bx, x, regions, mode, sites, max_keep, keys=True)
        assert len(keys) == 1 and len(keys[0]) == kf[-1] > 0
        b = bx._open(x)
        want = []
        for c, a, e, fl in regions:
            got = seqio.minimize_pacbio_read_list(b.chop_native(c, a, e, fl, right=(mode == "right")), max_keep)
            want += [seqio.name_key(r[2]) for r in got]
        assert keys[0] == want
    # a batch made without the option has none
    _d0, _kf0, keys0 = device(eng, b0, x, regions, mode, sites, 20, keys=True)
    assert keys0 == [None]
    _close(bx, b0)


def test_name_keys_are_refused_for_a_tagged_batch_and_for_a_batch_made_without_the_option(eng, files):
    x, _p, regions, sites, _recs, _refs = files
    bx, _bp, b0 = _backends()
    regions = regions[:3]
    st, en, fl = ([r[k] for r in regions] for k in (1, 2, 3))
    names = [r[0] for r in regions]
    for be, kw in ((bx, {"groups": True}), (bx, {"groups": True, "sites": sites}), (b0, {}), (b0, {"right": True})):
        got = be.chop_many_device(eng, x, names, np.asarray(st), np.asarray(en), np.asarray(fl), 20, **kw)
        try:
            n = int(got[0][-1])
            assert n > 0 and got[5][0].name_keys is None
            for count in (n, 0):
                with pytest.raises(L.VaporHipError) as ei:
                    got[5][0].read_name_keys(count)
                assert ei.value.code == L.E_ARG
        finally:
            for bt in got[5]:
                bt.close()
    # the right count is the only one taken
    got = bx.chop_many_device(eng, x, names, np.asarray(st), np.asarray(en), np.asarray(fl), 20)
    try:
        n = int(got[0][-1])
        assert len(got[5][0].read_name_keys(n)) == n == len(got[5][0].name_keys)
        for count in (n - 1, n + 1):
            with pytest.raises(L.VaporHipError):
                got[5][0].read_name_keys(count)
    finally:
        for bt in got[5]:
            bt.close()
    _close(bx, b0)


@pytest.mark.parametrize("mode", list(MODES))
def test_a_handle_with_the_option_off_answers_as_one_that_never_had_it(eng, files, mode):
    """kept_first, the addresses relative to the arena, q0, miss_bp, status, member and the bytes copied back: a handle whose option
    was set and taken back, one that never had it, and the host reader without it."""
    x, _p, regions, sites, _recs, _refs = files
    kw = dict(MODES[mode])
    if mode == "haplotag":
        kw["sites"] = sites
    st, en, fl = (np.asarray([r[k] for r in regions], dtype=np.int64) for k in (1, 2, 3))
    names = [r[0] for r in regions]
    answers = []
    for toggled in (False, True):
        be = seqio.InProcessBam()
        if toggled:
            be.dedup_qname = True
            got = be.chop_many_device(eng, x, names, st, en, fl, 20, **kw)      # (the file's handle now carries the option ...)
            for bt in got[5]:
                bt.close()
            be.dedup_qname = False                                              # (... and loses it again)
        got = be.chop_many_device(eng, x, names, st, en, fl, 20, **kw)
        try:
            addr = got[1]
            base = int(addr.min()) if len(addr) else 0
            answers.append([got[0].tolist(), (addr - np.uint64(base)).tolist(), got[2].tolist(), got[3].tolist(), got[4].tolist()]
                           + [np.asarray(a).tolist() for a in got[6:]] + [eng.bam_last_stats()["d2h_bytes"]])
            assert got[5][0].name_keys is None
        finally:
            for bt in got[5]:
                bt.close()
        _close(be)
    assert answers[0] == answers[1]
    be = seqio.InProcessBam()
    d0, e0 = device(eng, be, x, regions, mode, sites)
    sub = [r for r in regions if r[0] != "full257"]
    h0, eh = host(eng, be, x, sub, mode, sites)
    assert [(s, [r[1:] for r in rd]) for (s, rd), reg in zip(d0, regions) if reg[0] != "full257"] == h0
    _close(be)


def _cli(tmp_path, name, text, fa, bam, more):
    d = tmp_path / name
    d.mkdir()
    src = d / "in.bed"
    src.write_text(text)
    out = d / "out.vapor"
    assert cli.main(["bed", "--sv-input", str(src), "--reference", fa, "--pacbio-input", bam, "--output-path", str(d / "figs"),
                     "--output-file", str(out), "--no-figures"] + list(more)) == 0
    return out.read_text()


@pytest.mark.parametrize("case", ["both_ends", "phased"])
def test_cli_from_files_on_a_split_alignment_world_gives_the_tables_of_the_host_route(tmp_path, case, monkeypatch):
    """`bed --both-ends --dedup-qname` and `bed --phased --dedup-qname` from files, reads selected on the device, against the
    same run with VAPOR_BAM_DEVICE=0 (the native host reader); and the option decides something in these tables."""
    monkeypatch.setenv("VAPOR_QC_SEED", "7")
    base = synth.make_junction_world(61, ("DEL", "TANDUP", "DEL"), n_reads=8, ref_fraction=0.0)
    short = synth.make_world(seed=62, n_loci=2, svtypes=("DEL", "TANDUP"), span_range=(600, 900), read_len=3000, n_reads=8, alt_fraction=1.0)
    base.contigs.update(short.contigs)
    base.reads.update(short.reads)
    base.loci += short.loci
    if case == "phased":
        synth.phase_world(base, 9)
    w = synth.add_split_alignments(base, "full", window_dups=3)
    assert w.planted["split"] >= 16 and w.planted["window"] == 3
    fa, bam = synth.write_world_files(w, str(tmp_path), block_size=BLOCK)
    text = synth.bed_text(w)
    more = ["--both-ends"] if case == "both_ends" else ["--phased"]
    seqio.set_backend(seqio.InProcessBam())
    try:
        on_dev = _cli(tmp_path, "dev", text, fa, bam, more + ["--dedup-qname"])
        assert pipeline.engine_slot(0).bam_last_stats()["regions"] > 0        # (the reads of that run were selected on the device)
        off_dev = _cli(tmp_path, "dev_off", text, fa, bam, more)
        monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
        on_host = _cli(tmp_path, "host", text, fa, bam, more + ["--dedup-qname"])
    finally:
        seqio.set_backend(None)
    assert on_dev == on_host and on_dev != off_dev and on_dev.count("\n") == 6
