"""What `--realign` costs on the files path: tools/evidence_rate.py's runs for its mode `ra` - one make_support_world written to
files, `vapor bed` and `vapor bed --realign` of this tree alternating, each in a warm process of its own, with --parent DIR the
plain run of another checkout (the parent commit, built; it has no `--realign`) in turn with them.
  python tools/realign_rate.py [n_loci] [--repeats R] [--parent DIR] [--bed-repeat K] [--layers N] [--timeout S] [--kernel-only]
  python tools/realign_rate.py --kernels DIR
--kernel-only: this tree's `--realign` run once, in this process - the program of a kernel trace, a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/realign_rate.py 120 --bed-repeat 4 --kernel-only
--kernels DIR: reads that trace's *kernel_stats.csv and prints realign_kernel's launches, its time per launch and its share of
the run's kernel time.
`--realign-out` has a leg of its own:
  python tools/realign_rate.py --trace [n_loci] [--repeats R] [--parent DIR] [--bed-repeat K] [--layers N] [--timeout S] [--kernel-only]
the plain run and the `--realign` run of the parent checkout (which has `--realign`) and of this tree, and this tree's
`--realign --realign-out` run, alternating, each in a warm process of its own: the two trees' tables must be equal leg for leg,
the `--realign-out` run's table the `--realign` run's; its rate is printed relative to `--realign` alone, with the seconds the
writer's close takes.  --kernel-only: the `--realign-out` run once, in this process, for a kernel trace of its own; --kernels DIR
prints the two trace kernels beside realign_kernel when the trace holds them.
`--realign-polish` likewise:
  python tools/realign_rate.py --polish [n_loci] [--repeats R] [--parent DIR] [--bed-repeat K] [--layers N] [--timeout S]
                               [--kernel-only [--kernel-leg plain|ra|pol]]
the same legs with this tree's `--realign --realign-polish` run in place of the `--realign-out` run; its table must be the
`--realign` run's in the leading columns.  --kernel-only runs one leg once (`pol` unless --kernel-leg names another), and
--kernels DIR also prints the four polish kernels and a digest of (kernel, launches) over the whole trace, by which two trees'
`--realign` runs are seen to launch the same kernels.
`--realign-junction` likewise:
  python tools/realign_rate.py --junction [n_loci] [--repeats R] [--parent DIR] [--bed-repeat K] [--layers N] [--timeout S]
                                 [--kernel-only [--kernel-leg plain|ra|pol|jun]]
the plain, `--realign` and `--realign --realign-polish` runs of the parent checkout (which has all three) and of this tree, and
this tree's `--realign --realign-polish --realign-junction` run; its table must be the `--realign-polish` run's in the leading
columns.  --kernels DIR also prints the two junction kernels.
`--realign-revote` likewise:
  python tools/realign_rate.py --revote [n_loci] [--repeats R] [--parent DIR] [--bed-repeat K] [--layers N] [--timeout S]
                               [--kernel-only [--kernel-leg plain|ra|pol|rev]]
the same three shared legs and this tree's `--realign --realign-polish --realign-revote` run; its table must be the
`--realign-polish` run's in the leading columns.  The run's process also times polish.apply - the host's spelling, which the
device's replaces - over the loci of its last run, on the calls the device gave.  --kernels DIR also prints the three re-vote
kernels.
  python tools/realign_rate.py --junction-call [pairs] [rows] [band]
one Engine.realign_junction call (wall time with its copies, best of three) of `pairs` pairs of `rows` rows, the longer
sequence carrying a jump of 300 symbols, beside DESIGN.md 4.23's arithmetic for its 2 * pairs wavefronts."""
import contextlib
import csv
import glob
import hashlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evidence_rate  # noqa: E402


def kernels(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % d)
    rows = list(csv.DictReader(open(files[-1])))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print("kernel trace %s: %d kernels, %.3f ms of kernel time" % (os.path.basename(files[-1]), len(rows), total / 1e6))
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]:
        name = r["Name"].split("(")[0]
        print("  %-60s %6d launches  %10.1f us a launch  (min %.1f, max %.1f)  %5.1f %% of the kernel time"
              % (name[:60], int(r["Calls"]), float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3, float(r.get("MinNs") or 0) / 1e3,
                 float(r.get("MaxNs") or 0) / 1e3, 100.0 * float(r["TotalDurationNs"]) / total))
    mine = [r for r in rows if "realign_kernel" in r["Name"]]
    if not mine:
        raise SystemExit("the trace holds no realign_kernel")
    t = sum(float(r["TotalDurationNs"]) for r in mine)
    n = sum(int(r["Calls"]) for r in mine)
    print("realign_kernel: %d launches, %.1f us a launch, %.1f %% of the run's kernel time" % (n, t / n / 1e3, 100.0 * t / total))
    digest = hashlib.sha256("\n".join(sorted("%s %d" % (r["Name"], int(r["Calls"])) for r in rows)).encode()).hexdigest()[:16]
    print("launches: %d in all, digest of (kernel, launches) %s" % (sum(int(r["Calls"]) for r in rows), digest))
    for name in ("realign_trace_kernel", "traceback_kernel", "pileup_kernel", "consensus_kernel", "pileup_ins_kernel", "insert_kernel", "junction_rows_kernel",
                 "junction_pick_kernel", "spell_kernel", "spell_pack_kernel", "realign_onto_kernel"):
        mine = [r for r in rows if name in r["Name"]]
        if mine:
            t = sum(float(r["TotalDurationNs"]) for r in mine)
            n = sum(int(r["Calls"]) for r in mine)
            print("%s: %d launches, %.1f us a launch, %.1f %% of the run's kernel time" % (name, n, t / n / 1e3, 100.0 * t / total))


LEGS = {"plain": [], "ra": ["--realign"], "out": ["--realign", "--realign-out"], "pol": ["--realign", "--realign-polish"],
        "jun": ["--realign", "--realign-polish", "--realign-junction"], "rev": ["--realign", "--realign-polish", "--realign-revote"]}
TAIL = {"pol": 6, "jun": 6, "rev": 8}      # the columns a leg appends to the table of the leg before it


def trace_child(root, leg, fa, bam, bed, runs=4):
    """One process of the `--trace` leg: `vapor bed` with the leg's options, `runs` times (the first is the warm-up)."""
    sys.path.insert(0, root)
    from vapor_amd import cli
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "o.vapor")
    args = ["bed", "--sv-input", bed, "--reference", fa, "--pacbio-input", bam, "--output-path", tmp + "/f", "--output-file", out, "--no-figures"]
    args += LEGS[leg] + ([os.path.join(tmp, "traces")] if leg == "out" else [])
    close_s = []
    if leg == "out":
        from vapor_amd import realign
        orig = realign.TraceWriter.close

        def timed(self):
            t0 = time.perf_counter()
            try:
                return orig(self)
            finally:
                close_s.append(time.perf_counter() - t0)
        realign.TraceWriter.close = timed
    spelt = []                             # (`rev`: what every Engine.realign_revote call of a run gave, for the host's spelling below)
    if leg == "rev":
        from vapor_amd.engine import Engine
        orig_revote = Engine.realign_revote

        def kept(self, ss, pairs, band, first, col_off, *more, **kw):
            got = orig_revote(self, ss, pairs, band, first, col_off, *more, **kw)
            spelt.append((list(col_off), got[1], got[2], got[3]))
            return got
        Engine.realign_revote = kept
    times = []
    for _ in range(int(runs)):
        del spelt[:]
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            rc = cli.main(args)
            times.append(time.perf_counter() - t0)
        assert rc in (0, None), rc
    got = {"loci": sum(1 for _ in open(bed)), "best_s": min(times[1:] or times), "runs_s": times[1:] or times,
           "table": hashlib.sha256(open(out, "rb").read()).hexdigest()[:16]}
    if leg in TAIL:                        # (the table without the leg's own columns: the run's before it, byte for byte)
        lead = "".join("\t".join(ln.rstrip("\n").split("\t")[:-TAIL[leg]]) + "\n" for ln in open(out))
        got["lead"] = hashlib.sha256(lead.encode()).hexdigest()[:16]
    if leg == "rev":                       # (polish.apply over the last run's loci, on texts of the alleles' lengths: best of three)
        from vapor_amd import polish
        best, n_loci, n_cols = None, 0, 0
        for _ in range(3):
            t0 = time.perf_counter()
            n_loci = n_cols = 0
            for col_off, calls, sites, ins in spelt:
                for g in range(len(col_off) - 1):
                    polish.apply("A" * (col_off[g + 1] - col_off[g]), calls[col_off[g]:col_off[g + 1]], sites[g], ins[g])
                    n_loci += 1
                    n_cols += col_off[g + 1] - col_off[g]
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        got.update(apply_s=best, apply_loci=n_loci, apply_cols=n_cols)
    if leg == "out":
        sam = os.path.join(tmp, "traces.sam")
        got.update(close_s=min(close_s[1:] or close_s), sam_mb=os.path.getsize(sam) / 1e6,
                   records=sum(1 for ln in open(sam) if not ln.startswith("@")))
    print(json.dumps(got), flush=True)


def trace_main(argv, last="out"):
    def opt(name, default=None):
        if name in argv:
            k = argv.index(name)
            v = argv[k + 1]
            del argv[k:k + 2]
            return v
        return default
    repeats, bed_repeat, layers = int(opt("--repeats", "4")), int(opt("--bed-repeat", "1")), int(opt("--layers", "4"))
    limit, parent = float(opt("--timeout", "240")), opt("--parent")
    kernel_only, kernel_leg = "--kernel-only" in argv, opt("--kernel-leg", last)
    pos = [a for a in argv if not a.startswith("--")]
    n = int(pos[0]) if pos else 120
    here = evidence_rate.HERE
    sys.path.insert(0, here)
    from vapor_amd import _lib, synth
    w, what = evidence_rate.MODES["ra"][0](synth, n, {"layers": layers, "reads": 8})
    d = tempfile.mkdtemp()
    fa, bam = synth.write_world_files(w, d, block_size=0xFF00)
    bed = os.path.join(d, "in.bed")
    open(bed, "w").write(synth.bed_text(w) * bed_repeat)
    print("source %s; files of %d %s, the BED file %d times over: %.1f MB BAM" % (_lib.load().vapor_source_id().decode(), n, what, bed_repeat,
                                                                                 os.path.getsize(bam) / 1e6), flush=True)
    if kernel_only:
        trace_child(here, kernel_leg, fa, bam, bed, runs=1)
        return

    def run(root, leg):
        env = dict(os.environ)
        env.pop("VAPOR_BAM_DEVICE", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", root, leg, fa, bam, bed], env=env, capture_output=True,
                           text=True, timeout=limit)
        if r.returncode != 0:
            raise SystemExit("child %s %s failed:\n%s" % (root, leg, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    shared = ("plain", "ra", "pol") if last in ("jun", "rev") else ("plain", "ra")      # (the legs the parent has too)
    order = ([("parent", parent, leg) for leg in shared] if parent else []) + [("this", here, leg) for leg in shared + (last,)]
    res = {}
    for rep in range(repeats):
        for who, root, leg in order:
            got = run(root, leg)
            res.setdefault((who, leg), []).append(got)
            more = "  close %.4f s, %d records, %.1f MB of SAM" % (got["close_s"], got["records"], got["sam_mb"]) if leg == "out" else ""
            print("repeat %d  %-6s %-5s %7.0f loci/s  (runs %s s)  table %s%s"
                  % (rep, who, leg, got["loci"] / got["best_s"], " ".join("%.3f" % t for t in got["runs_s"]), got["table"], more), flush=True)
    print()
    rates = lambda runs: sorted(g["loci"] / g["best_s"] for g in runs)         # noqa: E731
    med = lambda runs: rates(runs)[len(runs) // 2]                              # noqa: E731
    for (who, leg), runs in res.items():
        r = rates(runs)
        print("%-6s %-5s loci/s over %d processes: min %.0f  median %.0f  max %.0f" % (who, leg, len(runs), r[0], med(runs), r[-1]))
    ra, out = res[("this", "ra")], res[("this", last)]
    if last == "out":
        print("--realign-out / --realign: rate %.3f (medians); tables equal: %s; the writer's close is %.1f %% of the run"
              % (med(out) / med(ra), {g["table"] for g in out} == {g["table"] for g in ra},
                 100.0 * min(g["close_s"] for g in out) / min(g["best_s"] for g in out)))
    elif last == "rev":
        pol = res[("this", "pol")]
        print("--realign-revote / --realign-polish: rate %.3f (medians); the leading columns equal --realign-polish's table: %s"
              % (med(out) / med(pol), {g["lead"] for g in out} == {g["table"] for g in pol}))
        g = min(out, key=lambda g: g["apply_s"])
        print("polish.apply on this host over the run's %d loci (%d columns): %.4f s, %.3f ms a locus - %.1f %% of the --realign-revote run"
              % (g["apply_loci"], g["apply_cols"], g["apply_s"], 1e3 * g["apply_s"] / max(g["apply_loci"], 1), 100.0 * g["apply_s"] / g["best_s"]))
    elif last == "jun":
        pol = res[("this", "pol")]
        print("--realign-junction / --realign-polish: rate %.3f (medians); the leading columns equal --realign-polish's table: %s"
              % (med(out) / med(pol), {g["lead"] for g in out} == {g["table"] for g in pol}))
    else:
        print("--realign-polish / --realign: rate %.3f (medians); the leading columns equal --realign's table: %s"
              % (med(out) / med(ra), {g["lead"] for g in out} == {g["table"] for g in ra}))
    if parent:
        for leg in shared:
            pa, mine = res[("parent", leg)], res[("this", leg)]
            rp = rates(pa)
            print("this / parent, %-5s: %.3f (medians); tables equal: %s; %d of this tree's %d runs below the parent's minimum (%.0f)"
                  % (leg, med(mine) / med(pa), {g["table"] for g in mine} == {g["table"] for g in pa},
                     sum(1 for v in rates(mine) if v < rp[0]), len(mine), rp[0]))
        print("%s against the parent's --realign: rate %.3f (medians)" % (" ".join(LEGS[last][1:]), med(out) / med(res[("parent", "ra")])))


def junction_call(argv):
    """One Engine.realign_junction call of P pairs of r rows at a band, best of three, beside 2 P r 4 (5 S + 45) SIMD cycles."""
    import numpy as np
    sys.path.insert(0, evidence_rate.HERE)
    from vapor_amd.engine import Engine
    pairs, rows, band = (int(v) for v in (argv + ["4096", "10000", "256"][len(argv):])[:3])
    rng = np.random.default_rng(1)
    n_seq = 64                                                     # (distinct sequences; the pairs go round them)
    seqs = []
    for _ in range(n_seq):
        l = "".join("ACGT"[j] for j in rng.integers(0, 4, rows + 300))
        seqs += [l[:rows // 2] + l[rows // 2 + 300:], l]
    S = next(w for w in (1, 2, 3, 5, 9, 17) if 64 * w >= 2 * band + 1)
    e = Engine(0)
    try:
        e.set_param("trace_budget", 16 * (rows + 1) * pairs + (1 << 20))      # (the tables of the call: 655 MB at the default shape)
        ss = e.seqset(seqs)
        tab = e.make_pairs([(2 * (t % n_seq), 2 * (t % n_seq) + 1, 0, 0, 0) for t in range(pairs)])
        times = []
        for _ in range(4):
            t0 = time.perf_counter()
            out, _o, _r = e.realign_junction(ss, tab, band)
            times.append(time.perf_counter() - t0)
        assert out[:, 0].tolist() == [0] * pairs and set((out[:, 4] - out[:, 3]).tolist()) == {300} and not out[:, 1].any()
        ss.close()
    finally:
        e.close()
    stated = 2.0 * pairs * rows * 4 * (5 * S + 45) / (1024 * 2.4e9)
    best = min(times[1:])
    print("realign_junction: %d pairs of %d rows at band %d (S = %d): %.2f ms (best of three; %s), stated %.2f ms, measured / stated %.2f"
          % (pairs, rows, band, S, best * 1e3, " ".join("%.2f" % (t * 1e3) for t in times[1:]), stated * 1e3, best / stated), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        kernels(sys.argv[2])
    elif len(sys.argv) > 1 and sys.argv[1] == "--trace-child":
        trace_child(*sys.argv[2:7])
    elif len(sys.argv) > 1 and sys.argv[1] == "--trace":
        trace_main(sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "--polish":
        trace_main(sys.argv[2:], "pol")
    elif len(sys.argv) > 1 and sys.argv[1] == "--junction":
        trace_main(sys.argv[2:], "jun")
    elif len(sys.argv) > 1 and sys.argv[1] == "--revote":
        trace_main(sys.argv[2:], "rev")
    elif len(sys.argv) > 1 and sys.argv[1] == "--junction-call":
        junction_call(sys.argv[2:])
    else:
        sys.argv.insert(1, "ra")
        evidence_rate.main()
