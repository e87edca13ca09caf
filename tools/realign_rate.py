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
`--realign` runs are seen to launch the same kernels."""
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
    for name in ("realign_trace_kernel", "traceback_kernel", "pileup_kernel", "consensus_kernel", "pileup_ins_kernel", "insert_kernel"):
        mine = [r for r in rows if name in r["Name"]]
        if mine:
            t = sum(float(r["TotalDurationNs"]) for r in mine)
            n = sum(int(r["Calls"]) for r in mine)
            print("%s: %d launches, %.1f us a launch, %.1f %% of the run's kernel time" % (name, n, t / n / 1e3, 100.0 * t / total))


LEGS = {"plain": [], "ra": ["--realign"], "out": ["--realign", "--realign-out"], "pol": ["--realign", "--realign-polish"]}


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
    times = []
    for _ in range(int(runs)):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            rc = cli.main(args)
            times.append(time.perf_counter() - t0)
        assert rc in (0, None), rc
    got = {"loci": sum(1 for _ in open(bed)), "best_s": min(times[1:] or times), "runs_s": times[1:] or times,
           "table": hashlib.sha256(open(out, "rb").read()).hexdigest()[:16]}
    if leg == "pol":                       # (the table without its last six columns: --realign's, byte for byte)
        lead = "".join("\t".join(ln.rstrip("\n").split("\t")[:-6]) + "\n" for ln in open(out))
        got["lead"] = hashlib.sha256(lead.encode()).hexdigest()[:16]
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
    order = ([("parent", parent, "plain"), ("parent", parent, "ra")] if parent else []) + [("this", here, leg) for leg in ("plain", "ra", last)]
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
    else:
        print("--realign-polish / --realign: rate %.3f (medians); the leading columns equal --realign's table: %s"
              % (med(out) / med(ra), {g["lead"] for g in out} == {g["table"] for g in ra}))
    if parent:
        for leg in ("plain", "ra"):
            pa, mine = res[("parent", leg)], res[("this", leg)]
            rp = rates(pa)
            print("this / parent, %-5s: %.3f (medians); tables equal: %s; %d of this tree's %d runs below the parent's minimum (%.0f)"
                  % (leg, med(mine) / med(pa), {g["table"] for g in mine} == {g["table"] for g in pa},
                     sum(1 for v in rates(mine) if v < rp[0]), len(mine), rp[0]))
        print("%s against the parent's --realign: rate %.3f (medians)" % (" ".join(LEGS[last][1:]), med(out) / med(res[("parent", "ra")])))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        kernels(sys.argv[2])
    elif len(sys.argv) > 1 and sys.argv[1] == "--trace-child":
        trace_child(*sys.argv[2:7])
    elif len(sys.argv) > 1 and sys.argv[1] == "--trace":
        trace_main(sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "--polish":
        trace_main(sys.argv[2:], "pol")
    else:
        sys.argv.insert(1, "ra")
        evidence_rate.main()
