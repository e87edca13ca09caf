"""What `--dedup-qname` costs on the files path (FASTA + BAM through the product CLI, reads extracted on the device): a world of
long DEL and TANDUP loci whose junction molecules are written as split alignments (synth.add_split_alignments: a primary record
and a supplementary one with the whole SEQ at the far breakpoint, window-internal secondary twins at the TANDUPs), and
`vapor bed --both-ends` on it in runs that alternate, each in a warm process of its own: with --parent DIR the plain run of
another checkout (the parent commit, built), this tree's plain run, this tree's run with --dedup-qname.  The plain runs launch
the same kernels in both trees; the run with the option adds bam_dedup_kernel behind every chop kernel and the keys' way back.
The ratio of the two rates of this tree is informational and carries no threshold.
  python tools/dedup_rate.py [n_loci] [--repeats R] [--parent DIR] [--bed-repeat K]
A child (`--child ROOT MODE FA BAM BED`) is one such process, importing vapor_amd from ROOT."""
import contextlib
import hashlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(root, mode, fa, bam, bed):
    sys.path.insert(0, root)
    from vapor_amd import cli
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "o.vapor")
    args = ["bed", "--sv-input", bed, "--reference", fa, "--pacbio-input", bam, "--output-path", tmp + "/f", "--output-file", out, "--no-figures",
            "--both-ends"]
    if mode == "dedup":
        args += ["--dedup-qname"]
    n = sum(1 for _ in open(bed))
    times = []
    for _ in range(4):                                  # (the first is the warm-up: engines, pools, page cache)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            rc = cli.main(args)
            times.append(time.perf_counter() - t0)
        assert rc in (0, None), rc
    print(json.dumps({"mode": mode, "loci": n, "best_s": min(times[1:]), "runs_s": times[1:],
                      "table": hashlib.sha256(open(out, "rb").read()).hexdigest()[:16]}), flush=True)


def main():
    argv = sys.argv[1:]

    def opt(name, default=None):
        if name in argv:
            k = argv.index(name)
            v = argv[k + 1]
            del argv[k:k + 2]
            return v
        return default
    repeats = int(opt("--repeats", "4"))
    bed_repeat = int(opt("--bed-repeat", "1"))
    parent = opt("--parent")
    pos = [a for a in argv if not a.startswith("--")]
    n = int(pos[0]) if pos else 200
    sys.path.insert(0, HERE)
    from vapor_amd import _lib, synth
    base = synth.make_junction_world(17, ("DEL", "TANDUP") * (n // 2), n_reads=10, ref_fraction=0.25)
    w = synth.add_split_alignments(base, "full", window_dups=2)
    d = tempfile.mkdtemp()
    fa, bam = synth.write_world_files(w, d, block_size=0xFF00)
    bed = os.path.join(d, "in.bed")
    open(bed, "w").write(synth.bed_text(w) * bed_repeat)
    print("source %s; %d loci (long DEL and TANDUP, 10 reads a junction side), the BED file %d times over; %d supplementary and %d "
          "secondary records planted; %.1f MB BAM; %d usable cores"
          % (_lib.load().vapor_source_id().decode(), len(w.loci), bed_repeat, w.planted["split"], w.planted["window"],
             os.path.getsize(bam) / 1e6, len(os.sched_getaffinity(0))), flush=True)

    def run(root, mode):
        env = dict(os.environ)
        env.pop("VAPOR_BAM_DEVICE", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, mode, fa, bam, bed], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("child %s %s failed:\n%s" % (root, mode, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    res = {}
    order = ([("parent", parent, "plain")] if parent else []) + [("this", HERE, "plain"), ("this", HERE, "dedup")]
    for rep in range(repeats):
        for who, root, mode in order:
            got = run(root, mode)
            res.setdefault((who, mode), []).append(got)
            print("repeat %d  %-6s %-6s %7.0f loci/s  (runs %s s)  table %s"
                  % (rep, who, mode, got["loci"] / got["best_s"], " ".join("%.3f" % t for t in got["runs_s"]), got["table"]), flush=True)
    print()
    for key, runs in res.items():
        rates = sorted(g["loci"] / g["best_s"] for g in runs)
        print("%-6s %-6s loci/s over %d processes: min %.0f  median %.0f  max %.0f  (spread %.1f %% of the median)"
              % (key[0], key[1], len(runs), rates[0], rates[len(rates) // 2], rates[-1], 100.0 * (rates[-1] - rates[0]) / rates[len(rates) // 2]))
    med = lambda runs: sorted(g["loci"] / g["best_s"] for g in runs)[len(runs) // 2]      # noqa: E731
    pl, dd = res[("this", "plain")], res[("this", "dedup")]
    print("--dedup-qname / plain, both --both-ends on the same files: rate %.2f (medians); the tables differ: %s"
          % (med(dd) / med(pl), {g["table"] for g in dd} != {g["table"] for g in pl}))
    if parent:
        pa = res[("parent", "plain")]
        rp = sorted(g["loci"] / g["best_s"] for g in pa)
        inside = sum(1 for g in pl if rp[0] <= g["loci"] / g["best_s"] <= rp[-1])
        print("this / parent, plain: %.3f (medians); tables equal: %s; %d of this tree's %d runs lie inside the parent's own spread (%.0f .. %.0f)"
              % (med(pl) / med(pa), {g["table"] for g in pl} == {g["table"] for g in pa}, inside, len(pl), rp[0], rp[-1]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:7])
    else:
        main()
