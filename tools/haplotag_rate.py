"""What `--phase-vcf` costs on the files path beside `--phased` (FASTA + BAM through the product CLI, reads extracted on the
device): the world of tools/files_ab.py with phased SNVs planted (synth.snv_world), written twice - untagged, and with its true
HP / PS tags (synth.phase_world, no read left out) - and scored with `--phase-vcf` on the untagged files and with `--phased` on
the tagged ones, the two alternating, every run a warm process of its own.
  python tools/haplotag_rate.py [n_loci] [--repeats R] [--reads N] [--profile]
Prints per run: loci/s (best of three in the process) and the table's hash; then the medians, the spreads and whether the two
tables are equal.  --profile: one more process of each kind under `rocprofv3 --kernel-trace --stats` (no counters), and the
times of the extraction kernels from its statistics.  A child (`--child MODE FA BAM BED VCF`) is one such process."""
import contextlib
import csv
import hashlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("bam_chop_tagged_kernel", "bam_chop_ops_kernel", "bam_haplotag_kernel", "bam_select_kernel", "bgzf_inflate_kernel")


def child(mode, fa, bam, bed, vcf):
    sys.path.insert(0, HERE)
    from vapor_amd import cli
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "o.vapor")
    args = ["bed", "--sv-input", bed, "--reference", fa, "--pacbio-input", bam, "--output-path", tmp + "/f", "--output-file", out, "--no-figures"]
    args += ["--phase-vcf", vcf] if mode == "haplotag" else ["--phased"]
    n = sum(1 for _ in open(bed))
    times = []
    for _ in range(4):                                  # (the first is the warm-up: engines, pools, page cache, the VCF)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            rc = cli.main(args)
            times.append(time.perf_counter() - t0)
        assert rc in (0, None), rc
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    print(json.dumps({"mode": mode, "loci": n, "best_s": min(times[1:]), "runs_s": times[1:],
                      "table": hashlib.sha256(open(out, "rb").read()).hexdigest()[:16],
                      "phased_rows": sum(1 for r in rows[1:] if len(r) > 10 and r[11] != ".")}), flush=True)


def kernel_stats(directory):
    """{kernel: (calls, total ns, mean ns)} from the kernel statistics rocprofv3 wrote under `directory`."""
    out = {}
    for d, _sub, files in os.walk(directory):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                for row in csv.DictReader(open(os.path.join(d, f))):
                    name = row.get("Name", "")
                    for k in KERNELS:
                        if k in name:
                            out[k] = (int(row["Calls"]), int(row["TotalDurationNs"]), float(row["AverageNs"]))
    return out


def main():
    argv = sys.argv[1:]

    def opt(name, default=None):
        if name in argv:
            k = argv.index(name)
            v = argv[k + 1]
            del argv[k:k + 2]
            return v
        return default
    repeats = int(opt("--repeats", "5"))
    n_reads = int(opt("--reads", "20"))
    profile = "--profile" in argv
    pos = [a for a in argv if not a.startswith("--")]
    n = int(pos[0]) if pos else 2000
    sys.path.insert(0, HERE)
    import copy
    from vapor_amd import _lib, synth
    w = synth.make_world(seed=11, n_loci=n, svtypes=("DEL", "DEL", "INV", "INS"), span_range=(100, 4000), read_len=9500, n_reads=n_reads)
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    sites = synth.snv_world(w, seed=13)
    tagged = copy.copy(w)
    tagged.reads = {c: [synth.SamRecord(r.qname, r.rname, r.pos, r.cigar, r.seq, r.ref_span) for r in rs] for c, rs in w.reads.items()}
    synth.phase_world(tagged, seed=12, untagged=0.0)
    tmp = tempfile.mkdtemp()
    files = {}
    for name, world in (("haplotag", w), ("phased", tagged)):
        os.mkdir(os.path.join(tmp, name))
        files[name] = synth.write_world_files(world, os.path.join(tmp, name), block_size=0xFF00)
    bed = os.path.join(tmp, "in.bed")
    open(bed, "w").write(synth.bed_text(w))
    vcf = os.path.join(tmp, "snv.vcf")
    open(vcf, "w").write(synth.snv_vcf_text(sites))
    print("source %s; files of %d loci of %d reads: %.1f MB BAM untagged, %.1f MB tagged; %d phased SNVs; %d usable cores"
          % (_lib.load().vapor_source_id().decode(), n, n_reads, os.path.getsize(files["haplotag"][1]) / 1e6,
             os.path.getsize(files["phased"][1]) / 1e6, sum(len(v) for v in sites.values()), len(os.sched_getaffinity(0))), flush=True)

    def run(mode, wrap=()):
        env = dict(os.environ)
        env.pop("VAPOR_BAM_DEVICE", None)
        fa, bam = files[mode]
        r = subprocess.run(list(wrap) + [sys.executable, os.path.abspath(__file__), "--child", mode, fa, bam, bed, vcf], env=env, capture_output=True,
                           text=True)
        if r.returncode != 0:
            raise SystemExit("child %s failed:\n%s" % (mode, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    res = {}
    for rep in range(repeats):
        for mode in ("phased", "haplotag"):
            got = run(mode)
            res.setdefault(mode, []).append(got)
            print("repeat %d  %-8s %7.0f loci/s  (runs %s s)  table %s  phased rows %d" % (rep, mode, got["loci"] / got["best_s"],
                  " ".join("%.3f" % t for t in got["runs_s"]), got["table"], got["phased_rows"]), flush=True)
    print()
    med = {}
    for mode, runs in res.items():
        rates = sorted(g["loci"] / g["best_s"] for g in runs)
        med[mode] = rates[len(rates) // 2]
        print("%-8s loci/s over %d processes: min %.0f  median %.0f  max %.0f  (spread %.1f %% of the median)"
              % (mode, len(runs), rates[0], med[mode], rates[-1], 100.0 * (rates[-1] - rates[0]) / med[mode]))
    print("--phase-vcf / --phased: rate %.3f (medians); the two tables are equal: %s"
          % (med["haplotag"] / med["phased"], {g["table"] for g in res["haplotag"]} == {g["table"] for g in res["phased"]} and len({g["table"] for g in res["phased"]}) == 1))
    if profile:
        for mode in ("phased", "haplotag"):
            d = tempfile.mkdtemp()
            run(mode, ("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"))
            st = kernel_stats(d)
            print("rocprofv3 --kernel-trace --stats, %s: %s" % (mode, "; ".join("%s %d calls, mean %.1f us" % (k, st[k][0], st[k][2] / 1e3)
                                                                                 for k in KERNELS if k in st) or "no statistics found"))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:7])
    else:
        main()
