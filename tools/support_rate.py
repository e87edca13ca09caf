"""What `--support` costs on the files path (FASTA + BAM through the product CLI): one synth.make_support_world - contigs tiled with
reads, het, hom and ref DEL, TANDUP, INV and INS loci of stated spans below and above 10 kb, their alt reads aligned with D, I and
split records, one spanner a layer and reference haplotype at every breakpoint - written to files, and runs alternating, each in a
warm process of its own: with --parent DIR the plain run of another checkout (the parent commit, built), this tree's plain run,
this tree's run with --support.  The spread between one build's own repeats can then be read beside the difference between the
builds; the five columns of the --support run's rows must be the plain run's.
  python tools/support_rate.py [n_loci] [--repeats R] [--parent DIR] [--bed-repeat K] [--layers N] [--sup-repeats F] [--kernel-only]
(--bed-repeat K: the same loci K times over in the BED file; --sup-repeats F: the --support run only in the first F repeats, it is
informational; --kernel-only: this tree's --support run once, in this process - for a kernel trace of bam_support_kernel)
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
SPANS = (300, 700, 1500, 4000, 900, 2500, 12000, 24000, 600, 15000)
TYPES = ("DEL", "TANDUP", "INV", "INS", "DEL", "TANDUP", "DEL")
ZYG = ("het", "hom", "ref")


def child(root, mode, fa, bam, bed, runs=4):
    sys.path.insert(0, root)
    from vapor_amd import cli
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "o.vapor")
    args = ["bed", "--sv-input", bed, "--reference", fa, "--pacbio-input", bam, "--output-path", tmp + "/f", "--output-file", out, "--no-figures"]
    if mode == "sup":
        args += ["--support"]
    n = sum(1 for _ in open(bed))
    times = []
    for _ in range(runs):                               # (the first is the warm-up: engines, pools, page cache)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            rc = cli.main(args)
            times.append(time.perf_counter() - t0)
        assert rc in (0, None), rc
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    own = "\n".join("\t".join(r[:-9] if mode == "sup" else r) for r in rows)
    measured = sum(1 for r in rows[1:] if mode == "sup" and r[-9] != ".")
    gts = {}
    for r in rows[1:]:
        if mode == "sup":
            gts[r[-2]] = gts.get(r[-2], 0) + 1
    print(json.dumps({"mode": mode, "loci": n, "best_s": min(times[1:] or times), "runs_s": times[1:] or times, "measured": measured, "gts": gts,
                      "table": hashlib.sha256(own.encode()).hexdigest()[:16]}), flush=True)


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
    sup_repeats = int(opt("--sup-repeats", "1000"))
    layers = int(opt("--layers", "4"))
    parent = opt("--parent")
    kernel_only = "--kernel-only" in argv
    pos = [a for a in argv if not a.startswith("--")]
    n = int(pos[0]) if pos else 200
    sys.path.insert(0, HERE)
    from vapor_amd import _lib, synth
    specs = [(TYPES[i % len(TYPES)], SPANS[i % len(SPANS)], ZYG[(i // 2) % 3]) for i in range(n)]
    w = synth.make_support_world(seed=17, specs=specs, layers=layers, read_len=6000)
    d = tempfile.mkdtemp()
    fa, bam = synth.write_world_files(w, d, block_size=0xFF00)
    bed = os.path.join(d, "in.bed")
    open(bed, "w").write(synth.bed_text(w) * bed_repeat)
    print("source %s; files of %d DEL / TANDUP / INV / INS loci (spans %d .. %d; het, hom, ref) at depth %d, the BED file %d times over: %.1f MB BAM, %d usable cores"
          % (_lib.load().vapor_source_id().decode(), n, min(SPANS), max(SPANS), 2 * layers, bed_repeat, os.path.getsize(bam) / 1e6,
             len(os.sched_getaffinity(0))), flush=True)
    if kernel_only:
        child(HERE, "sup", fa, bam, bed, runs=1)
        return

    def run(root, mode):
        env = dict(os.environ)
        env.pop("VAPOR_BAM_DEVICE", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, mode, fa, bam, bed], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("child %s %s failed:\n%s" % (root, mode, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    res = {}
    order = ([("parent", parent, "plain")] if parent else []) + [("this", HERE, "plain"), ("this", HERE, "sup")]
    for rep in range(repeats):
        for who, root, mode in order:
            if mode == "sup" and rep >= sup_repeats:
                continue
            got = run(root, mode)
            res.setdefault((who, mode), []).append(got)
            print("repeat %d  %-6s %-6s %7.0f loci/s  (runs %s s)  own columns %s%s"
                  % (rep, who, mode, got["loci"] / got["best_s"], " ".join("%.3f" % t for t in got["runs_s"]), got["table"],
                     "  measured %d, genotypes %s" % (got["measured"], " ".join("%s: %d" % kv for kv in sorted(got["gts"].items()))) if mode == "sup" else ""),
                  flush=True)
    print()
    for key, runs in res.items():
        rates = sorted(g["loci"] / g["best_s"] for g in runs)
        print("%-6s %-6s loci/s over %d processes: min %.0f  median %.0f  max %.0f  (spread %.1f %% of the median)"
              % (key[0], key[1], len(runs), rates[0], rates[len(rates) // 2], rates[-1], 100.0 * (rates[-1] - rates[0]) / rates[len(rates) // 2]))
    med = lambda runs: sorted(g["loci"] / g["best_s"] for g in runs)[len(runs) // 2]      # noqa: E731
    pl, dp = res[("this", "plain")], res[("this", "sup")]
    print("--support / plain: rate %.2f (medians); the rows' own columns equal: %s"
          % (med(dp) / med(pl), {g["table"] for g in dp} == {g["table"] for g in pl}))
    if parent:
        pa = res[("parent", "plain")]
        rp = sorted(g["loci"] / g["best_s"] for g in pa)
        inside = sum(1 for g in pl if rp[0] <= g["loci"] / g["best_s"] <= rp[-1])
        below = sum(1 for g in pl if g["loci"] / g["best_s"] < rp[0])
        print("this / parent, plain: %.3f (medians); tables equal: %s; %d of this tree's %d runs lie inside the parent's own spread (%.0f .. %.0f), %d below its minimum"
              % (med(pl) / med(pa), {g["table"] for g in pl} == {g["table"] for g in pa}, inside, len(pl), rp[0], rp[-1], below))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:7])
    else:
        main()
