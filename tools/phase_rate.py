"""What `--phased` costs on the files path (FASTA + BAM through the product CLI, reads extracted on the device): the world of
tools/files_ab.py, haplotagged (synth.phase_world), scored unphased and phased, each run in a warm process of its own; with
--parent DIR the unphased run of another checkout (the parent commit, built) alternates with this one's, so that the spread
between one build's own repeats can be read beside the difference between the builds.
  python tools/phase_rate.py [n_loci] [--qual] [--repeats R] [--parent DIR] [--reads N]
(--qual: seeded qualities instead of 0xFF; --reads: reads per locus, 20 in that world - with no more than the cap of 20 the three
lists' union is list A itself, with more it grows towards 60)
Prints per run: loci/s (best of three in the process), the table's hash, reads scored per locus, bytes the last extraction call
copied back from the device; then the summary.  A child (`--child ROOT MODE FA BAM BED`) is one such process, importing
vapor_amd from ROOT."""
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
    from vapor_amd import cli, fastpath, pipeline
    scored = [0, 0]                                     # reads, loci handed to the scoring plan
    real = fastpath._score

    def spy(engine, ss, loc, sc, rd_first, kfl, *a, **k):
        scored[0] += sum(kfl[loc[q][0] + 1] - kfl[loc[q][0]] for q, _k in sc)
        scored[1] += len(sc)
        return real(engine, ss, loc, sc, rd_first, kfl, *a, **k)
    fastpath._score = spy
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "o.vapor")
    args = ["bed", "--sv-input", bed, "--reference", fa, "--pacbio-input", bam, "--output-path", tmp + "/f", "--output-file", out, "--no-figures"]
    if mode == "phased":
        args.append("--phased")
    n = sum(1 for _ in open(bed))
    times = []
    for _ in range(4):                                  # (the first is the warm-up: engines, pools, page cache)
        scored[0] = scored[1] = 0
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            rc = cli.main(args)
            times.append(time.perf_counter() - t0)
        assert rc in (0, None), rc
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    first10 = "\n".join("\t".join(r[:10]) for r in rows) + "\n"
    d2h = -1
    try:
        d2h = pipeline.engine_slot(0).bam_last_stats().get("d2h_bytes", -1)
    except Exception:                                   # noqa: BLE001 - a checkout without the figure
        pass
    print(json.dumps({"mode": mode, "loci": n, "best_s": min(times[1:]), "runs_s": times[1:], "table": hashlib.sha256(open(out, "rb").read()).hexdigest()[:16],
                      "first10": hashlib.sha256(first10.encode()).hexdigest()[:16], "reads_scored": scored[0], "loci_scored": scored[1],
                      "d2h_bytes_last_call": d2h, "phased_rows": sum(1 for r in rows[1:] if len(r) > 10 and r[11] != ".")}), flush=True)


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
    parent = opt("--parent")
    n_reads = int(opt("--reads", "20"))
    qual = "--qual" in argv
    pos = [a for a in argv if not a.startswith("--")]
    n = int(pos[0]) if pos else 2000
    sys.path.insert(0, HERE)
    from vapor_amd import _lib, synth
    w = synth.make_world(seed=11, n_loci=n, svtypes=("DEL", "DEL", "INV", "INS"), span_range=(100, 4000), read_len=9500, n_reads=n_reads)
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    synth.phase_world(w, seed=12)
    tmp = tempfile.mkdtemp()
    fa, bam = synth.write_world_files(w, tmp, block_size=0xFF00, qual_seed=(7 if qual else None))
    bed = os.path.join(tmp, "in.bed")
    open(bed, "w").write(synth.bed_text(w))
    print("source %s; files of %d loci of %d reads, haplotagged: %.1f MB BAM, %s qualities, %d usable cores"
          % (_lib.load().vapor_source_id().decode(), n, n_reads, os.path.getsize(bam) / 1e6, "seeded" if qual else "absent", len(os.sched_getaffinity(0))), flush=True)

    def run(root, mode):
        env = dict(os.environ)
        env.pop("VAPOR_BAM_DEVICE", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, mode, fa, bam, bed], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("child %s %s failed:\n%s" % (root, mode, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    res = {}
    order = ([("parent", parent, "unphased")] if parent else []) + [("this", HERE, "unphased"), ("this", HERE, "phased")]
    for rep in range(repeats):
        for who, root, mode in order:
            got = run(root, mode)
            res.setdefault((who, mode), []).append(got)
            print("repeat %d  %-6s %-8s %7.0f loci/s  (runs %s s)  table %s  first ten columns %s  %.1f reads scored per locus (%d loci)  d2h of the last call %d B"
                  % (rep, who, mode, got["loci"] / got["best_s"], " ".join("%.3f" % t for t in got["runs_s"]), got["table"], got["first10"],
                     got["reads_scored"] / max(got["loci_scored"], 1), got["loci_scored"], got["d2h_bytes_last_call"]), flush=True)
    print()
    for key, runs in res.items():
        rates = sorted(g["loci"] / g["best_s"] for g in runs)
        print("%-6s %-8s loci/s over %d processes: min %.0f  median %.0f  max %.0f  (spread %.1f %% of the median)"
              % (key[0], key[1], len(runs), rates[0], rates[len(rates) // 2], rates[-1], 100.0 * (rates[-1] - rates[0]) / rates[len(rates) // 2]))
    un, ph = res[("this", "unphased")], res[("this", "phased")]
    med = lambda runs: sorted(g["loci"] / g["best_s"] for g in runs)[len(runs) // 2]      # noqa: E731
    print("phased / unphased: rate %.2f, reads scored %.2f; the phased table's first ten columns are the unphased table: %s; phased rows %d of %d"
          % (med(ph) / med(un), (ph[0]["reads_scored"] / max(ph[0]["loci_scored"], 1)) / (un[0]["reads_scored"] / max(un[0]["loci_scored"], 1)),
             {g["first10"] for g in ph} == {g["table"] for g in un} or {g["first10"] for g in ph} == {g["first10"] for g in un}, ph[0]["phased_rows"], n))
    if parent:
        pa = res[("parent", "unphased")]
        print("this / parent, unphased: %.3f (medians); tables equal: %s" % (med(un) / med(pa), {g["table"] for g in un} == {g["table"] for g in pa}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:7])
    else:
        main()
