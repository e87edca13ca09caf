"""What `--both-ends` costs on the files path (FASTA + BAM through the product CLI): one world of long DEL loci read from both
sides of their junction (synth.make_junction_world) and of breakend loci of every form (synth.make_bnd_world), scored by
`vapor vcf --bnd` and by `vapor vcf --bnd --both-ends`, each run in a warm process of its own, the processes alternating; with
--parent DIR the plain `--bnd` run of another checkout (the parent commit, built) alternates with them, so that the spread between
one build's own repeats can be read beside the difference between the builds.
  python tools/both_ends_rate.py [n_del] [n_bnd] [--repeats R] [--parent DIR] [--out FILE]
Prints per run: loci/s and views/s (best of three in the process), the table's hash, what the process's last device extraction
call did (vapor_bam_last_stats); then the summary.  A child (`--child ROOT MODE FA BAM VCF`) is one such process, importing
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


def child(root, mode, fa, bam, vcf):
    sys.path.insert(0, root)
    from vapor_amd import cli, pipeline
    args = ["vcf", "--sv-input", vcf, "--reference", fa, "--pacbio-input", bam, "--output-path", tempfile.mkdtemp() + "/f", "--output-file", "unused",
            "--no-figures", "--bnd"]
    if mode == "both":
        args.append("--both-ends")
    times = []
    for _ in range(4):                                  # (the first is the warm-up: engines, pools, page cache)
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            t0 = time.perf_counter()
            rc = cli.main(args)
            times.append(time.perf_counter() - t0)
        assert rc in (0, None), rc
    # (cli.main rewrites <vcf>.vapor as the annotated VCF: one record line per scored record)
    recs = [ln.split("\t") for ln in open(vcf + ".vapor").read().splitlines() if ln and not ln.startswith("#")]
    views = 0
    loci = set()
    for r in recs:
        key = r[7].split(";VaPor_GS=")[1] if ";VaPor_GS=" in r[7] else r[2]
        if key in loci:
            continue                                    # (a mate: the same locus)
        loci.add(key)
        n = [x for x in r[7].split(";") if x.startswith("VaPoR_BE_N=")]
        views += int(n[0].split("=")[1]) if n else (1 if ";VaPor_GS=" in r[7] and "VaPor_GT=NA" not in r[7] else 0)
    stats = {}
    try:
        stats = pipeline.engine_slot(0).bam_last_stats()
    except Exception:                                   # noqa: BLE001 - no device extraction in this process
        pass
    old = "\n".join(";".join(x for x in r[7].split(";") if not x.startswith("VaPoR_BE_")) for r in recs if "\t[" not in "\t".join(r))
    print(json.dumps({"mode": mode, "loci": len(loci), "views": views, "best_s": min(times[1:]), "runs_s": times[1:],
                      "table": hashlib.sha256(open(vcf + ".vapor", "rb").read()).hexdigest()[:16],
                      "old_columns": hashlib.sha256(old.encode()).hexdigest()[:16], "bam_last_stats": stats}), flush=True)


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
    out = opt("--out")
    pos = [a for a in argv if not a.startswith("--")]
    n_del = int(pos[0]) if pos else 300
    n_bnd = int(pos[1]) if len(pos) > 1 else 300
    sys.path.insert(0, HERE)
    from vapor_amd import _lib, synth
    w = synth.make_junction_world(21, svtypes=("DEL",) * n_del, n_reads=15)
    b = synth.make_bnd_world(22, forms=synth.BND_FORMS * (n_bnd // 4), n_reads=15, ins=("", "ACGTTGCA", "GGA"))
    w.contigs.update(b.contigs)
    w.reads.update(b.reads)
    simple = synth.SynthWorld()
    simple.loci = list(w.loci)
    w.loci += b.loci
    tmp = tempfile.mkdtemp()
    fa, bam = synth.write_world_files(w, tmp, block_size=0xFF00)
    text = synth.vcf_text(simple, header=False) + synth.bnd_vcf_text(b)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("source %s; files of %d long DEL loci and %d breakend loci, 15 reads a junction side: %.1f MB BAM, %d usable cores"
        % (_lib.load().vapor_source_id().decode(), n_del, len(b.loci), os.path.getsize(bam) / 1e6, len(os.sched_getaffinity(0))))

    def run(root, mode, k):
        vcf = os.path.join(tmp, "in_%s_%s_%d.vcf" % (os.path.basename(root) or "x", mode, k))
        open(vcf, "w").write(text)
        env = dict(os.environ)
        env.pop("VAPOR_BAM_DEVICE", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, mode, fa, bam, vcf], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("child %s %s failed:\n%s" % (root, mode, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    res = {}
    order = ([("parent", parent, "bnd")] if parent else []) + [("this", HERE, "bnd"), ("this", HERE, "both")]
    for rep in range(repeats):
        for who, root, mode in order:
            got = run(root, mode, rep)
            res.setdefault((who, mode), []).append(got)
            st = got["bam_last_stats"]
            say("repeat %d  %-6s %-5s %7.0f loci/s %7.0f views/s  (%d loci, %d views; runs %s s)  table %s  old columns %s  last extraction call: %s"
                % (rep, who, mode, got["loci"] / got["best_s"], got["views"] / got["best_s"], got["loci"], got["views"],
                   " ".join("%.3f" % t for t in got["runs_s"]), got["table"], got["old_columns"],
                   ("%d regions, %d blocks, %.1f MB -> %.1f MB, inflate %.2f ms, call %.2f ms" % (
                       st["regions"], st["blocks"], st["compressed_bytes"] / 1e6, st["inflated_bytes"] / 1e6, st["inflate_ms"], st["call_ms"])) if st else "none"))
    say()
    med = lambda runs, f="loci": sorted(g[f] / g["best_s"] for g in runs)[len(runs) // 2]      # noqa: E731
    for key, runs in res.items():
        rates = sorted(g["loci"] / g["best_s"] for g in runs)
        say("%-6s %-5s loci/s over %d processes: min %.0f  median %.0f  max %.0f  (spread %.1f %% of the median); views/s median %.0f"
            % (key[0], key[1], len(runs), rates[0], rates[len(rates) // 2], rates[-1], 100.0 * (rates[-1] - rates[0]) / rates[len(rates) // 2],
               med(runs, "views")))
    un, bo = res[("this", "bnd")], res[("this", "both")]
    t_un = sorted(g["best_s"] for g in un)[len(un) // 2]
    t_bo = sorted(g["best_s"] for g in bo)[len(bo) // 2]
    extra = bo[0]["views"] - un[0]["views"]
    say("both-ends / plain: loci/s %.2f, views/s %.2f; %d extra views and %d more loci (5to5) cost %.1f ms: %.1f us per extra view; "
        "the old columns of the records both runs score are equal: %s"
        % (med(bo) / med(un), med(bo, "views") / med(un, "views"), extra, bo[0]["loci"] - un[0]["loci"], 1e3 * (t_bo - t_un),
           1e6 * (t_bo - t_un) / max(extra, 1), {g["old_columns"] for g in bo} == {g["old_columns"] for g in un}))
    if parent:
        pa = res[("parent", "bnd")]
        say("this / parent, plain --bnd: %.3f (medians); tables equal: %s" % (med(un) / med(pa), {g["table"] for g in un} == {g["table"] for g in pa}))
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:7])
    else:
        main()
