"""What the read filter costs on the files path (FASTA + BAM through the product CLI, reads extracted on the device): the world
of tools/files_ab.py written twice - as it is, and with synth.add_decoys' records planted (seven a locus) - and three runs
alternating, each in a warm process of its own: with --parent DIR the plain run of another checkout (the parent commit, built) on
the clean files, this tree's plain run on the clean files, this tree's run with --min-mapq 20 --exclude-flags 0xF04 on the decoy
files.  The spread between one build's own repeats can then be read beside the difference between the builds, and the filtered
run's table must be the plain run's.
  python tools/read_filter_rate.py [n_loci] [--qual | --both] [--repeats R] [--parent DIR] [--bed-repeat K] [--filtered-repeats F]
(--qual: seeded qualities instead of 0xFF; --both: the two one after the other on one world, its files written side by side)
(--bed-repeat K: the same loci K times over in the BED file, as tools/files_ab.py --repeat does - a run of several seconds from
files of 2 000 loci; --filtered-repeats F: the filtered run only in the first F repeats, it is informational)
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
FILTER = ["--min-mapq", "20", "--exclude-flags", "0xF04"]


def child(root, mode, fa, bam, bed):
    sys.path.insert(0, root)
    from vapor_amd import cli
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "o.vapor")
    args = ["bed", "--sv-input", bed, "--reference", fa, "--pacbio-input", bam, "--output-path", tmp + "/f", "--output-file", out, "--no-figures"]
    if mode == "filtered":
        args += FILTER
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


_WORLDS = {}


def _write(name, qual, directory):
    from vapor_amd import synth
    return synth.write_world_files(_WORLDS[name], directory, block_size=0xFF00, qual_seed=(7 if qual else None))


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
    filtered_repeats = int(opt("--filtered-repeats", "1000"))
    parent = opt("--parent")
    quals = [False, True] if "--both" in argv else ["--qual" in argv]
    pos = [a for a in argv if not a.startswith("--")]
    n = int(pos[0]) if pos else 2000
    sys.path.insert(0, HERE)
    from vapor_amd import _lib, synth
    w = synth.make_world(seed=11, n_loci=n, svtypes=("DEL", "DEL", "INV", "INS"), span_range=(100, 4000), read_len=9500, n_reads=20)
    d = synth.add_decoys(w, seed=13)
    for world in (w, d):
        for c in world.reads:
            world.reads[c] = sorted(world.reads[c], key=lambda r: r.pos)
    # every file set in a process of its own (forked: the worlds are inherited, not copied)
    import multiprocessing
    _WORLDS.update(clean=w, decoy=d)
    jobs = [(name, q, tempfile.mkdtemp()) for q in quals for name in ("clean", "decoy")]
    with multiprocessing.get_context("fork").Pool(len(jobs)) as pool:
        written = pool.starmap(_write, jobs)
    bed = os.path.join(jobs[0][2], "in.bed")
    open(bed, "w").write(synth.bed_text(w) * bed_repeat)
    for qual in quals:
        files = {name: fb for (name, q, _t), fb in zip(jobs, written) if q == qual}
        section(files, bed, n, bed_repeat, qual, parent, repeats, filtered_repeats)
        print(flush=True)


def section(files, bed, n, bed_repeat, qual, parent, repeats, filtered_repeats):
    from vapor_amd import _lib
    print("source %s; files of %d loci of 20 reads, the BED file %d times over: %.1f MB BAM clean, %.1f MB with 7 decoys a locus, %s qualities, %d usable cores"
          % (_lib.load().vapor_source_id().decode(), n, bed_repeat, os.path.getsize(files["clean"][1]) / 1e6, os.path.getsize(files["decoy"][1]) / 1e6,
             "seeded" if qual else "absent", len(os.sched_getaffinity(0))), flush=True)

    def run(root, mode):
        fa, bam = files["decoy" if mode == "filtered" else "clean"]
        env = dict(os.environ)
        env.pop("VAPOR_BAM_DEVICE", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, mode, fa, bam, bed], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("child %s %s failed:\n%s" % (root, mode, r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    res = {}
    order = ([("parent", parent, "plain")] if parent else []) + [("this", HERE, "plain"), ("this", HERE, "filtered")]
    for rep in range(repeats):
        for who, root, mode in order:
            if mode == "filtered" and rep >= filtered_repeats:
                continue
            got = run(root, mode)
            res.setdefault((who, mode), []).append(got)
            print("repeat %d  %-6s %-8s %7.0f loci/s  (runs %s s)  table %s"
                  % (rep, who, mode, got["loci"] / got["best_s"], " ".join("%.3f" % t for t in got["runs_s"]), got["table"]), flush=True)
    print()
    for key, runs in res.items():
        rates = sorted(g["loci"] / g["best_s"] for g in runs)
        print("%-6s %-8s loci/s over %d processes: min %.0f  median %.0f  max %.0f  (spread %.1f %% of the median)"
              % (key[0], key[1], len(runs), rates[0], rates[len(rates) // 2], rates[-1], 100.0 * (rates[-1] - rates[0]) / rates[len(rates) // 2]))
    med = lambda runs: sorted(g["loci"] / g["best_s"] for g in runs)[len(runs) // 2]      # noqa: E731
    pl, fi = res[("this", "plain")], res[("this", "filtered")]
    print("filtered on the decoy files / plain on the clean files: rate %.2f (medians); tables equal: %s"
          % (med(fi) / med(pl), {g["table"] for g in fi} == {g["table"] for g in pl}))
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
