"""What an evidence mode (`--depth`, `--signatures`, `--links`, `--support`; `--realign` through tools/realign_rate.py) costs on the files path (FASTA + BAM through the
product CLI): one synthetic world of the mode (MODES below: its maker in vapor_amd/synth.py, its flag, the columns it appends to a
row) written to files, and runs alternating, each in a warm process of its own: with --parent DIR the plain run and the run with
the mode on of another checkout (the parent commit, built), then this tree's plain run and its run with the mode on.  The spread
between one build's own repeats can then be read beside the difference between the builds; the five columns of a mode run's rows
must be the plain run's, and the tables of the two trees' mode runs must be equal.
  python tools/evidence_rate.py MODE [n_loci] [--repeats R] [--parent DIR] [--bed-repeat K] [--layers N] [--reads N]
                                [--mode-repeats F] [--plain-repeats F] [--timeout S] [--kernel-only]
(MODE: depth, sig, links, sup or ra - `--realign`, which a parent checkout from before the option does not run: its plain run only; --bed-repeat K: the same loci K times over in the BED file; --mode-repeats / --plain-repeats F:
those runs only in the first F repeats; --timeout S: the limit of one process; --kernel-only: this tree's mode run once, in this
process - for a kernel trace of the mode's kernel)
A child (`--child ROOT MODE ON FA BAM BED`) is one such process, importing vapor_amd from ROOT."""
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


def _spans_types(n, types, spans, zyg=("het", "hom")):
    return [(types[i % len(types)], spans[i % len(spans)], zyg[(i // 2) % len(zyg)]) for i in range(n)]


def _depth_world(synth, n, o):
    spans = SPANS[:-1] + (30000,)
    w = synth.make_depth_world(seed=17, specs=_spans_types(n, ("DEL", "TANDUP"), spans), layers=o["layers"], read_len=6000, errors=(0.01, 0.04, 0.03))
    return w, "DEL / TANDUP loci (spans %d .. %d) at depth %d" % (min(spans), max(spans), 2 * o["layers"])


def _sig_world(synth, n, o):
    w = synth.make_signature_world(seed=17, specs=_spans_types(n, TYPES, SPANS), layers=o["layers"], read_len=6000, jitter=(0, 2, -2, 2))
    return w, "DEL / TANDUP / INV / INS loci (spans %d .. %d) at depth %d" % (min(SPANS), max(SPANS), 2 * o["layers"])


def _links_world(synth, n, o):
    types = ("DEL", "TANDUP", "INV", "DEL")
    w = synth.make_links_world(seed=17, specs=[types[i % 4] for i in range(n)], reads=o["reads"], half=3000, margin=8000, ref_reads=o["reads"],
                               jitter=(0, 2, -2, 2))
    return w, "DEL / TANDUP / INV loci of 12 kb, %d split molecules a junction" % o["reads"]


def _sup_world(synth, n, o):
    w = synth.make_support_world(seed=17, specs=_spans_types(n, TYPES, SPANS, ("het", "hom", "ref")), layers=o["layers"], read_len=6000)
    return w, "DEL / TANDUP / INV / INS loci (spans %d .. %d; het, hom, ref) at depth %d" % (min(SPANS), max(SPANS), 2 * o["layers"])


def _count(label, col):
    return lambda rows: "%s %d" % (label, sum(1 for r in rows if r[col] not in (".", "0")))


def _genotypes(rows, col=-2):
    gts = {}
    for r in rows:
        gts[r[col]] = gts.get(r[col], 0) + 1
    return "genotypes " + " ".join("%s: %d" % kv for kv in sorted(gts.items()))


# per mode: the world's maker, the CLI's flag, the columns the mode appends to a row, what is said of a mode run's rows
MODES = {"depth": (_depth_world, "--depth", 4, lambda rows: "supported %d" % sum(1 for r in rows if r[-1] == "1")),
         "sig": (_sig_world, "--signatures", 6, _count("with signature reads", -3)),
         "links": (_links_world, "--links", 7, _count("with linked reads", -5)),
         "sup": (_sup_world, "--support", 9, _genotypes),
         "ra": (_sup_world, "--realign", 7, lambda rows: _genotypes(rows, -3))}
NOT_IN_PARENT = ("ra",)          # modes a parent checkout does not have: only its plain run is taken


def child(root, mode, on, fa, bam, bed, runs=4):
    sys.path.insert(0, root)
    from vapor_amd import cli
    _world, flag, cols, said = MODES[mode]
    on = on == "1"
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "o.vapor")
    args = ["bed", "--sv-input", bed, "--reference", fa, "--pacbio-input", bam, "--output-path", tmp + "/f", "--output-file", out, "--no-figures"]
    n = sum(1 for _ in open(bed))
    times = []
    for _ in range(runs):                               # (the first is the warm-up: engines, pools, page cache)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            rc = cli.main(args + ([flag] if on else []))
            times.append(time.perf_counter() - t0)
        assert rc in (0, None), rc
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    own = "\n".join("\t".join(r[:-cols] if on else r) for r in rows)
    note = "  measured %d, %s" % (sum(1 for r in rows[1:] if r[-cols] != "."), said(rows[1:])) if on else ""
    print(json.dumps({"loci": n, "best_s": min(times[1:] or times), "runs_s": times[1:] or times, "note": note,
                      "table": hashlib.sha256(own.encode()).hexdigest()[:16],
                      "answers": hashlib.sha256(open(out, "rb").read()).hexdigest()[:16]}), flush=True)


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
    only_first = {True: int(opt("--mode-repeats", "1000")), False: int(opt("--plain-repeats", "1000"))}
    o = {"layers": int(opt("--layers", "4")), "reads": int(opt("--reads", "8"))}
    limit = float(opt("--timeout", "240"))
    parent = opt("--parent")
    kernel_only = "--kernel-only" in argv
    pos = [a for a in argv if not a.startswith("--")]
    if not pos or pos[0] not in MODES:
        raise SystemExit("usage: evidence_rate.py {%s} [n_loci] [options]" % "|".join(MODES))
    mode, n = pos[0], int(pos[1]) if len(pos) > 1 else 200
    flag = MODES[mode][1]
    sys.path.insert(0, HERE)
    from vapor_amd import _lib, synth
    w, what = MODES[mode][0](synth, n, o)
    d = tempfile.mkdtemp()
    fa, bam = synth.write_world_files(w, d, block_size=0xFF00)
    bed = os.path.join(d, "in.bed")
    open(bed, "w").write(synth.bed_text(w) * bed_repeat)
    print("source %s; files of %d %s, the BED file %d times over: %.1f MB BAM, %d usable cores"
          % (_lib.load().vapor_source_id().decode(), n, what, bed_repeat, os.path.getsize(bam) / 1e6, len(os.sched_getaffinity(0))), flush=True)
    if kernel_only:
        child(HERE, mode, "1", fa, bam, bed, runs=1)
        return

    def run(root, on):
        env = dict(os.environ)
        env.pop("VAPOR_BAM_DEVICE", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, mode, "01"[on], fa, bam, bed], env=env, capture_output=True, text=True,
                           timeout=limit)
        if r.returncode != 0:
            raise SystemExit("child %s %s failed:\n%s" % (root, mode if on else "plain", r.stderr[-3000:]))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    res = {}
    order = ([("parent", parent, False)] + ([("parent", parent, True)] if mode not in NOT_IN_PARENT else []) if parent else [])
    order += [("this", HERE, False), ("this", HERE, True)]
    for rep in range(repeats):
        for who, root, on in order:
            if rep >= only_first[on]:
                continue
            got = run(root, on)
            res.setdefault((who, on), []).append(got)
            print("repeat %d  %-6s %-6s %7.0f loci/s  (runs %s s)  own columns %s%s"
                  % (rep, who, mode if on else "plain", got["loci"] / got["best_s"], " ".join("%.3f" % t for t in got["runs_s"]), got["table"], got["note"]),
                  flush=True)
    print()
    rates = lambda runs: sorted(g["loci"] / g["best_s"] for g in runs)         # noqa: E731
    med = lambda runs: rates(runs)[len(runs) // 2]                              # noqa: E731
    for (who, on), runs in res.items():
        r = rates(runs)
        print("%-6s %-6s loci/s over %d processes: min %.0f  median %.0f  max %.0f  (spread %.1f %% of the median)"
              % (who, mode if on else "plain", len(runs), r[0], med(runs), r[-1], 100.0 * (r[-1] - r[0]) / med(runs)))
    pl, md = res[("this", False)], res[("this", True)]
    print("%s / plain: rate %.2f (medians); the rows' own columns equal: %s" % (flag, med(md) / med(pl), {g["table"] for g in md} == {g["table"] for g in pl}))
    if parent:
        for on, mine in ((False, pl), (True, md)):
            if ("parent", on) not in res:
                continue
            pa = res[("parent", on)]
            rp = rates(pa)
            inside = sum(1 for g in mine if rp[0] <= g["loci"] / g["best_s"] <= rp[-1])
            below = sum(1 for g in mine if g["loci"] / g["best_s"] < rp[0])
            print("this / parent, %s: %.3f (medians); tables equal: %s; %d of this tree's %d runs lie inside the parent's own spread (%.0f .. %.0f), %d below its minimum"
                  % (mode if on else "plain", med(mine) / med(pa), {g["answers"] for g in mine} == {g["answers"] for g in pa}, inside, len(mine), rp[0], rp[-1], below))
        if ("parent", True) in res:
            print("%s: this tree's median %.0f loci/s, the parent's minimum %.0f: %s"
                  % (flag, med(md), rates(res[("parent", True)])[0], "not below" if med(md) >= rates(res[("parent", True)])[0] else "BELOW"))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:8])
    else:
        main()
