"""Rate of `vapor bed --refine 50` on one MI355X: a warm process, one world of DEL / INV / TANDUP loci from FASTA + BAM files,
three ways -

    unrefined   `vapor bed` as it is without the option
    brute       --refine 50 by the brute-force route (VAPOR_REFINE_ROUTE=brute: one Score request per candidate - the reads
                uploaded and joined against the window once per candidate -, host finish, pick in Python)
    batched     --refine 50 by the batched route (one sequence set and one plan per batch of grids, reads and window uploaded
                once, the (read, window) pairs joined once, grid_pick_kernel behind finish_kernel)

Per way loci/s (best of --reps timed runs after a warm one).  The two refined tables must be byte-identical.  Writes
$OUT/refine_rate.json (default profile_out/) and prints it.  Under `rocprofv3 --kernel-trace --stats -- python
tools/refine_rate.py --only batched --reps 1` the kernel statistics give grid_pick_kernel's share.
Usage: python tools/refine_rate.py [--loci 240] [--reps 2] [--only batched]"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=240)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--refine", default="50")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    from vapor_amd import _lib, cli, refine, synth
    w = synth.make_world(seed=17, n_loci=a.loci, svtypes=("DEL", "INV", "TANDUP"), span_range=(150, 2500), read_len=6000, n_reads=20)
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    tmp = tempfile.mkdtemp(prefix="vapor_refine_rate_")
    fa, bam = synth.write_world_files(w, tmp, block_size=0xFF00)
    bed = os.path.join(tmp, "in.bed")
    open(bed, "w").write(synth.bed_text(w))
    m, t = refine.parse(a.refine)
    rec = {"source_id": _lib.load().vapor_source_id().decode(), "loci": a.loci, "refine": "%d:%d" % (m, t),
           "candidates_per_locus": len(refine.candidates(m, t, 1000, 5000)), "reads_per_locus": 20, "ways": {}}
    shas = {}
    for name, more, route in (("unrefined", [], None), ("brute", ["--refine", a.refine], "brute"), ("batched", ["--refine", a.refine], "batched")):
        if a.only and name not in a.only.split(","):
            continue
        out = os.path.join(tmp, "o_%s.vapor" % name)
        args = ["bed", "--sv-input", bed, "--reference", fa, "--pacbio-input", bam, "--output-path", tmp + "/f", "--output-file", out,
                "--no-figures"] + more
        if route:
            os.environ["VAPOR_REFINE_ROUTE"] = route
        else:
            os.environ.pop("VAPOR_REFINE_ROUTE", None)
        best = 1e9
        for rep in range(a.reps + 1):                              # (the first run is the warm one: engines, pools, page cache)
            with contextlib.redirect_stdout(io.StringIO()):
                t0 = time.perf_counter()
                cli.main(args)
                dt = time.perf_counter() - t0
            if rep:
                best = min(best, dt)
        rows = open(out).read().splitlines()[1:]
        shas[name] = hashlib.sha256(open(out, "rb").read()).hexdigest()[:16]
        r = {"loci_per_s": round(a.loci / best, 1), "run_s": round(best, 3), "table_sha16": shas[name]}
        if more:
            r["refined_loci"] = sum(1 for x in rows if x.split("\t")[-1] != ".")
            r["winner_is_not_the_call"] = sum(1 for x in rows if x.split("\t")[-1] != "." and x.split("\t")[-4:-2] != x.split("\t")[1:3])
        rec["ways"][name] = r
        print("%-10s %9.1f loci/s  (%.3f s)" % (name, r["loci_per_s"], best), file=sys.stderr, flush=True)
    os.environ.pop("VAPOR_REFINE_ROUTE", None)
    ways = rec["ways"]
    ok = True
    if "brute" in ways and "batched" in ways:
        rec["tables_identical"] = ok = shas["brute"] == shas["batched"]
        rec["batched_vs_brute"] = round(ways["batched"]["loci_per_s"] / ways["brute"]["loci_per_s"], 2)
    if "unrefined" in ways and "batched" in ways:
        rec["batched_vs_unrefined"] = round(ways["batched"]["loci_per_s"] / ways["unrefined"]["loci_per_s"], 4)
    d = os.environ.get("OUT", "profile_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "refine_rate.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
