"""Host time of one vapor_plan_set_reads and of one vapor_plan_set_grid call on a live plan (tools/prof_host.py times the Python
side against a stand-in engine and never enters the library): the checks of csrc/vapor_finish_plan.h, the upload image, the
blocks from the context's pool and the blocking copies.  Two tables: the candidates of a batch of grids (loci x reads-per-locus
reads, groups of --group loci) and a small one.  Per call the median and the fastest of --reps calls, in microseconds, after
--warm unrecorded ones; a JSON line at the end.
Usage: python tools/finish_calls_rate.py [--loci 2000] [--reads 20] [--group 25] [--reps 300]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=2000)
    ap.add_argument("--reads", type=int, default=20)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warm", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    from vapor_amd import _lib as L
    from vapor_amd import synth
    from vapor_amd.engine import Engine
    alleles, reads, pr = synth.make_pairs(seed=3, n_alleles=4, reads_per_allele=5, read_len=2000, allele_len=3500)
    eng = Engine(0)
    ss = eng.seqset(alleles + reads)
    plan = eng.plan(ss, eng.make_pairs([(len(alleles) + r, al, 0, 10, 3) for r, al in pr]))
    plan.run()
    rec = {"source_id": L.load().vapor_source_id().decode(), "reps": a.reps, "tables": {}}
    for name, n_loci, per, group in (("batch", a.loci, a.reads, a.group), ("small", 3, 2, 1)):
        n_loci -= n_loci % group
        t = np.zeros(n_loci * per, dtype=L.READ_DTYPE)
        t["ref_a"] = np.arange(len(t)) % plan.n
        t["alt_a"] = (np.arange(len(t)) + 1) % plan.n
        t["kind"] = 1
        t["locus"] = np.arange(len(t)) // per
        t["len_ref"] = t["len_alt"] = 3000
        first = np.arange(0, n_loci + 1, group, dtype=np.int32)
        times = {"set_reads": [], "set_grid": []}
        for rep in range(a.warm + a.reps):
            t0 = time.perf_counter()
            plan.set_reads(t, n_loci)
            t1 = time.perf_counter()
            plan.set_grid(first)
            t2 = time.perf_counter()
            if rep >= a.warm:
                times["set_reads"].append((t1 - t0) * 1e6)
                times["set_grid"].append((t2 - t1) * 1e6)
        plan.run_grid()                                        # (the tables are ones a run takes)
        rec["tables"][name] = dict({"reads": len(t), "loci": n_loci, "groups": len(first) - 1},
                                   **{k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2)} for k, v in times.items()})
        for k, v in times.items():
            print("%-6s %-9s %8d reads %6d loci %5d groups   median %9.2f us   fastest %9.2f us" % (
                name, k, len(t), n_loci, len(first) - 1, statistics.median(v), min(v)), file=sys.stderr, flush=True)
    plan.close()
    ss.close()
    eng.close()
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
