#!/usr/bin/env python3
"""Rate of `vapor vcf --bnd` beside long deletions on the same world, from FASTA / BAM files (profiles/bnd_rate.txt).

The world is synth.make_world's long deletions (spans of 10 kb and more: the drivers' junction-window branch, SF:1727-1745).
The deletion run scores their DEL records.  The breakend run scores the same junctions written as breakend pairs: `t[A:e+1[`
at A:s with its `]A:s]t` mate (one 3to5 locus), or every other pair a `t]A:e+1]` 3to3 record with its mate (the
reverse-complemented right piece; same windows and reads).  Figures are off; each run is repeated and the best wall time
of cli.main is kept.

    python tools/bnd_rate.py [--loci 2000] [--repeat 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vapor_amd import cli, pipeline, seqio, synth  # noqa: E402


def bnd_text(w) -> str:
    out = []
    for t, l in enumerate(w.loci):
        c, s, q = l.chrom, l.start, l.end + 1
        rs, rq = w.contigs[c][s - 1], w.contigs[c][q - 1]
        form = "3to5" if t % 2 == 0 else "3to3"
        mate = "5to3" if form == "3to5" else "3to3"
        out.append("\t".join([c, str(s), "b%d_1" % t, rs, synth.bnd_alt(form, rs, "", c, q), ".", "PASS",
                              "SVTYPE=BND;MATEID=b%d_2" % t, "GT", "0/1"]))
        out.append("\t".join([c, str(q), "b%d_2" % t, rq, synth.bnd_alt(mate, rq, "", c, s), ".", "PASS",
                              "SVTYPE=BND;MATEID=b%d_1" % t, "GT", "0/1"]))
    return "\n".join(out) + "\n"


def run(d, name, text, fa, bam, bnd):
    vcf = os.path.join(d, name + ".vcf")
    with open(vcf, "w") as f:
        f.write(text)
    args = ["vcf", "--sv-input", vcf, "--reference", fa, "--pacbio-input", bam, "--output-path", os.path.join(d, "figs"),
            "--output-file", "unused", "--no-figures"] + (["--bnd"] if bnd else [])
    t0 = time.perf_counter()
    assert cli.main(args) == 0
    dt = time.perf_counter() - t0
    rows = [x for x in open(vcf + ".vapor") if not x.startswith("#")]
    return dt, len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    w = synth.make_world(seed=2000, n_loci=a.loci, svtypes=("DEL",), spans=(10000, 12500, 16000, 24000), read_len=1500, n_reads=10)
    d = tempfile.mkdtemp(prefix="bnd_rate_")
    fa, bam = synth.write_world_files(w, d)
    seqio.set_backend(seqio.InProcessBam())
    pipeline.set_engine(None)
    texts = {"DEL": synth.vcf_text(w, header=False), "BND": bnd_text(w)}
    run(d, "warm", texts["DEL"], fa, bam, False)              # (engine, readers and library loaded)
    res = {}
    for rep in range(a.repeat):
        for kind in ("DEL", "BND"):
            dt, n = run(d, "%s_%d" % (kind, rep), texts[kind], fa, bam, kind == "BND")
            best = res.get(kind)
            if best is None or dt < best["s"]:
                res[kind] = {"s": round(dt, 4), "loci": a.loci, "records": len(texts[kind].splitlines()), "annotated": n,
                             "loci_per_s": round(a.loci / dt, 1)}
    res["bnd_over_del_time"] = round(res["BND"]["s"] / res["DEL"]["s"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
