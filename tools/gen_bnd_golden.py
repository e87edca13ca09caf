#!/usr/bin/env python3
"""Golden vectors of `vapor vcf --bnd`: the breakend loci of a small translocation world
(vapor_amd.synth.make_bnd_world), scored by the REFERENCE's own pieces on the windows and alleles §7 defines -
ref_seq_readin (SF:1203-1217) and the long-deletion branch's read selection (simple_del_chop_pacbio_read_simple_short,
SF:1378-1390), window_size_refine (SF:2030-2046) on the ref window and then on the alt allele, the within_10Perc_m1b scorer
(SF:277-294) with that branch's reduction (SF:1739-1745), result_organize_ins (SF:1219-1231), write_output_main (SF:2084-2088)
and vcf_vapor_modify (SF:1972-2028) for the annotated VCF.  The views come from the world's truth, not from the parser under test.

TEST INFRASTRUCTURE - runs only where the reference is available (loaded by oracle.gen_golden.load_reference, as the other
goldens).  Writes tests/golden/bnd.json.gz.

    python tools/gen_bnd_golden.py
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402
from vapor_amd import synth  # noqa: E402

NAME = "bnd.json.gz"
F = 500
WORLD = dict(seed=2027, forms=("3to5", "3to3", "5to3", "5to5", "3to5", "3to3", "5to3"), ins=("", "", "", "", "ACGTT", "GGA", "TC"),
             n_reads=8, ref_fraction=0.25, read_len=2400)


def views(w):
    """(record index in bnd_records, scored view [A, p, B, q, CT, ins]) per junction whose form is scored: 5to3 as its mirror."""
    out = []
    for j, l in enumerate(w.loci):
        form, b, p, q, ins = l.extra["form"], l.extra["mate_chrom"], l.start, l.end, l.ins_seq or ""
        if form in ("3to5", "3to3"):
            out.append((2 * j, [l.chrom, p, b, q, form, ins]))
        elif form == "5to3":
            out.append((2 * j, [b, q, l.chrom, p, "3to5", ins]))
    return out


def score_view(m, v, num_reads_cff=3):
    a, p, b, q, ct, ins = v
    key = ":".join([str(i) for i in v[:5]] + ["BND"])
    rec = {"view": v, "key": key}
    reads = m.simple_del_chop_pacbio_read_simple_short("x.bam", [a, p], F)
    rec["reads"] = [[x[0], x[1], x[2]] for x in reads]
    scores = []
    if len(reads) > num_reads_cff:
        ref_seq = m.ref_seq_readin("ref.fa", a, p - F, p + F)
        rec["ref_seq"] = ref_seq
        k = m.window_size_refine(ref_seq)[0]
        rec["k_ref"] = k
        if not k == "Error":
            right = m.ref_seq_readin("ref.fa", b, q - 1, q - 1 + F) if ct == "3to5" else m.ref_seq_readin("ref.fa", b, q - F, q, "TRUE")
            alt = m.ref_seq_readin("ref.fa", a, p - F, p) + ins + right
            rec["alt_seq"] = alt
            k = m.window_size_refine(alt)[0]
            rec["k"] = k
            if not k == "Error":
                for x in reads:
                    s = m.calcu_vapor_single_read_score_within_10Perc_m1b(ref_seq, alt, x, k)
                    if 0 not in s:
                        scores.append(1 - float(s[1]) / float(s[0]))
    rec["scores"] = scores
    rec["organize"] = m.result_organize_ins([key, scores])
    return rec


def main():
    m = gg.load_reference()
    m.make_event_figure_1 = lambda *a, **k: None
    w = synth.make_bnd_world(**WORLD)
    m.os = gg.ShimOS(w)
    np.random.seed(7)                 # (the reference's X-means draws from numpy's global generator, SF:860-881)
    tmp = tempfile.mkdtemp(prefix="vapor_golden_")
    vcf = os.path.join(tmp, "bnd.vcf")
    text = synth.bnd_vcf_text(w, mates=True, header=False)
    with open(vcf, "w") as f:
        f.write(text)
    per_locus, rec_hash = [], {}
    for r, v in views(w):
        got = score_view(m, v)
        per_locus.append(got)
        rec_hash[r] = rec_hash[r + 1] = got["key"]         # both mates carry the locus's annotation
        print("  %s: k=%s, %d reads, scores %s" % (got["key"], got.get("k"), len(got["reads"]), [round(s, 2) for s in got["scores"]]))
    m.os = os
    m.write_output_initiate(vcf + ".vapor")
    for got in per_locus:
        m.write_output_main(vcf + ".vapor", got["organize"])
    table = open(vcf + ".vapor").read()
    rec_new = {}
    for k1, v in sorted(rec_hash.items()):
        rec_new.setdefault(v, []).append(k1)
    m.vcf_vapor_modify(vcf, rec_new)
    final = open(vcf + ".vapor").read()
    gg.dump(NAME, {"source": "breakend loci of DESIGN.md §7 through ref_seq_readin SF:1203-1217, simple_del_chop_pacbio_read_simple_short "
                             "SF:1378-1390, window_size_refine SF:2030-2046, within_10Perc_m1b SF:277-294 reduced as SF:1739-1745, "
                             "result_organize_ins SF:1219-1231, write_output_main SF:2084-2088, vcf_vapor_modify SF:1972-2028",
                   "world_args": {k: list(v) if isinstance(v, tuple) else v for k, v in WORLD.items()},
                   "world": gg.world_to_json(w), "vcf": text, "cases": per_locus, "vapor_text": table, "final": final})


if __name__ == "__main__":
    main()
