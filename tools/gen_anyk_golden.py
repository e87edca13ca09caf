#!/usr/bin/env python3
"""Golden vectors of the any-k route: kmerhits / dotdata at every k from 1 to 64, subkeys, key_modify and the three scorers
at k = 15 and k = 45, from the REFERENCE implementation (loaded by oracle.gen_golden.load_reference, as the other goldens).

TEST INFRASTRUCTURE - runs only where the reference is available.  Writes tests/golden/kmerhits_anyk.json.gz: full hit lists
for the small cases, the count and sha256 of the (j, i) int32 rows for the large ones.  The k > 40 cases run the reference's
edit-distance branch (about a minute and a half each at ~110 bp), so the cases run in parallel processes.

    python tools/gen_anyk_golden.py [--jobs N]

--designs leaves every case of the file as it is and adds, under names of their own: every k from 1 to 40 that EXACT_K lacks
(both modes, the same ~200-symbol shape), the last_symbol designs of tests/anyk_designs.py and its eight golden_rounds() pairs
(k = 41 and 64, D = 64 and 65; a few minutes each in the reference).  A case whose name the file already holds is not run again.

    python tools/gen_anyk_golden.py --designs [--jobs N]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402
from vapor_amd import synth  # noqa: E402

NAME = "kmerhits_anyk.json.gz"
EXACT_K = (1, 2, 3, 5, 7, 11, 15, 16, 17, 25, 31, 32, 33, 39)
EDIT_K = (41, 45, 50, 57, 64)
FULL_MAX = 4000          # hit lists up to this many dots are stored in full, longer ones as count + sha256

_M = None


def _ref():
    global _M
    if _M is None:
        _M = gg.load_reference()
    return _M


def _mut(rng, s, sub=0.04, ins=0.03, dele=0.03):
    out = []
    for c in s:
        r = rng.random()
        if r < dele:
            continue
        if r < dele + sub:
            c = "ACGT"[int(rng.integers(0, 4))]
        out.append(c)
        if rng.random() < ins:
            out.append("ACGT"[int(rng.integers(0, 4))])
    return "".join(out)


def _hits_entry(hits):
    e = {"n": len(hits), "sha": gg.hits_digest(hits)}
    if len(hits) <= FULL_MAX:
        e["hits"] = [[int(j), int(i)] for j, i in hits]
    return e


def job_kmerhits(spec):
    name, k, s1, s2, inv = spec
    m = _ref()
    with contextlib.redirect_stdout(io.StringIO()):          # the reference prints "Window size:<k>" per seq2 position at k > 40
        try:
            r = {"ok": _hits_entry(m.kmerhits(s1, s2, k, 1, inv))}
        except Exception as e:  # noqa: BLE001 - the reference's failure mode is part of the vector
            r = {"error": type(e).__name__}
    return {"kind": "kmerhits", "name": name, "k": k, "s1": s1, "s2": s2, "inversions": inv, "out": r}


def job_scorer(spec):
    name, ref, alt, read, miss, k = spec
    m = _ref()
    x = [read, miss, name]
    c = {"kind": "scorer", "name": name, "ref": ref, "alt": alt, "read": read, "miss": miss, "k": k}
    with contextlib.redirect_stdout(io.StringIO()):
        c["s1"] = gg.call(m.calcu_vapor_single_read_score_abs_dis_m1b, ref, alt, x, k)
        c["s2"] = gg.call(m.calcu_vapor_single_read_score_within_10Perc_m1b, ref, alt, x, k)
        c["s3"] = gg.call(m.calcu_vapor_single_read_score_directed_dis_m1b_redefine_diagnal, ref, alt, x, k)
    return c


def _run(job):
    fn, spec = job
    return fn(spec)


def kmerhits_specs():
    rng = np.random.default_rng(4242)
    rd = lambda n: synth.random_dna(rng, n)  # noqa: E731
    out = []
    for k in EXACT_K:
        a = rd(int(rng.integers(120, 220)))
        b = _mut(rng, a[10:]) + synth.revcomp(a[:60])
        for inv in (True, False):
            out.append(("exact_k%d_%s" % (k, "inv" if inv else "fwd"), k, a, b, inv))
    odd = [
        ("palindrome_AT", 2, "ATATATGCAT" * 3, "TATAATCGAT" * 2),
        ("palindrome_k4", 4, "ACGTTGCAACGT" * 2, "GCATACGTTTGCAA" * 2),
        ("iupac_lower", 5, "ACGRYacgrySWKMbdhvNNacgt" * 2, "acgNNACGnnSWKMacgrYACGT" * 2),
        ("n_runs", 7, "NNNNNNNNNNACGTACGTNNNNNNNNnnnnnnnACGT", "ACGTNNNNNNNNNNnnnnnnnnACGTACGT"),
        ("x_in_seq1", 3, "ACGXTTGCAXXAC", "ACGXTTGCAXUAC"),
        ("x_in_seq2", 3, "ACGTTGCAAAC", "ACGXTTGCAXUACGTT"),
        ("u_and_x", 2, "XUXUXXUUACXU", "UXUXXXUUUACUXZ"),
        ("shorter_than_k", 11, "ACGTACGT", "ACGTACGTACGTACGT"),
        ("seq2_shorter", 11, "ACGTACGTACGTACGT", "ACGTACG"),
        ("empty1", 3, "", "ACGTACGT"),
        ("empty2", 3, "ACGTACGT", ""),
        ("k1_mixed", 1, "ACGTNacgtnRX", "TGCANtgcanYXU"),
        ("k40_case", 33, "acgt" * 12 + "ACGT" * 12, "ACGT" * 12 + "acgt" * 12),
    ]
    for name, k, a, b in odd:
        for inv in (True, False):
            out.append(("%s_%s" % (name, "inv" if inv else "fwd"), k, a, b, inv))
    big = synth.random_dna(rng, 10000)
    win = synth.random_dna(rng, 4000) + _mut(rng, big, 0.03, 0.02, 0.02) + synth.revcomp(big[2000:6000])
    win = win[:20000] + synth.random_dna(rng, max(0, 20000 - len(win)))
    for k in (15, 25):
        out.append(("big_10k_20k_k%d" % k, k, big, win, True))
    for k in EDIT_K:
        L = int(rng.integers(max(60, k + 16), 121))
        a = rd(L)
        unit = rd(7)
        cases = {
            "clean": (a, a[5:] + rd(8)),
            "mutated": (a, _mut(rng, a, 0.03, 0.02, 0.02)),
            "revstrand": (a, synth.revcomp(_mut(rng, a, 0.02, 0.01, 0.01))),
            "tandem": ((unit * 40)[:L], _mut(rng, (unit * 40)[:L], 0.02, 0.02, 0.02)),
            "homopolymer": ("A" * (k + 8) + a[: L - k - 8], "A" * (k + 5) + "C" + "A" * 6),
            "lower": (a.lower(), a[3:].lower()[: L - 10] + a[:10]),
            "n": (a[:30] + "N" * 6 + a[36:], a[:28] + "NN" + a[30:]),
        }
        for nm, (s1, s2) in cases.items():
            out.append(("edit_k%d_%s" % (k, nm), k, s1, s2, True))
        out.append(("edit_k%d_fwd" % k, k, a, _mut(rng, a, 0.03, 0.02, 0.02), False))
    return out


def design_specs():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import anyk_designs as ad
    rng = np.random.default_rng(4343)
    out = []
    for k in range(1, 41):
        if k in EXACT_K:
            continue
        a = synth.random_dna(rng, int(rng.integers(120, 220)))
        b = _mut(rng, a[10:]) + synth.revcomp(a[:60])
        for inv in (True, False):
            out.append(("exact_k%d_%s" % (k, "inv" if inv else "fwd"), k, a, b, inv))
    for p in ad.last_symbol():
        out.append(("last_symbol_%s" % p.name, p.k, p.s1, p.s2, not p.forward))
    for p in ad.golden_rounds():
        assert len(p.s1) <= 200 and len(p.s2) <= 200, p.name
        out.append((p.name, p.k, p.s1, p.s2, not p.forward))
    return out


def add_designs(n_jobs):
    import gzip
    import json
    with gzip.open(os.path.join(ROOT, "tests", "golden", NAME), "rt") as f:
        gold = json.load(f)
    have = {c["name"] for c in gold["cases"]}
    specs = sorted((s for s in design_specs() if s[0] not in have), key=lambda s: -s[1])      # the slow ones (k > 40) first
    with mp.get_context("fork").Pool(n_jobs) as pool:
        res = pool.map(job_kmerhits, specs, chunksize=1)
    order = {s[0]: t for t, s in enumerate(design_specs())}
    gold["cases"] += sorted(res, key=lambda c: order[c["name"]])
    gg.dump(NAME, gold)
    print("added %d cases" % len(res))


def scorer_specs():
    rng = np.random.default_rng(5151)
    out = []
    # k = 15, ~1 kb: a deletion and an inversion allele with a read of the alternative
    g = synth.random_dna(rng, 1400)
    ref = g[:1000]
    alt = ref[:400] + ref[600:]
    out.append(("del_k15", ref, alt, _mut(rng, alt, 0.02, 0.02, 0.02), 0, 15))
    alt2 = ref[:350] + synth.revcomp(ref[350:650]) + ref[650:]
    out.append(("inv_k15", ref, alt2, _mut(rng, alt2, 0.02, 0.02, 0.02)[3:], 2, 15))
    # k = 45, ~100 bp
    g = synth.random_dna(rng, 200)
    ref = g[:80]
    alt = ref[:40] + g[150:170] + ref[40:]
    out.append(("ins_k45", ref, alt, _mut(rng, alt, 0.02, 0.02, 0.02), 0, 45))
    alt2 = ref[:25] + ref[45:]
    out.append(("del_k45", ref, alt2, _mut(rng, ref, 0.02, 0.02, 0.02), 1, 45))
    return out


def subkeys_cases():
    m = _ref()
    keys = ["ACGTACGTAC", "acgRYswkmNn", "ACGTNRYSWKMBDHV", "acgtnrysbdhvwkm", "AAGGCCTT", "A", "", "ACGX", "GATTACAGATTACA"]
    sub = []
    for key in keys:
        for nb in (0, 1, 2, 3):
            for inv in (False, True):
                sub.append({"key": key, "nth_base": nb, "inversions": inv, "out": gg.call(m.subkeys, key, nb, inv)})
    km = [{"key": key, "out": m.key_modify(key)} for key in keys + ["RrYySsWwKkMmBbDdHhVv", "xyzXYZ"]]
    return sub, km


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--designs", action="store_true", help="add the designed cases to the file, leaving its cases as they are")
    a = ap.parse_args()
    if a.designs:
        return add_designs(a.jobs)
    jobs = [(job_kmerhits, s) for s in kmerhits_specs()] + [(job_scorer, s) for s in scorer_specs()]
    # the slow ones (k > 40) first, so that the pool's tail is short
    order = sorted(range(len(jobs)), key=lambda t: -(jobs[t][1][1] if jobs[t][0] is job_kmerhits else
                                                      (99 if jobs[t][1][5] > 40 else 0)))
    with mp.get_context("fork").Pool(a.jobs) as pool:
        res = pool.map(_run, [jobs[t] for t in order], chunksize=1)
    back = [None] * len(jobs)
    for t, r in zip(order, res):
        back[t] = r
    sub, km = subkeys_cases()
    gg.dump(NAME, {"source": "kmerhits SF:951-983 (k 1..64), subkeys SF:1403-1422, key_modify SF:908-949, scorers SF:182-294",
                   "cases": [c for c in back if c["kind"] == "kmerhits"],
                   "scorers": [c for c in back if c["kind"] == "scorer"], "subkeys": sub, "key_modify": km})


if __name__ == "__main__":
    main()
