"""Speed of the any-k route (vapor_anyk_batch) on one MI355X, one pair per call:
  exact: k = 15 on a 10 kb read x 20 kb window, against vapor_wide_batch at k = 10 on the same pair (target: at most 1.5 x);
  edit:  k = 50 (the edit-distance branch) on a 10 kb read at ~10 % error x 20 kb window (target: at most 250 ms per pair).
Usage: python tools/anyk_rate.py [--reps N] [--only exact|edit]  -> one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes().decode()


def mutate(rng, s, sub, ins, dele):
    """substitutions, insertions and deletions at the given per-base rates"""
    a = np.frombuffer(s.encode(), dtype=np.uint8)
    r = rng.random(len(a))
    keep = r >= dele
    out = a.copy()
    subs = (r >= dele) & (r < dele + sub)
    out[subs] = ACGT[rng.integers(0, 4, int(subs.sum()))]
    parts = []
    ins_at = rng.random(len(a)) < ins
    for p in np.flatnonzero(keep):
        parts.append(out[p])
        if ins_at[p]:
            parts.append(ACGT[rng.integers(0, 4)])
    return np.asarray(parts, dtype=np.uint8).tobytes().decode()


def timed(fn, reps):
    fn()                                    # warm-up: code objects, pool allocations
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("exact", "edit"), default=None)
    a = ap.parse_args()
    from vapor_amd.engine import Engine
    rng = np.random.default_rng(1)
    eng = Engine(0)
    win = rand(rng, 20000)
    out = {}
    if a.only in (None, "exact"):
        rd = mutate(rng, win[5000:15000], 0.02, 0.01, 0.01)
        ss = eng.seqset([rd, win])
        p15 = eng.make_pairs([(0, 1, 0, 15, 7)])
        p10 = eng.make_pairs([(0, 1, 0, 10, 7)])
        assert np.array_equal(eng.score_anyk(ss, p10), eng.score_wide(ss, p10))
        t15 = timed(lambda: eng.score_anyk(ss, p15), a.reps)
        t10a = timed(lambda: eng.score_anyk(ss, p10), a.reps)
        t10w = timed(lambda: eng.score_wide(ss, p10), a.reps)
        dots = int(eng.score_anyk(ss, p15)[0, 0])
        ss.close()
        out["exact_k15_10kx20k"] = {"dots": dots, "anyk_k15_ms": t15 * 1e3, "anyk_k10_ms": t10a * 1e3, "wide_k10_ms": t10w * 1e3,
                                    "anyk_k15_over_wide_k10": t15 / t10w, "target_ratio": 1.5}
    if a.only in (None, "edit"):
        rd = mutate(rng, win[4000:14400], 0.04, 0.03, 0.03)[:10000]
        ss = eng.seqset([rd, win])
        p50 = eng.make_pairs([(0, 1, 0, 50, 7)])
        reps = max(1, min(a.reps, 3))
        t50 = timed(lambda: eng.score_anyk(ss, p50), reps)
        st = eng.score_anyk(ss, p50)
        ss.close()
        out["edit_k50_10kx20k_10pct"] = {"read_len": len(rd), "dots": int(st[0, 0]), "status": int(st[0, 15]),
                                         "anyk_ms": t50 * 1e3, "target_ms": 250.0}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
