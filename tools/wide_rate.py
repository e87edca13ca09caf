"""Speed of the wide route (vapor_wide_batch) on one MI355X: pairs/s for 70 kb x 70 kb and 300 kb x 300 kb pairs, the C oracle
on one core for the same pair, and narrow-sized pairs through both routes (the cost of the wider format).
Usage: python tools/wide_rate.py [--reps N]  -> one JSON line."""
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


def mutate(rng, s, rate=0.02):
    a = np.frombuffer(s.encode(), dtype=np.uint8).copy()
    pos = rng.random(len(a)) < rate
    a[pos] = ACGT[rng.integers(0, 4, int(pos.sum()))]
    return a.tobytes().decode()


def timed(fn, reps):
    fn()                                    # warm-up: code objects, pool allocations
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from vapor_amd.engine import Engine
    from oracle import oracle as orc
    rng = np.random.default_rng(1)
    eng = Engine(0)
    out = {}
    for n in (70000, 300000):
        al = rand(rng, n)
        rd = mutate(rng, al)
        ss = eng.seqset([rd, al])
        pr = eng.make_pairs([(0, 1, 0, 10, 7)])
        st = eng.score_wide(ss, pr)
        dt = timed(lambda: eng.score_wide(ss, pr), a.reps)
        t0 = time.perf_counter()
        exp = orc.pair_stats(10, rd, al)
        t_orc = time.perf_counter() - t0
        ss.close()
        assert st[0, :10].tolist() == exp[:10].tolist()
        out["pair_%dk" % (n // 1000)] = {"dots": int(st[0, 0]), "wide_ms": dt * 1e3, "pairs_per_s": 1.0 / dt,
                                         "oracle_one_core_ms": t_orc * 1e3, "speedup_vs_oracle": t_orc / dt}
    from vapor_amd import synth
    alleles, reads, prs = synth.make_pairs(seed=3, n_alleles=8, reads_per_allele=8, read_len=8000, allele_len=12000)
    ss = eng.seqset(alleles + reads)
    pr = eng.make_pairs([(len(alleles) + r, al, 0, 10, 7) for r, al in prs])
    narrow = eng.score(ss, pr)
    wide = eng.score_wide(ss, pr)
    assert np.array_equal(narrow, wide)
    tn = timed(lambda: eng.score(ss, pr), a.reps)
    tw = timed(lambda: eng.score_wide(ss, pr), a.reps)
    ss.close()
    out["narrow_sized_%d_pairs" % len(pr)] = {"narrow_ms": tn * 1e3, "wide_ms": tw * 1e3, "wide_over_narrow": tw / tn}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
