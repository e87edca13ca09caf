"""Files-path rate of `vapor bed` with a bgzipped reference: a warm process, 10 000 loci from FASTA + BAM files (bench.py's
files_rate style: the file's distinct loci several times over), three ways -

    plain        ref.fa + .fai (FaiFasta on the host, as before)
    bgzf_device  ref.fa.gz + .fai + .gzi, the fast route's windows inflated and cut on the device (vapor_fasta_windows_device)
    bgzf_host    the same file, every window read by the host reader (seqio.BgzfFasta): the device route is switched off here, in
                 the tool, by answering fastpath._device_fasta with None - the product has no such switch

Per way: loci/s (best of --reps timed runs after a warm one), the seconds the host spent reading windows (FaiFasta / BgzfFasta
fetch, summed over threads) and in the device call, and the device call's last_stats.  The three tables must be byte-identical.
Writes $OUT/fasta_rate.json (default profile_out/) and prints it.
Usage: python tools/fasta_rate.py [--distinct 1000] [--repeat 10] [--reps 3] [--only bgzf_device]"""
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
    ap.add_argument("--distinct", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    from vapor_amd import _lib, cli, fastpath, seqio, synth
    from vapor_amd.engine import Engine
    w = synth.make_world(seed=11, n_loci=a.distinct, svtypes=("DEL", "DEL", "INV", "INS"), span_range=(100, 4000), read_len=9500, n_reads=20)
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    tmp = tempfile.mkdtemp(prefix="vapor_fasta_rate_")
    t0 = time.perf_counter()
    fa, bam = synth.write_world_files(w, tmp, block_size=0xFF00)
    fz = seqio.write_bgzf_fasta(os.path.join(tmp, "ref.fa.gz"), [(n, w.contigs[n]) for n in w.contigs])
    bed = os.path.join(tmp, "in.bed")
    open(bed, "w").write(synth.bed_text(w) * a.repeat)
    n_loci = a.distinct * a.repeat
    rec = {"source_id": _lib.load().vapor_source_id().decode(), "loci": n_loci, "distinct_loci": a.distinct,
           "fasta_mb": round(os.path.getsize(fa) / 1e6, 2), "fasta_gz_mb": round(os.path.getsize(fz) / 1e6, 2),
           "bam_mb": round(os.path.getsize(bam) / 1e6, 1), "write_s": round(time.perf_counter() - t0, 1), "ways": {}}

    # time spent reading windows: every fetch of the two host readers, and every device call
    spent = {"host_s": 0.0, "host_calls": 0, "device_s": 0.0, "device_calls": 0, "device_windows": 0, "device_ok": 0, "stats": []}

    def timed(fn, key):
        def wrapped(*x, **k):
            t = time.perf_counter()
            try:
                return fn(*x, **k)
            finally:
                spent[key + "_s"] += time.perf_counter() - t
                spent[key + "_calls"] += 1
        return wrapped
    seqio.FaiFasta.fetch = timed(seqio.FaiFasta.fetch, "host")
    seqio.BgzfFasta.fetch = timed(seqio.BgzfFasta.fetch, "host")
    dev_call = Engine.fasta_windows_device

    def dev_spy(self, *x, **k):
        t = time.perf_counter()
        got = dev_call(self, *x, **k)
        spent["device_s"] += time.perf_counter() - t
        spent["device_calls"] += 1
        spent["device_windows"] += len(got[0])
        spent["device_ok"] += int((got[2] == 0).sum())
        spent["stats"].append(self.fasta_last_stats())
        return got
    Engine.fasta_windows_device = dev_spy
    on_device = fastpath._device_fasta

    shas = {}
    for name, ref, dev in (("plain", fa, True), ("bgzf_device", fz, True), ("bgzf_host", fz, False)):
        if a.only and name not in a.only.split(","):
            continue
        fastpath._device_fasta = on_device if dev else (lambda *_x: None)
        out = os.path.join(tmp, "o_%s.vapor" % name)
        args = ["bed", "--sv-input", bed, "--reference", ref, "--pacbio-input", bam, "--output-path", tmp + "/f", "--output-file", out, "--no-figures"]
        with contextlib.redirect_stdout(io.StringIO()):
            cli.main(args)                                       # (warm: engines, pools, page cache)
        best, best_spent = 1e9, None
        for _ in range(a.reps):
            for k in spent:
                spent[k] = [] if k == "stats" else 0
            with contextlib.redirect_stdout(io.StringIO()):
                t = time.perf_counter()
                cli.main(args)
                dt = time.perf_counter() - t
            if dt < best:
                best, best_spent = dt, {k: (v if k != "stats" else v[-3:]) for k, v in spent.items()}
        shas[name] = hashlib.sha256(open(out, "rb").read()).hexdigest()[:16]
        r = {"loci_per_s": round(n_loci / best, 1), "run_s": round(best, 3), "table_sha16": shas[name],
             "host_window_s": round(best_spent["host_s"], 3), "host_window_calls": best_spent["host_calls"],
             "device_call_s": round(best_spent["device_s"], 3), "device_calls": best_spent["device_calls"],
             "device_windows": best_spent["device_windows"], "device_windows_ok": best_spent["device_ok"]}
        st = best_spent["stats"]
        if st:
            r["last_stats_of_last_calls"] = st
        rec["ways"][name] = r
        print("%-12s %8.1f loci/s  host windows %.3f s (%d fetches)  device %.3f s (%d calls, %d windows)" % (
            name, r["loci_per_s"], r["host_window_s"], r["host_window_calls"], r["device_call_s"], r["device_calls"], r["device_windows"]),
            file=sys.stderr, flush=True)
    rec["tables_identical"] = len(set(shas.values())) == 1
    ways = rec["ways"]
    if "plain" in ways and "bgzf_device" in ways:
        rec["device_vs_plain"] = round(ways["bgzf_device"]["loci_per_s"] / ways["plain"]["loci_per_s"], 3)
    if "plain" in ways and "bgzf_host" in ways:
        rec["host_vs_plain"] = round(ways["bgzf_host"]["loci_per_s"] / ways["plain"]["loci_per_s"], 3)
    d = os.environ.get("OUT", "profile_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "fasta_rate.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return 0 if rec["tables_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
