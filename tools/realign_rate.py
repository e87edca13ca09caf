"""What `--realign` costs on the files path: tools/evidence_rate.py's runs for its mode `ra` - one make_support_world written to
files, `vapor bed` and `vapor bed --realign` of this tree alternating, each in a warm process of its own, with --parent DIR the
plain run of another checkout (the parent commit, built; it has no `--realign`) in turn with them.
  python tools/realign_rate.py [n_loci] [--repeats R] [--parent DIR] [--bed-repeat K] [--layers N] [--timeout S] [--kernel-only]
  python tools/realign_rate.py --kernels DIR
--kernel-only: this tree's `--realign` run once, in this process - the program of a kernel trace, a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/realign_rate.py 120 --bed-repeat 4 --kernel-only
--kernels DIR: reads that trace's *kernel_stats.csv and prints realign_kernel's launches, its time per launch and its share of
the run's kernel time."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evidence_rate  # noqa: E402


def kernels(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % d)
    rows = list(csv.DictReader(open(files[-1])))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print("kernel trace %s: %d kernels, %.3f ms of kernel time" % (os.path.basename(files[-1]), len(rows), total / 1e6))
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]:
        name = r["Name"].split("(")[0]
        print("  %-60s %6d launches  %10.1f us a launch  (min %.1f, max %.1f)  %5.1f %% of the kernel time"
              % (name[:60], int(r["Calls"]), float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3, float(r.get("MinNs") or 0) / 1e3,
                 float(r.get("MaxNs") or 0) / 1e3, 100.0 * float(r["TotalDurationNs"]) / total))
    mine = [r for r in rows if "realign_kernel" in r["Name"]]
    if not mine:
        raise SystemExit("the trace holds no realign_kernel")
    t = sum(float(r["TotalDurationNs"]) for r in mine)
    n = sum(int(r["Calls"]) for r in mine)
    print("realign_kernel: %d launches, %.1f us a launch, %.1f %% of the run's kernel time" % (n, t / n / 1e3, 100.0 * t / total))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        kernels(sys.argv[2])
    else:
        sys.argv.insert(1, "ra")
        evidence_rate.main()
