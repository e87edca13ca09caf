#!/usr/bin/env python3
"""What `vapor bed | vcf --realign` writes under every legal combination of --realign-out, --realign-polish, --realign-junction
and --realign-revote, as SHA-256 digests: tests/golden/realign_options.json, names and digests only.

TEST INFRASTRUCTURE.  Nothing but the command line is used (cli.main and its argument list), so that the same script runs on
any commit that has the four options: the file is written on the commit BEFORE a change that must not move an output byte, and
tests/test_realign_options_cpu.py compares the tree's own runs with it.  The world, the reads and the engine are the ones
tests/test_revote_cpu.py runs on: synth.make_support_world(seed=4, specs=test_polish_cpu.SPECS, layers=4, read_len=4000) in
memory, and an engine whose distances, traces, piles, junctions and second votes are the Python statements.  `bed` runs for all
ten combinations, `vcf` for the fullest one.

    python tools/gen_realign_options_golden.py          # writes the file
"""
from __future__ import annotations

import contextlib
import hashlib
import io
import itertools
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NAME = "realign_options.json"
FLAGS = ("--realign-polish", "--realign-junction", "--realign-revote")
EXTS = (".fa", ".sam", ".pol.fa")


def combinations():
    """The ten legal ones as (name, flags, with --realign-out), the order of the file."""
    out = []
    for pol, jun, rev in itertools.product((False, True), repeat=3):
        if (jun or rev) and not pol:
            continue
        flags = [f for f, on in zip(FLAGS, (pol, jun, rev)) if on]
        for files in (False, True):
            out.append((" ".join(["--realign"] + flags + (["--realign-out"] if files else [])), flags, files))
    return out


def _sha(text) -> str:
    return hashlib.sha256(text if isinstance(text, bytes) else text.encode()).hexdigest()


def digests(tmp_path=None):
    """{run: {what: sha256}} of every run, on the engine and the world named above."""
    import test_polish_cpu as TP
    import test_revote_cpu as TRV
    import test_signature_cpu as TS
    from oracle import oracle as orc
    from vapor_amd import pipeline, seqio, synth
    orc.build()
    orc.lib()
    tmp = pathlib.Path(tmp_path if tmp_path is not None else tempfile.mkdtemp())
    w = synth.make_support_world(seed=4, specs=TP.SPECS, layers=4, read_len=4000)
    texts = {"bed": synth.bed_text(w), "vcf": synth.vcf_text(w)}
    pipeline.set_engine(TRV.RevoteFake(orc))
    got = {}
    try:
        runs = [("bed",) + c for c in combinations()] + [("vcf",) + combinations()[-1]]
        for k, (cmd, name, flags, files) in enumerate(runs):
            pre = str(tmp / ("pre%d" % k))
            seqio.set_backend(seqio.MemorySamtools(w))
            with contextlib.redirect_stdout(io.StringIO()):               # (`vapor bed` prints its rows)
                table, annotated = TS.run_main(tmp, "run%d" % k, cmd, texts[cmd],
                                               ["--realign"] + flags + (["--realign-out", pre] if files else []))
            mine = got["%s %s" % (cmd, name)] = {"table": _sha(table)}
            if annotated is not None:
                mine["annotated"] = _sha(annotated)
            for ext in EXTS:
                if os.path.exists(pre + ext):
                    mine[ext] = _sha(open(pre + ext, "rb").read())
    finally:
        pipeline.set_engine(None)
        seqio.set_backend(None)
    return got


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", NAME)
    with open(path, "w") as f:
        json.dump(digests(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d runs" % (path, len(json.load(open(path)))))
