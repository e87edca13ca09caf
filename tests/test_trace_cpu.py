"""`--realign-out` without a device: the numpy statement (realign.trace_statement) against the plain-integer model
(tests/trace_model.py) on every designed case, the model's mutants every one of which those cases tell from the rule at least
three times, the CIGAR text and the POS fold, the parser, the header's prototype and the export lists, the host arithmetic of the
call under the sanitizers as a program of its own (tools/trace_check.cpp), and cli.main on an engine whose `realign` and
`realign_trace` are the statements: the table of `--realign`, and SAM and FASTA exactly as the section spells them."""
import os
import re
import subprocess

import numpy as np
import pytest

import realign_model as RM
import test_realign_cpu as TR
import test_signature_cpu as TS
import trace_model as M
from conftest import ROOT
from vapor_amd import _lib as L
from vapor_amd import cli, modes, pipeline, realign, seqio, synth


# ------------------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_statement_equals_the_model_on_every_designed_case():
    cases, expect = M.designed_cases(), M.designed_expected()
    assert len(cases) == len(RM.designed_cases()) + len(M.own_cases()) and len(M.own_cases()) >= 40
    wrong = []
    for (name, r, a, o, band), e in zip(cases, expect):
        d, i_end, j_end, runs = realign.trace_statement(r, a, o, band)
        if (d, i_end, j_end, runs) != tuple(e[:4]) or realign.cigar_text(runs, len(r) - i_end) != e[4]:
            wrong.append((name, (d, i_end, j_end, runs), e))
        assert d == realign.statement(r, a, o, band), name
    assert not wrong, (len(wrong), wrong[:3])


def test_the_statement_equals_the_model_on_the_fuzz():
    for name, r, a, o, band in RM.fuzz_cases():
        e = M.trace(r, a, o, band)
        assert realign.trace_statement(r, a, o, band) == tuple(e[:4]), name


def test_the_rule_is_well_defined_on_every_designed_case():
    """X, I and D together cost exactly d; the runs consume i_end read symbols and j_end allele symbols; no two neighbours share
    an op; the end cell lies on the last row or the last column."""
    for (name, r, a, o, _band), (d, i_end, j_end, runs, cigar) in zip(M.designed_cases(), M.designed_expected()):
        n, m = len(r), len(a) - o
        assert sum(k for k, op in runs if op in "XID") == d, name
        assert sum(k for k, op in runs if op in "=XI") == i_end and sum(k for k, op in runs if op in "=XD") == j_end, name
        assert all(x[1] != y[1] and x[0] > 0 for x, y in zip(runs, runs[1:])), name
        assert (i_end == n or j_end == m) and 0 <= i_end <= n and 0 <= j_end <= m, name
        assert cigar == "*" or sum(int(k) for k, op in re.findall(r"(\d+)([=XIS])", cigar)) == n, name


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_is_told_from_the_rule_by_three_designed_cases(mutant):
    assert len(M.MUTANTS) == 5
    assert M.told_apart(mutant) >= 3, (mutant, M.told_apart(mutant))


def test_the_designed_cases_the_section_names_are_there():
    names = [c[0] for c in M.own_cases()]
    for word in ("leading D", "n = 0", "m = 0", "off2 == len(seq2)", "long clip", "row tie", "column tie", "vertical and horizontal tie"):
        assert sum(word in n for n in names) >= 2, word
    by = dict(zip((c[0] for c in M.designed_cases()), M.designed_expected()))
    assert by["leading D of 5 B=32"][3][0] == (5, "D") and by["leading D of 12 B=33"][3][0] == (12, "D")
    assert by["long clip m=40 B=2"][4] == "40=240S" and by["m = 0 B=32"][:5] == (0, 0, 0, [], "50S") and by["n = m = 0"][4] == "*"
    assert by["column tie, repeated tail"][1:3] == (10, 10) and by["row tie, repeated tail"][1:3] == (10, 10)


# ------------------------------------------------------------------------------------------------------------------------------
# CIGAR text, the POS fold, the allele a read is shown on
# ------------------------------------------------------------------------------------------------------------------------------
def test_cigar_text_and_the_leading_d_fold():
    runs = [(5, "D"), (19, "="), (1, "X"), (3, "I"), (2, "D"), (7, "=")]
    assert realign.fold_leading_d(runs) == (5, runs[1:]) and realign.fold_leading_d(runs[1:]) == (0, runs[1:])
    assert realign.fold_leading_d([]) == (0, []) and realign.fold_leading_d([(4, "D")]) == (4, [])
    assert realign.cigar_text(runs[1:], 0) == "19=1X3I2D7=" and realign.cigar_text(runs[1:], 9) == "19=1X3I2D7=9S"
    assert realign.cigar_text([], 0) == "*" and realign.cigar_text([], 50) == "50S"
    assert realign.aligned(runs) and not realign.aligned([(4, "D")]) and not realign.aligned([(2, "I"), (1, "D")]) and not realign.aligned([])
    head = np.asarray([3, 0, 30, 30, 2, 0, 0, 0], dtype=np.int32)
    words = np.asarray([99, 99, 20 << 2 | 0, 10 << 2 | 1], dtype=np.uint32)
    assert realign.runs_of(head, words) == [(20, "="), (10, "X")] and realign.runs_of(np.zeros(8, dtype=np.int32), words) == []
    assert realign.OPS == "=XID" == M.OPS


def test_the_allele_choice_and_the_vote_tag():
    m = realign.MARGIN
    assert [realign.fits_alt(v) for v in (m, m + 5, 1, 0, -1, -m)] == [True, True, True, False, False, False]
    assert [realign.vote_text(v) for v in (m, m - 1, 0, 1 - m, -m)] == ["ALT", "NC", "NC", "NC", "REF"]
    for v in range(-2 * m, 2 * m + 1):                   # (a voter is shown on the allele it votes for)
        assert realign.vote_text(v) != "ALT" or realign.fits_alt(v)
        assert realign.vote_text(v) != "REF" or not realign.fits_alt(v)


def test_a_sam_record():
    read = ("ACGTACGTAC", 7, 14, 2, 8, 11, [(3, "D"), (4, "="), (1, "X"), (3, "=")])
    line = realign.sam_record("c1:5:9:DEL", 3, read)
    assert line.split("\t") == ["c1:5:9:DEL/3", "0", "c1:5:9:DEL|ALT", "11", "255", "4=1X3=2S", "*", "0", "0", "ACGTACGTAC", "*", "NM:i:2",
                                "rd:i:14", "ad:i:2", "vt:Z:ALT"]
    on_ref = realign.sam_record("k", 0, ("ACGT", 0, 1, 1, 4, 4, [(4, "=")])).split("\t")
    assert on_ref[2] == "k|REF" and on_ref[3] == "1" and on_ref[11:] == ["NM:i:1", "rd:i:1", "ad:i:1", "vt:Z:NC"]
    assert realign.sam_record("k", 0, ("ACGT", 0, 4, 9, 0, 0, [])) is None
    assert realign.sam_record("k", 0, ("ACGT", 0, 4, 9, 4, 2, [(2, "D"), (4, "I")])) is None


def test_the_writer_orders_by_job_and_numbers_repeated_keys(tmp_path):
    def payload(ref, alt, reads):
        p = realign.Payload([r[2] - r[3] for r in reads])
        p.traces = realign.Traces(ref, alt, reads)
        return p
    w = realign.TraceWriter(str(tmp_path / "o"))
    w.take(5, "k:2", payload("ACGTACGT", "ACGT", [("ACGT", 0, 0, 0, 4, 4, [(4, "=")])]))
    w.take(1, "k:1", payload("AAAA", "AAAT", [("AAAT", 0, 1, 0, 4, 4, [(4, "=")]), ("GGGG", 0, 4, 4, 0, 0, [])]))
    w.take(3, "k:1", payload("CCCC", "CC", []))
    w.take(2, "none", None)
    w.take(4, "bare", realign.Payload([1]))
    assert w.close() == (str(tmp_path / "o.sam"), str(tmp_path / "o.fa"))
    assert (tmp_path / "o.fa").read_text() == ">k:1|REF\nAAAA\n>k:1|ALT\nAAAT\n>k:1#2|REF\nCCCC\n>k:1#2|ALT\nCC\n>k:2|REF\nACGTACGT\n>k:2|ALT\nACGT\n"
    sam = (tmp_path / "o.sam").read_text().splitlines()
    assert sam[0] == "@HD\tVN:1.6\tSO:unknown"
    assert sam[1:7] == ["@SQ\tSN:k:1|REF\tLN:4", "@SQ\tSN:k:1|ALT\tLN:4", "@SQ\tSN:k:1#2|REF\tLN:4", "@SQ\tSN:k:1#2|ALT\tLN:2",
                        "@SQ\tSN:k:2|REF\tLN:8", "@SQ\tSN:k:2|ALT\tLN:4"]
    assert [ln.split("\t")[:3] for ln in sam[7:]] == [["k:1/0", "0", "k:1|ALT"], ["k:2/0", "0", "k:2|REF"]]
    ranked = realign.TraceWriter(str(tmp_path / "o"), 2, 4)
    assert ranked.close() == (str(tmp_path / "o.rank2.sam"), str(tmp_path / "o.rank2.fa"))


# ------------------------------------------------------------------------------------------------------------------------------
# the parser
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_option_parses_and_the_help_text_is_unchanged(monkeypatch):
    p = cli.build_parser()
    assert p.parse_args(TR.BASE + ["--realign", "--realign-out", "pre"]).realign_out == "pre" and p.parse_args(TR.BASE).realign_out is None
    assert "--realign-out" not in cli.MODE_OPTIONS and len(cli.MODE_OPTIONS) == 9
    monkeypatch.setenv("COLUMNS", "80")
    with open(os.path.join(ROOT, "tests", "golden", "cli_help.txt")) as f:
        assert p.format_help() == f.read()
    assert "--realign-out" not in p.format_help() and "--realign-out" not in p.format_usage()
    assert modes.REALIGN.sink is None


def test_refused_without_realign_and_outside_bed_and_vcf(capsys):
    for cmd in ("bed", "vcf", "svelter", "ins"):
        TR._refused([cmd] + TR.BASE + ["--realign-out", "pre"], "--realign-out needs --realign", capsys)
    for cmd in ("svelter", "ins"):
        TR._refused([cmd] + TR.BASE + ["--realign", "--realign-out", "pre"], "--realign applies to `vapor bed` and `vapor vcf`", capsys)
    TR._refused(["bed"] + TR.BASE + ["--realign-out", "pre", "--support"], "--realign-out needs --realign", capsys)


# ------------------------------------------------------------------------------------------------------------------------------
# the entry, its binding and the host arithmetic of the call
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_bound():
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    assert re.search(r"\bint vapor_realign_trace\(vapor_ctx\* ctx, vapor_seqset\* set, int64_t n_pairs, const vapor_pair\* pairs, int32_t band,\s+"
                     r"int32_t cap_runs, int32_t\* head, uint32_t\* runs\);", h)
    assert "vapor_realign_trace" in L.EXPORTS and "vapor_realign_trace" in L.OPTIONAL_EXPORTS and L.ABI_VERSION == 3
    lib = L.load()
    assert hasattr(lib, "vapor_realign_trace") and len(lib.vapor_realign_trace.argtypes) == 8
    from vapor_amd import build
    assert any(p.endswith("vapor_realign_trace.h") for p in build.KERNEL_FILES) and any(p.endswith("vapor_trace_plan.h") for p in build.DEPS)
    stub = open(os.path.join(ROOT, "vapor_amd", "csrc", "vapor_bam.cpp")).read()
    assert re.search(r'__attribute__\(\(weak\)\) int vapor_realign_trace\(', stub)


def test_an_engine_without_the_entry_raises_one_clear_error(monkeypatch):
    from vapor_amd.engine import Engine

    class Without:
        def vapor_build_flags(self):
            return b""
    monkeypatch.setattr(L, "load", lambda: Without())
    e = object.__new__(Engine)
    assert e.realign_trace_available() is False
    with pytest.raises(NotImplementedError, match=r"vapor_realign_trace: the loaded library has no traceback kernel \(--realign-out\)"):
        Engine.realign_trace(e, None, np.zeros(0, dtype=L.PAIR_DTYPE), 256, 64)


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trace") / "trace_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"),
                           os.path.join(ROOT, "tools", "trace_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "words: 6 widths",
    "words and head: stated",
    "groups: 400 calls, many in several groups",
    "end slots: 4000 pairs",
    "trace_check: all equal",
])
def test_the_calls_host_arithmetic_against_direct_statements_under_sanitizers(check_output, line):
    assert line in check_output


# ------------------------------------------------------------------------------------------------------------------------------
# through cli.main, on an engine whose distances and traces are the statements'
# ------------------------------------------------------------------------------------------------------------------------------
_TRACED = {}


class TraceFake(TR.RealignFake):
    """RealignFake plus realign_trace: the statement over the set's texts, in the entry's layout, overflow status included."""

    def __init__(self, orc):
        super().__init__(orc)
        self.trace_calls = []            # per call: (pairs, cap_runs)

    def realign_trace(self, ss, pairs, band, cap_runs):
        self.trace_calls.append((len(pairs), cap_runs))
        head = np.zeros((len(pairs), 8), dtype=np.int32)
        runs = np.zeros((len(pairs), cap_runs), dtype=np.uint32)
        for t, p in enumerate(pairs):
            key = (ss.seqs[p["seq1"]], ss.seqs[p["seq2"]], int(p["off2"]), band)
            if key not in _TRACED:
                _TRACED[key] = realign.trace_statement(*key)
            d, i_end, j_end, rr = _TRACED[key]
            head[t, :5] = (d, 0 if len(rr) <= cap_runs else L.E_OVERFLOW, i_end, j_end, len(rr))
            if len(rr) <= cap_runs and rr:
                runs[t, cap_runs - len(rr):] = [k << 2 | realign.OPS.index(op) for k, op in rr]
        return head, runs


@pytest.fixture()
def fake(oracle):
    eng = TraceFake(oracle)
    pipeline.set_engine(eng)
    yield eng
    pipeline.set_engine(None)
    seqio.set_backend(None)


SPECS = (("DEL", 600, "hom"), ("DEL", 600, "ref"), ("DEL", 600, "het"), ("INS", 250, "hom"), ("INV", 700, "hom"), ("TANDUP", 300, "hom"))


def check_files(sam_text, fa_text, table_rows):
    """SAM and FASTA as the section spells them; returns the records as lists of fields."""
    fa = fa_text.splitlines()
    assert len(fa) % 4 == 0 and all(ln.startswith(">") for ln in fa[0::2])
    entries = [(ln[1:], len(seq)) for ln, seq in zip(fa[0::2], fa[1::2])]
    assert all(a[0].endswith("|REF") and b[0].endswith("|ALT") and a[0][:-4] == b[0][:-4] for a, b in zip(entries[0::2], entries[1::2]))
    sam = sam_text.splitlines()
    assert sam[0] == "@HD\tVN:1.6\tSO:unknown"
    assert sam[1:1 + len(entries)] == ["@SQ\tSN:%s\tLN:%d" % e for e in entries]
    length = dict(entries)
    keys = [e[0][:-4] for e in entries[0::2]]
    assert keys == [k for k in table_rows if k in keys]                   # job order
    records = [ln.split("\t") for ln in sam[1 + len(entries):]]
    seq_of = {ln[1:]: seq for ln, seq in zip(fa[0::2], fa[1::2])}
    for f in records:
        assert len(f) == 15 and not f[0].startswith("@")
        key, index = f[0].rsplit("/", 1)
        assert key in keys and int(index) >= 0 and f[1] == "0" and f[2] in (key + "|ALT", key + "|REF") and f[4] == "255"
        assert f[6:9] == ["*", "0", "0"] and f[10] == "*"
        ops = [(int(k), op) for k, op in re.findall(r"(\d+)([=XIDS])", f[5])]
        assert "".join("%d%s" % o for o in ops) == f[5] and ops[0][1] != "D" and all(op != "S" for _k, op in ops[:-1])
        assert sum(k for k, op in ops if op in "=XIS") == len(f[9])                                   # the CIGAR consumes its read
        assert int(f[3]) >= 1 and int(f[3]) - 1 + sum(k for k, op in ops if op in "=XD") <= length[f[2]]      # ... inside its @SQ
        tags = dict(t.split(":", 1) for t in f[11:])
        assert list(tags) == ["NM", "rd", "ad", "vt"]
        rd, ad = int(tags["rd"][2:]), int(tags["ad"][2:])
        assert tags["vt"] == "Z:" + realign.vote_text(rd - ad) and f[2].endswith("|ALT") == realign.fits_alt(rd - ad)
        assert int(tags["NM"][2:]) == (ad if f[2].endswith("|ALT") else rd)
        # the record says what it claims: walking the CIGAR over the allele, '=' are matches, 'X' are not, and NM counts X, I, D
        # (a leading D folded into POS is part of d)
        a, b, pa, pb, cost = f[9], seq_of[f[2]], 0, int(f[3]) - 1, 0
        for k, op in ops:
            if op in "=X":
                same = [RM.matches(RM.code(ord(x)), RM.code(ord(y))) for x, y in zip(a[pa:pa + k], b[pb:pb + k])]
                assert len(same) == k and all(same) == (op == "=") and (op == "=" or not any(same)), (f[0], f[5])
                pa, pb = pa + k, pb + k
            elif op == "I":
                pa += k
            elif op == "D":
                pb += k
            cost += k if op in "XID" else 0
        assert cost <= int(tags["NM"][2:])
    return records


def test_cli_on_a_world_in_memory(fake, tmp_path):
    w = synth.make_support_world(seed=4, specs=SPECS, layers=4, read_len=4000)
    text = synth.bed_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    plain, _ = TS.run_main(tmp_path, "ra", "bed", text, ["--realign"])
    # a run without --realign-out never calls realign_trace
    assert fake.realign_calls and not fake.trace_calls
    files = {}
    for name, more in (("whole", []), ("one", ["--chunk", "1"])):
        fake.trace_calls.clear()
        seqio.set_backend(seqio.MemorySamtools(w))
        pre = str(tmp_path / (name + "_pre"))
        table, _ = TS.run_main(tmp_path, name, "bed", text, ["--realign", "--realign-out", pre] + more)
        assert table == plain                                             # the table is --realign's, byte for byte
        assert fake.trace_calls
        files[name] = (open(pre + ".sam").read(), open(pre + ".fa").read())
        assert sorted(os.listdir(str(tmp_path))).count(name + "_pre.sam") == 1
    assert files["whole"] == files["one"]                                 # neither threads nor chunking show
    rows = [r.split("\t") for r in plain.splitlines()[1:]]
    keys = [":".join(str(v) for v in r[:3]) for r in rows]
    sam, fa = files["whole"]
    records = check_files(sam, fa, [e[1:-4] for e in fa.splitlines()[0::4]])
    names = [ln[1:] for ln in fa.splitlines()[0::2]]
    assert len(names) == 2 * len(SPECS) and all(any(n.startswith(k + ":") for n in names) for k in keys), (names, keys)
    # every read of the table's VaPoR_RA_Rec is a record (these reads all align), with the table's diff, in read order
    at = 0
    for r, name in zip(rows, names[0::2]):
        diffs = [int(v) for v in r[-1].split(",")]
        mine = records[at:at + len(diffs)]
        at += len(diffs)
        assert [f[0] for f in mine] == ["%s/%d" % (name[:-4], k) for k in range(len(diffs))]
        assert [int(f[12][5:]) - int(f[13][5:]) for f in mine] == diffs
    assert at == len(records)
    # the hom DEL locus: every ALT-voting read lies on |ALT with no D or I run of 50 or more; on |REF it would carry the event
    first = [f for f in records if f[0].startswith(names[0][:-4] + "/")]
    assert first and all(f[14] != "vt:Z:ALT" or (f[2].endswith("|ALT") and not [k for k, op in re.findall(r"(\d+)([ID])", f[5]) if int(k) >= 50])
                         for f in first) and any(f[14] == "vt:Z:ALT" for f in first)
    # a modest first cap, and one more call for what overflowed
    caps = [c for _n, c in fake.trace_calls]
    assert caps[0] == realign.FIRST_CAP_RUNS and all(c >= realign.FIRST_CAP_RUNS for c in caps)
    # a locus without a payload writes nothing
    seqio.set_backend(seqio.MemorySamtools(w))
    pre = str(tmp_path / "few_pre")
    TS.run_main(tmp_path, "few", "bed", text, ["--realign", "--realign-out", pre, "--PB-supp", "1000"])
    assert open(pre + ".fa").read() == "" and open(pre + ".sam").read() == "@HD\tVN:1.6\tSO:unknown\n"


def test_cli_vcf_writes_the_same_alignments(fake, tmp_path):
    w = synth.make_support_world(seed=4, specs=SPECS[:3], layers=4, read_len=4000)
    seqio.set_backend(seqio.MemorySamtools(w))
    plain, annotated_plain = TS.run_main(tmp_path, "ra", "vcf", synth.vcf_text(w), ["--realign"])
    seqio.set_backend(seqio.MemorySamtools(w))
    pre = str(tmp_path / "pre")
    table, annotated = TS.run_main(tmp_path, "out", "vcf", synth.vcf_text(w), ["--realign", "--realign-out", pre])
    assert table == plain and annotated == annotated_plain
    keys = [r.split("\t")[0] for r in table.splitlines()[1:]]
    records = check_files(open(pre + ".sam").read(), open(pre + ".fa").read(), keys)
    assert records and {f[0].rsplit("/", 1)[0] for f in records} <= set(keys)
