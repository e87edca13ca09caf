"""The extra-columns modes (vapor_amd/modes.py: `--refine`, `--phased`, `--both-ends`, `--depth`, `--signatures`, `--links`,
`--support`) as cli.py and the VCF writer see them: one surface for all seven - the payload's round trip through the gather's
floats, columns against ##INFO lines, the ##INFO text itself, the INFO keys of a record and the chunk hooks - and the option
combinations the parser refuses, every message written out, with the parser's help text against a recording.  No engine is
needed."""
import itertools
import os
import re

import pytest

from vapor_amd import cli, depth, links, modes, signature, support
from vapor_amd import simple_function as SF

NAN = float("nan")
MODES = {"refine": modes.refine(50, 10), "phased": modes.PHASED, "both-ends": modes.BOTH_ENDS, "depth": modes.DEPTH,
         "signatures": modes.SIGNATURES, "links": modes.LINKS, "support": modes.SUPPORT}
EVIDENCE = {"depth": depth, "signatures": signature, "links": links, "support": support}      # the modes of a chunk hook, their rule modules
PAYLOADS = {"refine": [[880.0, 2285.0, 0.4, 0.75, 6.0], [880.0, 2285.0, NAN, NAN, 0.0]],
            "phased": [(True, 7, [0.5, -1.0], None), (False, None, None, [1.0])],
            "both-ends": [[[0.5], None, [], [1.0, -2.0]]],
            "depth": [depth.Payload([37000, 80000, 16000, 2000], "TANDUP"), depth.Payload([0, 300, 0, 0])],
            "signatures": [signature.Payload([3, 4, 5, -2, 3, 1, 2], "INS", 880, 880), signature.Payload([0] * 7, "INV", 100, 22000)],
            "links": [links.Payload([3, 4, 2, 2, 1, 3, -5, 1], 2000, 3000), links.Payload([0] * 8, 1, 1 << 31)],
            "support": [support.Payload([2, 1, 3, 0, 4, 7, 9], "INV", 100, 900), support.Payload([0] * 7, "TANDUP", 5, 6)]}
REFINE_LINES = [
    '##INFO=<ID=VaPoR_RPOS,Number=1,Type=Integer,Description="Start of the best-scoring candidate breakpoint pair (--refine)">',
    '##INFO=<ID=VaPoR_REND,Number=1,Type=Integer,Description="End of the best-scoring candidate breakpoint pair (--refine)">',
    '##INFO=<ID=VaPoR_QS0,Number=1,Type=Float,Description="VaPoR_QS of the called breakpoints on the widened window (--refine)">',
    '##INFO=<ID=VaPoR_GS0,Number=1,Type=Float,Description="VaPoR_GS of the called breakpoints on the widened window (--refine)">',
]
NUMBER_DOT = {"refine": set(), "phased": {"VaPoR_H1_Rec", "VaPoR_H2_Rec"}, "both-ends": {"VaPoR_BE_Rec", "VaPoR_BE_SQS"},
              "depth": set(), "signatures": set(), "links": set(), "support": set()}
TYPES = {"refine": ["Integer", "Integer", "Float", "Float"],
         "phased": ["Integer", "String"] + ["Float"] * 7,
         "both-ends": ["Integer", "Float", "Float", "String", "Float", "Float", "String"],
         "depth": ["Float", "Float", "Float", "Integer"], "signatures": ["Integer"] * 6, "links": ["Integer"] * 7,
         "support": ["Integer"] * 6 + ["Float", "String", "Integer"]}


def _same(a, b):
    """== with nan == nan, and with what a payload carries beside its list (a type, two coordinates)."""
    if isinstance(a, (list, tuple)):
        return (type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
                and getattr(a, "__dict__", None) == getattr(b, "__dict__", None))
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


@pytest.mark.parametrize("name", list(MODES))
def test_payload_round_trip_and_columns(name):
    m = MODES[name]
    assert m.name == name and m.pack(None) == [] and m.unpack(m.pack(None)) is None and m.unpack([]) is None
    for x in PAYLOADS[name]:
        flat = m.pack(x)
        assert flat and all(isinstance(v, float) for v in flat)
        assert _same(m.unpack(flat), x), x
        assert len(m.columns_many([x, None])[0]) == len(m.COLUMNS)
    assert len(m.COLUMNS) == len(m.INFO) == len(m.keys) == len(m.columns_many([None])[0])
    assert m.columns_many([None])[0] == ["."] * len(m.COLUMNS)
    assert [i[0] for i in m.INFO] == list(m.COLUMNS)
    assert all(len(i) == 4 for i in m.INFO)
    assert m.attr == {"refine": "info", "phased": "phase", "both-ends": "views"}.get(name, name)
    if name == "refine":
        assert m.keys == ("VaPor_RPOS", "VaPor_REND", "VaPor_QS0", "VaPor_GS0") and not m.skip_dot and m.margin_step == (50, 10)
        assert m.columns_many(PAYLOADS[name]) == [["880", "2285", "0.4", "0.75"], ["880", "2285", "NA", "NA"]]
    else:
        assert tuple(m.keys) == tuple(m.COLUMNS) and m.skip_dot
    assert m.phased == (name == "phased")


class _Job:
    """What a chunk hook reads of a cli.Job."""
    def __init__(self, spec=None, ctx=None, bnd=None):
        self.spec, self.ctx, self.bnd = spec, ctx, bnd


def hook_payloads(mode):
    """{type: payload} of a mode's chunk_payloads hook over one locus of every kind a chunk holds - the four simple types, one
    that has no spec's measure (DISDUP), a breakend, a row of fixed scores (None) - from a pattern that matches no file: every
    locus the hook answers for has a payload of zeros."""
    from vapor_amd import seqio
    ctx = (3, "/nowhere/readsXXX.bam", "r.fa")
    types = ["DEL", "TANDUP", "INV", "INS", "DISDUP", "BND", None]
    jobs = [_Job((t, "c", 5001, 5001 if t == "INS" else 5600, "ACGT" * 20 if t == "INS" else ""), ctx) for t in types[:5]]
    jobs += [_Job(bnd=(["c", 5000, "d", 700, "3to5", ""], ctx)), _Job()]

    class NoFile:
        def isfile(self, path):
            return False

        def contig_length(self, *a):
            raise AssertionError("a pattern without files has no contig to ask")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(seqio, "_backend", NoFile())
        mp.setattr(os, "listdir", lambda d: [])
        got = mode.chunk_payloads(jobs, list(range(len(jobs))), None)
    return {types[t]: p for t, p in got.items()}


@pytest.mark.parametrize("name", list(MODES))
def test_chunk_hooks(name):
    """An evidence mode's payload is its chunk's: it has a chunk_payloads hook and no chunk_gens; of the three older modes only
    --both-ends has a hook, chunk_gens.  The hook answers for its module's types and for no other."""
    m = MODES[name]
    if name not in EVIDENCE:
        assert m.chunk_payloads is None and (m.chunk_gens is None) == (name != "both-ends")
        return
    mod = EVIDENCE[name]
    assert callable(m.chunk_payloads) and m.chunk_gens is None
    assert mod.TYPES == {"depth": ("DEL", "TANDUP"), "signatures": ("DEL", "TANDUP", "INV", "INS"), "links": ("DEL", "TANDUP", "INV", "BND"),
                         "support": ("DEL", "TANDUP", "INV", "INS")}[name]
    got = hook_payloads(m)
    assert tuple(got) == mod.TYPES
    for ty, p in got.items():
        assert type(p) is mod.Payload and m.columns_many([p])[0][0] in ("0", ".") and not any(list(p)[:3]), (ty, p)


@pytest.mark.parametrize("name", list(MODES))
def test_info_lines_and_record_keys_of_the_annotated_vcf(name, tmp_path):
    m = MODES[name]
    vcf = tmp_path / "in.vcf"
    vcf.write_text('##fileformat=VCFv4.1\n##INFO=<ID=SVTYPE,Number=1,Type=String,Description="t">\n##source=x\n'
                   "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
                   "c1\t100\ta\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=500\nc1\t900\tb\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=990\n")
    values = ["v%d" % k for k in range(len(m.COLUMNS))]
    table = "\t".join(["#CHR"] * 10 + list(m.COLUMNS)) + "\n"
    table += "\t".join(["c1:100:500:DEL", "0.5", "0.25", "0/1", "1.5", "0.5,-1.0"] + values) + "\n"
    table += "\t".join(["c1:900:990:DEL", "0.5", "0.25", "0/1", "1.5", "0.5,-1.0"] + ["."] * len(m.COLUMNS)) + "\n"
    (tmp_path / "in.vcf.vapor").write_text(table)
    SF.vcf_vapor_modify(str(vcf), {"c1:100:500:DEL": [4], "c1:900:990:DEL": [5]}, mode=m)
    with_mode = (tmp_path / "in.vcf.vapor").read_text().splitlines()
    (tmp_path / "in.vcf.vapor").write_text(table)
    SF.vcf_vapor_modify(str(vcf), {"c1:100:500:DEL": [4], "c1:900:990:DEL": [5]})
    plain = (tmp_path / "in.vcf.vapor").read_text().splitlines()
    new = [ln for ln in with_mode if ln not in plain and ln.startswith("##")]
    at = with_mode.index(new[0])
    assert with_mode[at - 1].startswith("##INFO=<ID=VaPoR_REC,") and with_mode[at:at + len(new)] == new     # behind the row's own four
    got = [re.fullmatch(r'##INFO=<ID=(\w+),Number=([1.]),Type=(\w+),Description="([^"]+)">', ln).groups() for ln in new]
    assert [g[0] for g in got] == list(m.COLUMNS)
    assert {g[0] for g in got if g[1] == "."} == NUMBER_DOT[name] and all(g[1] in "1." for g in got)
    assert [g[2] for g in got] == TYPES[name]
    assert all(g[3].endswith("(--%s)" % name) for g in got)
    if name == "refine":
        assert new == REFINE_LINES
    # the records: the mode's keys behind the row's own, a '.' written by --refine and left out by the other two
    recs = [ln.split("\t") for ln in with_mode if not ln.startswith("#")]
    recs_plain = [ln.split("\t") for ln in plain if not ln.startswith("#")]
    assert len(recs) == 2 and [r[7] for r in recs_plain] == [r[7].split(";" + m.keys[0] + "=")[0] for r in recs]
    assert recs[0][7][len(recs_plain[0][7]):] == "".join(";%s=%s" % kv for kv in zip(m.keys, values))
    assert recs[1][7][len(recs_plain[1][7]):] == ("".join(";%s=." % k for k in m.keys) if name == "refine" else "")


BASE = ["--sv-input", "a.bed", "--reference", "r.fa", "--pacbio-input", "x.bam", "--output-path", "o", "--output-file", "o.vapor"]
# a run has one mode: the options that make one, as they are given, and what the parser says to every pair of them - written out
# from the parser as it was before the refusals became one table, not computed with it
GIVEN = {"--refine": ["--refine", "20"], "--phase-vcf": ["--phase-vcf", "p.vcf"], "--phased": ["--phased"], "--both-ends": ["--both-ends"],
         "--depth": ["--depth"], "--signatures": ["--signatures"], "--links": ["--links"], "--support": ["--support"]}
ONE = "(a run has one mode)"
HAP = "cannot be combined (refinement per haplotype is not implemented)"
TAGS = "cannot be combined (right-anchored reads are not read with their tags)"
PAIRS = {
    ("--refine", "--phase-vcf"): "--phased and --refine " + HAP,
    ("--refine", "--phased"): "--phased and --refine " + HAP,
    ("--refine", "--both-ends"): "--both-ends and --refine cannot be combined (refined candidates are scored from one side)",
    ("--refine", "--depth"): "--depth and --refine cannot be combined (depth is measured over the called breakpoints)",
    ("--refine", "--signatures"): "--signatures and --refine cannot be combined " + ONE,
    ("--refine", "--links"): "--links and --refine cannot be combined " + ONE,
    ("--refine", "--support"): "--support and --refine cannot be combined " + ONE,
    # (the same mode with another source of tags: no pair - the file is then asked for)
    ("--phase-vcf", "--phased"): "--phase-vcf: [Errno 2] No such file or directory: 'p.vcf'",
    ("--phase-vcf", "--both-ends"): "--both-ends and --phased " + TAGS,
    ("--phase-vcf", "--depth"): "--depth and --phase-vcf cannot be combined (depth is not measured per haplotype)",
    ("--phase-vcf", "--signatures"): "--signatures and --phase-vcf cannot be combined (signatures are not counted per haplotype)",
    ("--phase-vcf", "--links"): "--links and --phase-vcf cannot be combined (links are not counted per haplotype)",
    ("--phase-vcf", "--support"): "--support and --phase-vcf cannot be combined " + ONE,
    ("--phased", "--both-ends"): "--both-ends and --phased " + TAGS,
    ("--phased", "--depth"): "--depth and --phased cannot be combined (depth is not measured per haplotype)",
    ("--phased", "--signatures"): "--signatures and --phased cannot be combined (signatures are not counted per haplotype)",
    ("--phased", "--links"): "--links and --phased cannot be combined (links are not counted per haplotype)",
    ("--phased", "--support"): "--support and --phased cannot be combined " + ONE,
    ("--both-ends", "--depth"): "--depth and --both-ends cannot be combined " + ONE,
    ("--both-ends", "--signatures"): "--signatures and --both-ends cannot be combined " + ONE,
    ("--both-ends", "--links"): "--links and --both-ends cannot be combined " + ONE,
    ("--both-ends", "--support"): "--support and --both-ends cannot be combined " + ONE,
    ("--depth", "--signatures"): "--signatures and --depth cannot be combined " + ONE,
    ("--depth", "--links"): "--links and --depth cannot be combined " + ONE,
    ("--depth", "--support"): "--support and --depth cannot be combined " + ONE,
    ("--signatures", "--links"): "--links and --signatures cannot be combined " + ONE,
    ("--signatures", "--support"): "--support and --signatures cannot be combined " + ONE,
    ("--links", "--support"): "--support and --links cannot be combined " + ONE,
}
ALONE = {"--refine": "--refine", "--phase-vcf": "--phased", "--phased": "--phased", "--both-ends": "--both-ends", "--depth": "--depth",
         "--signatures": "--signatures", "--links": "--links", "--support": "--support"}       # the name the sub-command rule speaks of
TRIPLES = [
    (["--depth", "--signatures", "--links"], "--signatures and --depth cannot be combined " + ONE),
    (["--links", "--support", "--refine", "20"], "--links and --refine cannot be combined " + ONE),
    (["--phase-vcf", "p.vcf", "--depth", "--both-ends"], "--both-ends and --phased " + TAGS),
]


def _refused(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and err.startswith("usage: vapor ") and err.endswith("\nvapor: error: %s\n" % message), (argv, err)


def test_every_pair_of_mode_options_is_refused_in_its_own_words(capsys):
    assert len(PAIRS) == 28 and set(PAIRS) == set(itertools.combinations(GIVEN, 2))
    for (a, b), message in PAIRS.items():
        for cmd in ("bed", "vcf"):
            _refused([cmd] + BASE + GIVEN[a] + GIVEN[b], message, capsys)
            _refused([cmd] + BASE + GIVEN[b] + GIVEN[a], message, capsys)


def test_a_mode_option_applies_to_bed_and_vcf_only(capsys):
    for opt, spoken in ALONE.items():
        for cmd in ("svelter", "ins"):
            _refused([cmd] + BASE + GIVEN[opt], "%s applies to `vapor bed` and `vapor vcf`" % spoken, capsys)
    # the sub-command's refusal comes first within an option's block
    _refused(["svelter"] + BASE + ["--depth", "--refine", "20"], "--refine applies to `vapor bed` and `vapor vcf`", capsys)
    _refused(["ins"] + BASE + ["--both-ends", "--support"], "--both-ends applies to `vapor bed` and `vapor vcf`", capsys)
    _refused(["ins"] + BASE + ["--signatures", "--links"], "--signatures applies to `vapor bed` and `vapor vcf`", capsys)


@pytest.mark.parametrize("more, message", TRIPLES)
def test_three_mode_options_the_first_block_that_fires_speaks(more, message, capsys):
    for cmd in ("bed", "vcf"):
        _refused([cmd] + BASE + more, message, capsys)


def test_help_text_is_the_recording(monkeypatch):
    monkeypatch.setenv("COLUMNS", "80")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_help.txt")) as f:
        assert cli.build_parser().format_help() == f.read()



@pytest.mark.parametrize("cmd, more, message", [
    ("bed", ["--refine", "20", "--phased"], "--phased and --refine cannot be combined"),
    ("bed", ["--both-ends", "--refine", "20"], "--both-ends and --refine cannot be combined"),
    ("vcf", ["--both-ends", "--phased"], "--both-ends and --phased cannot be combined"),
    ("bed", ["--phase-sample", "S"], "--phase-sample names a sample of --phase-vcf"),
    ("svelter", ["--both-ends"], "--both-ends applies to `vapor bed` and `vapor vcf`"),
    ("ins", ["--refine", "20"], "--refine applies to `vapor bed` and `vapor vcf`"),
])
def test_refused_option_combinations(cmd, more, message, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main([cmd] + BASE + more)
    assert e.value.code == 2 and message in capsys.readouterr().err
