"""The extra-columns modes (vapor_amd/modes.py: `--refine`, `--phased`, `--both-ends`) as cli.py and the VCF writer see them: one
surface for all three - the payload's round trip through the gather's floats, columns against ##INFO lines, the ##INFO text
itself and the INFO keys of a record - and the option combinations the parser refuses.  No engine is needed."""
import re

import pytest

from vapor_amd import cli, modes
from vapor_amd import simple_function as SF

NAN = float("nan")
MODES = {"refine": modes.refine(50, 10), "phased": modes.PHASED, "both-ends": modes.BOTH_ENDS}
PAYLOADS = {"refine": [[880.0, 2285.0, 0.4, 0.75, 6.0], [880.0, 2285.0, NAN, NAN, 0.0]],
            "phased": [(True, 7, [0.5, -1.0], None), (False, None, None, [1.0])],
            "both-ends": [[[0.5], None, [], [1.0, -2.0]]]}
REFINE_LINES = [
    '##INFO=<ID=VaPoR_RPOS,Number=1,Type=Integer,Description="Start of the best-scoring candidate breakpoint pair (--refine)">',
    '##INFO=<ID=VaPoR_REND,Number=1,Type=Integer,Description="End of the best-scoring candidate breakpoint pair (--refine)">',
    '##INFO=<ID=VaPoR_QS0,Number=1,Type=Float,Description="VaPoR_QS of the called breakpoints on the widened window (--refine)">',
    '##INFO=<ID=VaPoR_GS0,Number=1,Type=Float,Description="VaPoR_GS of the called breakpoints on the widened window (--refine)">',
]
NUMBER_DOT = {"refine": set(), "phased": {"VaPoR_H1_Rec", "VaPoR_H2_Rec"}, "both-ends": {"VaPoR_BE_Rec", "VaPoR_BE_SQS"}}
TYPES = {"refine": ["Integer", "Integer", "Float", "Float"],
         "phased": ["Integer", "String"] + ["Float"] * 7,
         "both-ends": ["Integer", "Float", "Float", "String", "Float", "Float", "String"]}


def _same(a, b):
    """== with nan == nan."""
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
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
    assert m.attr == {"refine": "info", "phased": "phase", "both-ends": "views"}[name]
    if name == "refine":
        assert m.keys == ("VaPor_RPOS", "VaPor_REND", "VaPor_QS0", "VaPor_GS0") and not m.skip_dot and m.margin_step == (50, 10)
        assert m.columns_many(PAYLOADS[name]) == [["880", "2285", "0.4", "0.75"], ["880", "2285", "NA", "NA"]]
    else:
        assert tuple(m.keys) == tuple(m.COLUMNS) and m.skip_dot
    assert m.phased == (name == "phased")


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
