"""The input parsers on the reference's OWN fixture files: vapor_test/vapor_test.vcf (44
records), vapor_test.bed and every simulate/Structural_Variants_{het,homo}/*.vcf|bed went through the reference's
vcf_list_readin / bed_info_readin (vapor_vali/vapor:22-50, 127-202) when tests/golden/parsers.json.gz was made
(oracle/gen_golden.py parsers); here they go through vapor_amd.cli's.  Compared: a digest of the returned structure - bucket
dict in first-seen order and record-index map for a VCF, the row list for a BED - or the exception type where the reference
raises (the 4-column BEDs: pin[4], vapor_vali/vapor:31; their 5-column re-expression parses).  Both the whole files
(tests/golden/parser_files.json.xz, the reference's fixture files verbatim, oracle/gen_golden.py parser_files) and their
first 300 lines (part of parsers.json.gz) are compared."""
import hashlib
import json
import lzma
import os

import pytest

from conftest import GOLDEN, load_golden

GOLD = load_golden("parsers.json.gz")
with lzma.open(os.path.join(GOLDEN, "parser_files.json.xz"), "rt") as _f:
    FILES = json.load(_f)["files"]


def _digest(obj) -> str:
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()


def _five_columns(text: str) -> str:
    out = []
    for n, line in enumerate(text.splitlines()):
        f = line.split()
        out.append("\t".join(f[:3] + ["sv%d" % (n + 1), f[3]]) if len(f) == 4 else line)
    return "\n".join(out) + "\n"


def _run(kind, text, tmp_path):
    from vapor_amd import cli
    path = tmp_path / ("in." + kind)
    path.write_text(text)
    try:
        if kind == "vcf":
            buckets, rec_hash = cli.vcf_list_readin(str(path))
            return {"digest": _digest([buckets, sorted([list(kv) for kv in rec_hash.items()])]),
                    "buckets": {k: len(v) for k, v in buckets.items()}, "records_keyed": len(rec_hash)}
        rows = cli.bed_info_readin(str(path), str(tmp_path / "figs") + "/")
        return {"digest": _digest(rows), "rows": len(rows)}
    except Exception as e:      # noqa: BLE001 - the reference's failure mode is part of the vector
        return {"error": type(e).__name__}


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["file"].replace("/", ":"))
def test_parsers_on_the_reference_fixture_files(case, tmp_path):
    kind = case["kind"]
    assert _run(kind, case["slice_text"], tmp_path) == case["slice"]
    if kind == "bed":
        assert _run(kind, _five_columns(case["slice_text"]), tmp_path) == case["slice_5col"]
    text = FILES[case["file"]]
    assert hashlib.sha256(text.encode()).hexdigest() == case["input_sha256"]
    assert _run(kind, text, tmp_path) == case["whole"]
    if kind == "bed":
        assert _run(kind, _five_columns(text), tmp_path) == case["whole_5col"]


def test_parser_fixture_covers_what_the_survey_names():
    files = [c["file"] for c in GOLD["cases"]]
    assert "vapor_test/vapor_test.vcf" in files and "vapor_test/vapor_test.bed" in files
    assert sum(f.startswith("simulate/Structural_Variants_het/") for f in files) >= 30
    assert sum(f.startswith("simulate/Structural_Variants_homo/") for f in files) >= 20
    v = [c for c in GOLD["cases"] if c["file"] == "vapor_test/vapor_test.vcf"][0]
    assert v["lines"] >= 44 and v["slice_lines"] == v["lines"] and sum(v["whole"]["buckets"].values()) >= 40
    # the shipped 4-column BED is what the reference can no longer read; re-expressed it parses
    b = [c for c in GOLD["cases"] if c["file"] == "vapor_test/vapor_test.bed"][0]
    assert b["whole"] == {"error": "IndexError"} and b["whole_5col"]["rows"] == 19
