"""`--realign-revote` without a device: the numpy statement (revote.statement) against the plain-integer model
(tests/revote_model.py) on every designed locus and a seeded fuzz, `spell` against the codes of polish.apply's text, the model's
nine mutants every one of which is told from the rule at least three times, the columns, their gate and their round trip, the
parser, the header's prototype and the export lists, the host plan of the call under the sanitizers as a program of its own
(tools/revote_check.cpp), and cli.main on an engine whose entries are the statements."""
import os
import re
import subprocess

import numpy as np
import pytest

import plane_model as PM
import polish_model as PMOD
import revote_model as M
import test_junction_cpu as TJ
import test_polish_cpu as TP
import test_realign_cpu as TR
import test_signature_cpu as TS
from conftest import ROOT
from vapor_amd import _lib as L
from vapor_amd import cli, junction, pipeline, polish, realign, revote, seqio, synth


# ------------------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------------------
def arrays(pol):
    """polish_model's calls, sites and texts in the shape Engine.realign_polish gives them."""
    _counts, calls, sites, ins, _stats = pol
    s = np.zeros((polish.MAX_SITES, 2), dtype=np.int32)
    x = np.zeros((polish.MAX_SITES, polish.RMAX), dtype=np.uint8)
    for k, (site, text) in enumerate(zip(sites, ins)):
        s[k] = site
        x[k, :len(text)] = list(text)
    return np.asarray(calls, dtype=np.uint8), s, x


def stated(locus, pol):
    """revote.statement in the model's shape."""
    _name, _pairs, votes, allele, band = locus
    lout, vout, spelt, own = revote.statement([(r.decode("latin-1"), o) for r, o in votes], allele.decode("latin-1"), *arrays(pol), band)
    return lout.tolist(), vout.tolist(), spelt.tolist(), own.tolist()


def test_the_constants_are_the_models_and_the_headers():
    assert (M.MARGIN, M.MIN_COV, M.RMAX, M.MAX_SITES, M.MAX_SEQ_LEN, M.E_ARG) == (realign.MARGIN, polish.MIN_COV, polish.RMAX, polish.MAX_SITES,
                                                                                 L.MAX_SEQ_LEN, L.E_ARG)
    assert revote.E_ARG == L.E_ARG
    h = open(os.path.join(ROOT, "vapor_amd", "csrc", "vapor_revote_plan.h")).read()
    assert "enum VoutField { V_D = 0, V_STATUS = 1, V_OFF2 = 2, V_M = 3 };" in h and "enum LoutField { L_STATUS = 0, L_PLEN = 1 };" in h
    for text in (b"ACGTacgtNnRrYy*-x", bytes(range(256))):
        assert revote.codes_of(text).tolist() == PM.codes(text).tolist() == [M.rm.code(v) for v in text]
        assert revote.codes_of(text, True).tolist() == PM.codes(text, True).tolist()
    assert revote.codes_of(revote.text_of([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15])).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15]
    assert [M.rm.code(v) for v in M.bytes_of([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15])] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15]


def test_the_statement_equals_the_model_on_every_designed_locus():
    loci, expect = M.designed_loci(), M.designed_expected()
    assert len(loci) >= 120
    wrong = [l[0] for l, e in zip(loci, expect) if stated(l, M.polish_of(l)) != tuple(e)]
    assert not wrong, (len(wrong), wrong[:5])


def test_the_statement_equals_the_model_on_the_fuzz():
    loci = M.fuzz_loci()
    assert len(loci) == 40
    for l in loci:
        pol = M.polish_of(l)
        assert stated(l, pol) == tuple(M.revote(l[2], l[3], l[4], pol)), l[0]


def test_spell_gives_the_codes_of_the_polished_text():
    """For a set without VAPOR_SEQ_UPPER the codes of polish.apply's text are the spelt codes; an upper-cased twin spells what
    its plane holds."""
    n = 0
    for l in M.designed_loci() + M.fuzz_loci():
        calls, sites, ins = arrays(M.polish_of(l))
        text = polish.apply(l[3].decode("latin-1"), calls, sites, ins)
        spelt, own = revote.spell(revote.codes_of(l[3]), calls, sites, ins)
        assert spelt.tolist() == revote.codes_of(text).tolist() and int(own[-1]) == len(text) and len(own) == len(l[3]) + 1, l[0]
        assert np.all(np.diff(own) >= 0) and text == PMOD.text(l[3], *M.polish_of(l)[1:4]).decode("latin-1")
        up, _own = revote.spell(revote.codes_of(l[3], True), calls, sites, ins)
        assert up.tolist() == revote.codes_of(text.upper()).tolist()
        n += spelt.tolist() != up.tolist()
    assert n >= 3                                     # (lower-case alleles are among them)


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_is_told_from_the_rule_at_least_three_times(mutant):
    assert len(M.MUTANTS) == 9 and len(M.SPELL_MUTANTS) == 6
    assert M.told_apart(mutant) >= 3, (mutant, M.told_apart(mutant))


def test_the_designed_loci_the_section_names_are_there():
    loci, expect = M.designed_loci(), M.designed_expected()
    by = dict(zip((l[0] for l in loci), zip(loci, expect)))
    # the polished length at nibble, word and chunk edges
    for plen in (7, 8, 9, 31, 32, 33, 63, 64, 65):
        l, e = by["plen %d" % plen]
        assert e[0] == [0, plen, 0, 0] and len(l[3]) == plen + 1 and len(e[2]) == plen
        assert by["plen %d, nothing called" % plen][1][0] == [0, plen, 0, 0]
    # flagged columns at 255, 256 and 257: ranks 0, 1 and 2 across a round, texts of 1, 2 and 3 bases
    l, e = by["sites before (255, 256, 257)"]
    pol = M.polish_of(l)
    assert [s for s in pol[2]] == [[255, 1], [256, 2], [257, 3]] and e[3][254:259] == [254, 256, 259, 263, 264] and e[0][1] == 306
    # reads that start at column 0, at a flagged column, at a deleted column and the one behind it, and at len
    l, e = by["3 identical planted reads"]
    pol = M.polish_of(l)
    starts = {o for _r, o in l[2]}
    assert {0, 70, 71, 110, 150} <= starts and pol[1][70] == M.DELETE and pol[1][110] & M.SITE_BIT
    at = {o: v for (_r, o), v in zip(l[2], e[1])}
    assert at[70][2] == at[71][2] == 70 and at[110][2] == 109 + 3 and at[150][2:] == [152, 0] and at[150][0] == 0
    # more than 256 sites, 1 200 columns; fewer than three voters
    l, e = by["more than 256 sites"]
    assert len(l[3]) == 1200 and e[0] == [0, 1456, 0, 0] and len(l[2]) >= 6
    assert by["two voters"][1][0] == [0, 65, 0, 0] and by["no voter"][1][2] == [M.rm.code(v) for v in by["no voter"][0][3]]
    # every band the section names, so that every compiled width runs
    assert {l[4] for l in loci} >= {1, 2, 31, 32, 33, 100, 256, 512}
    assert all(v[1] == 0 for e in expect for v in e[1])


# ------------------------------------------------------------------------------------------------------------------------------
# the columns
# ------------------------------------------------------------------------------------------------------------------------------
def payload(d_ref, d_alt, d_pol, pn=None, status=0, pstatus=0):
    p = realign.Payload(realign.votes(d_ref, d_alt))
    pn = sum(1 for v in p if v >= realign.MARGIN) if pn is None else pn
    p.polish = polish.Polish([pstatus, pn, 100, 0, 0, 0, 0, 0])
    p.revote = revote.Revote(status, d_ref, d_pol)
    return p


def test_the_eight_columns_equal_the_model_and_the_gate_holds():
    assert len(M.COLUMN_CASES) >= 9
    for c in M.COLUMN_CASES:
        assert revote.eight(payload(*c)) == M.eight(*c), c
    c = M.COLUMN_CASES[0]
    got = revote.eight(payload(*c))
    assert got[:4] == ["4", "2", "0", "0.667"] and got[4] == "0/1" and got[-2:] == ["20,20,20,10,-32,-28", "15"]
    assert revote.eight(None) == ["."] * 8 and revote.eight(realign.Payload([20, 20, 20])) == ["."] * 8
    assert revote.eight(payload(*c, status=L.E_ARG)) == ["."] * 8                 # the re-vote status, or a vote pair's
    assert revote.eight(payload(*c, pstatus=L.E_NOMEM)) == ["."] * 8              # the polish status
    assert revote.eight(payload(*c, pn=2)) == ["."] * 8                           # fewer than MIN_COV piled
    p = payload(*c)
    p.revote = None
    assert revote.eight(p) == ["."] * 8
    # a negative GAIN is reported as it is
    assert revote.eight(payload([30, 30, 30], [5, 5, 5], [6, 7, 5]))[-1] == "-3"


def test_the_columns_and_their_round_trip():
    names = ("VaPoR_RA2_ALT", "VaPoR_RA2_REF", "VaPoR_RA2_NC", "VaPoR_RA2_VAF", "VaPoR_RA2_GT", "VaPoR_RA2_GQ", "VaPoR_RA2_Rec", "VaPoR_RA2_GAIN")
    assert revote.COLUMNS == names and [i[0] for i in revote.INFO] == list(names) and all(len(i) == 4 for i in revote.INFO)
    for src, width in ((polish, 13), (junction, 19)):
        s = revote.over(src)
        assert s.COLUMNS == src.COLUMNS + names and s.INFO == src.INFO + revote.INFO
        assert s.columns(None) == ["."] * (width + 8) and s.pack(None) == [] and s.unpack([]) is None
        p = payload(*M.COLUMN_CASES[0])
        if src is junction:
            p.junction = junction.Junction((0, 5, 9, 4, 0, 5, 9, 4, junction.DEL))
        assert s.columns(p) == src.columns(p) + revote.eight(p) and s.columns(p)[-1] == "15"
        q = s.unpack(s.pack(p))
        assert list(q) == list(p) and (q.revote.status, q.revote.d_ref, q.revote.d_pol) == (0, p.revote.d_ref, p.revote.d_pol)
        assert s.columns(q) == s.columns(p) and src.columns(q) == src.columns(p)
        p.revote = revote.Revote(L.E_ARG, p.revote.d_ref, [-1] * 6)
        assert s.columns(s.unpack(s.pack(p)))[-8:] == ["."] * 8
        p.revote = None
        q = s.unpack(s.pack(p))
        assert q.revote is None and s.columns(q) == src.columns(p) + ["."] * 8
        bare = s.unpack(s.pack(realign.Payload([1, 2])))
        assert list(bare) == [1, 2] and bare.polish is None and bare.revote is None
        assert s.columns_many([None, p]) == [s.columns(None), s.columns(p)]
    assert revote.columns(None) == ["."] * 21 and revote.unpack(revote.pack(payload(*M.COLUMN_CASES[1]))).revote.d_pol == (10, 10, 10, 9)


# ------------------------------------------------------------------------------------------------------------------------------
# the parser, the request and the modes
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_and_the_help_text_is_unchanged(monkeypatch):
    p = cli.build_parser()
    base = TR.BASE + ["--realign", "--realign-polish"]
    assert p.parse_args(base + ["--realign-revote"]).realign_revote is True and p.parse_args(base).realign_revote is False
    for more in (["--realign-junction"], ["--realign-out", "pre"], ["--realign-junction", "--realign-out", "pre"]):
        a = p.parse_args(base + ["--realign-revote"] + more)
        assert a.realign_revote and a.realign_junction == ("--realign-junction" in more) and a.realign_out == ("pre" if "pre" in more else None)
    assert "--realign-revote" not in cli.MODE_OPTIONS and len(cli.MODE_OPTIONS) == 9
    monkeypatch.setenv("COLUMNS", "80")
    with open(os.path.join(ROOT, "tests", "golden", "cli_help.txt")) as f:
        assert p.format_help() == f.read()
    assert "--realign-revote" not in p.format_help() and "--realign-revote" not in p.format_usage()


def test_refused_without_realign_polish(capsys):
    for cmd in ("bed", "vcf", "svelter", "ins"):
        TR._refused([cmd] + TR.BASE + ["--realign-revote"], "--realign-revote needs --realign-polish", capsys)
    TR._refused(["bed"] + TR.BASE + ["--realign", "--realign-revote"], "--realign-revote needs --realign-polish", capsys)
    TR._refused(["vcf"] + TR.BASE + ["--realign", "--realign-out", "pre", "--realign-revote"], "--realign-revote needs --realign-polish", capsys)


# ------------------------------------------------------------------------------------------------------------------------------
# the entry, its binding and the host plan of the call
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_bound():
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    assert re.search(r"\bint vapor_realign_revote\(vapor_ctx\* ctx, vapor_seqset\* set, int64_t n_pairs, const vapor_pair\* pairs, int32_t band, "
                     r"int64_t n_loci,\s+const int64_t\* first, const int64_t\* col_off, int32_t\* stats, uint8_t\* calls, int32_t\* sites, "
                     r"uint8_t\* ins,\s+uint32_t\* counts, int64_t n_votes, const vapor_pair\* votes, const int64_t\* vfirst, int32_t\* vout, "
                     r"int32_t\* lout,\s+const int64_t\* spelt_off, uint8_t\* spelt\);", h)
    assert "#define VAPOR_ABI_VERSION 3" in h
    assert "vapor_realign_revote" in L.EXPORTS and "vapor_realign_revote" in L.OPTIONAL_EXPORTS and L.ABI_VERSION == 3
    lib = L.load()
    assert hasattr(lib, "vapor_realign_revote") and len(lib.vapor_realign_revote.argtypes) == 20
    from vapor_amd import build
    assert any(p.endswith("vapor_revote.h") for p in build.KERNEL_FILES) and any(p.endswith("vapor_revote_plan.h") for p in build.DEPS)
    stub = open(os.path.join(ROOT, "vapor_amd", "csrc", "vapor_bam.cpp")).read()
    assert re.search(r'__attribute__\(\(weak\)\) int vapor_realign_revote\(', stub)
    # the polish's host code is shared, not copied: both entries are one call each into the same function
    hip = open(os.path.join(ROOT, "vapor_amd", "csrc", "vapor_hip.hip")).read()
    assert len(re.findall(r"return polish_call\(\"vapor_realign_(polish|revote)\"", hip)) == 2 and hip.count("hipLaunchKernelGGL(consensus_kernel") == 1


def test_an_engine_without_the_entry_raises_one_clear_error(monkeypatch):
    from vapor_amd.engine import Engine

    class Without:
        def vapor_build_flags(self):
            return b""
    monkeypatch.setattr(L, "load", lambda: Without())
    e = object.__new__(Engine)
    assert e.realign_revote_available() is False
    with pytest.raises(NotImplementedError, match=r"vapor_realign_revote: the loaded library has no re-vote kernels \(--realign-revote\)"):
        Engine.realign_revote(e, None, np.zeros(0, dtype=L.PAIR_DTYPE), 256, [0], [0], np.zeros(0, dtype=L.PAIR_DTYPE), [0])


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("revote") / "revote_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"),
                           os.path.join(ROOT, "tools", "revote_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "constants and layout: stated",
    "tables: 2000 calls, refused ones among them",
    "vote pairs: 20000 cases, served and refused ones",
    "groups: 300 calls, many in several groups, the pieces move some cuts",
    "call plan: 65 calls, every kind of locus and slot, spelt bytes dealt past group 0 and clamped, the polish's share unchanged; "
    "check_args: 154 cases",
    "revote_check: all equal",
])
def test_the_calls_host_plan_against_direct_statements_under_sanitizers(check_output, line):
    assert line in check_output


# ------------------------------------------------------------------------------------------------------------------------------
# through cli.main, on an engine whose distances, traces, piles, junctions and second votes are the statements'
# ------------------------------------------------------------------------------------------------------------------------------
_REVOTED = {}


def stated_revote(self, ss, pairs, band, first, col_off, votes, vfirst, want_counts=False, want_spelt=False, spelt_off=None):
    """Engine.realign_revote by polish.statement and revote.statement over the set's texts (`texts` where the stand-in keeps the
    derived ones there)."""
    texts = getattr(ss, "texts", None) or ss.seqs
    stats, calls, sites, ins, _none = TP.stated_polish(self, ss, pairs, band, first, col_off, want_counts)
    ng = len(first) - 1
    vout = np.zeros((len(votes), 4), dtype=np.int32)
    lout = np.zeros((ng, 4), dtype=np.int32)
    for g in range(ng):
        mine = votes[vfirst[g]:vfirst[g + 1]]
        allele = texts[pairs[first[g]]["seq2"]] if first[g + 1] > first[g] else texts[mine[0]["seq2"]] if len(mine) else None
        if allele is None:
            lout[g] = (L.E_ARG, 0, 0, 0)
            continue
        assert all(texts[v["seq2"]] is allele or texts[v["seq2"]] == allele for v in mine)
        key = (tuple((texts[v["seq1"]], int(v["off2"])) for v in mine), allele, calls[col_off[g]:col_off[g + 1]].tobytes(), sites[g].tobytes(),
               ins[g].tobytes(), band)
        if key not in _REVOTED:
            _REVOTED[key] = revote.statement(list(key[0]), allele, calls[col_off[g]:col_off[g + 1]], sites[g], ins[g], band)[:2]
        lout[g], vout[vfirst[g]:vfirst[g + 1]] = _REVOTED[key]
    return stats, calls, sites, ins, None, vout, lout, None, None


class RevoteFake(TJ.JunctionFake):
    """JunctionFake plus realign_revote: the statements over the set's texts; records what it was asked."""

    def __init__(self, orc):
        super().__init__(orc)
        self.revote_calls = []           # per call: (pairs, loci, vote pairs)

    def realign_revote(self, ss, pairs, band, first, col_off, votes, vfirst, want_counts=False, want_spelt=False, spelt_off=None):
        self.revote_calls.append((len(pairs), len(first) - 1, len(votes)))
        return stated_revote(self, ss, pairs, band, first, col_off, votes, vfirst)


@pytest.fixture()
def fake(oracle):
    eng = RevoteFake(oracle)
    pipeline.set_engine(eng)
    yield eng
    pipeline.set_engine(None)
    seqio.set_backend(None)


SPECS = TP.SPECS
POLISH = ["--realign", "--realign-polish"]


def test_cli_on_a_world_in_memory(fake, tmp_path):
    w = synth.make_support_world(seed=4, specs=SPECS, layers=4, read_len=4000)
    text = synth.bed_text(w)
    earlier = {}
    for name, more in (("po", []), ("ju", ["--realign-junction"])):
        seqio.set_backend(seqio.MemorySamtools(w))
        earlier[name], _ = TS.run_main(tmp_path, name, "bed", text, POLISH + more + ["--realign-out", str(tmp_path / (name + "_pre"))])
    assert fake.polish_calls and not fake.revote_calls                             # no realign_revote call without the flag
    n_polish = len(fake.polish_calls)
    tables = {}
    for name, more in (("whole", []), ("one", ["--chunk", "1"]), ("files", ["--realign-out", str(tmp_path / "rv_pre")]),
                       ("junction", ["--realign-junction"]), ("all", ["--realign-junction", "--realign-out", str(tmp_path / "all_pre")])):
        fake.revote_calls.clear()
        seqio.set_backend(seqio.MemorySamtools(w))
        tables[name], _ = TS.run_main(tmp_path, name, "bed", text, POLISH + ["--realign-revote"] + more)
        assert fake.revote_calls and len(fake.polish_calls) == n_polish            # the one call, in place of the polish's
    assert tables["whole"] == tables["one"] == tables["files"] and tables["junction"] == tables["all"]
    for pre in ("rv_pre", "all_pre"):                                               # --realign-out's three files, byte for byte
        for ext in (".sam", ".fa", ".pol.fa"):
            assert open(str(tmp_path / pre) + ext).read() == open(str(tmp_path / "po_pre") + ext).read(), (pre, ext)
    rows = [r.split("\t") for r in tables["whole"].splitlines()]
    assert rows[0][-21:] == list(polish.COLUMNS + revote.COLUMNS) and len(rows) == 1 + len(SPECS)
    assert "\n".join("\t".join(r[:-8]) for r in rows) + "\n" == earlier["po"]       # polish's columns unchanged, followed by the eight
    jrows = [r.split("\t") for r in tables["junction"].splitlines()]
    assert jrows[0][-27:] == list(junction.COLUMNS + revote.COLUMNS)
    assert "\n".join("\t".join(r[:-8]) for r in jrows) + "\n" == earlier["ju"]      # junction's too
    assert [r[-8:] for r in jrows] == [r[-8:] for r in rows]
    n_gated = 0
    for r, (kind, _size, zyg) in zip(rows[1:], SPECS):
        ra, pn, two = r[-21:-14], r[-14], r[-8:]
        if pn == "." or int(pn) < polish.MIN_COV:
            assert two == ["."] * 8, (kind, zyg, r[-21:])                          # fewer than three voters: no second vote
            n_gated += 1
            continue
        assert len(two[6].split(",")) == len(ra[6].split(","))                     # every read votes again, not only the piled ones
        if zyg == "hom" and kind != "INS":
            # exact DEL, INV and TANDUP calls: the polished allele is the call's own, and so is the vote
            assert two[:7] == ra and two[7] == "0", (kind, r[-21:])
        d1, d2 = [int(v) for v in ra[6].split(",")], [int(v) for v in two[6].split(",")]
        assert int(two[7]) == sum(b - a for a, b in zip(d1, d2) if a >= realign.MARGIN)
    assert n_gated >= 1 and sum(1 for r in rows[1:] if r[-1] != ".") >= 4
    # a locus without a payload: '.' in all of them, and no call
    seqio.set_backend(seqio.MemorySamtools(w))
    fake.revote_calls.clear()
    few, _ = TS.run_main(tmp_path, "few", "bed", text, POLISH + ["--realign-revote", "--PB-supp", "1000"])
    assert all(r.split("\t")[-21:] == ["."] * 21 for r in few.splitlines()[1:]) and not fake.revote_calls


def test_vcf_info_keys(fake, tmp_path):
    w = synth.make_support_world(seed=4, specs=SPECS[:2], layers=4, read_len=4000)
    seqio.set_backend(seqio.MemorySamtools(w))
    table, annotated = TS.run_main(tmp_path, "v", "vcf", synth.vcf_text(w), POLISH + ["--realign-revote"])
    for name in revote.COLUMNS:
        assert "##INFO=<ID=%s," % name in annotated
    recs = [ln for ln in annotated.splitlines() if not ln.startswith("#")]
    rows = [r.split("\t") for r in table.splitlines()[1:]]
    assert len(recs) == len(rows) == 2
    for rec, r in zip(recs, rows):
        for name, v in zip(revote.COLUMNS, r[-8:]):
            assert ("%s=%s" % (name, v) in rec.split("\t")[7].split(";")) == (v != "."), (name, v)       # a '.' is left out
    assert rows[0][-1] != "." and rows[1][-8:] == ["."] * 8                         # the hom locus votes again, the ref locus has no pile


def test_a_call_that_ends_5_bases_late_gains_on_the_polished_allele(fake, tmp_path):
    """test_polish_cpu's world whose DEL call ends 5 bases late: every piled read loses the edits the call was wrong by - GAIN is
    positive and no piled read's diff shrinks."""
    w = synth.make_support_world(seed=4, specs=SPECS[:1], layers=4, read_len=4000)
    shifted = []
    for ln in synth.bed_text(w).splitlines():
        f = ln.split("\t")
        f[2] = str(int(f[2]) + 5)
        shifted.append("\t".join(f))
    seqio.set_backend(seqio.MemorySamtools(w))
    table, _ = TS.run_main(tmp_path, "s", "bed", "\n".join(shifted) + "\n", POLISH + ["--realign-revote"])
    r = table.splitlines()[1].split("\t")
    d1, d2 = [int(v) for v in r[-15].split(",")], [int(v) for v in r[-2].split(",")]
    piled = [(a, b) for a, b in zip(d1, d2) if a >= realign.MARGIN]
    print("5 bases late:", r[-21:])
    assert len(piled) == int(r[-14]) >= 3 and all(b >= a for a, b in piled) and int(r[-1]) == sum(b - a for a, b in piled) > 0
    assert int(r[-8]) >= int(r[-21])                                               # no ALT voter is lost
