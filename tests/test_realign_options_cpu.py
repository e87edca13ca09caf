"""The path of a `--realign-*` option from the command line to the columns ("How a `--realign-*` option plugs
in"), without a device: every combination of the flags through the parser, realign.Options, modes.realign and the one wrapper
drivers.vapor_realign; the floats a payload travels as between ranks, against lists written out by hand; and what `vapor bed |
vcf` writes under every legal combination, against the digests tools/gen_realign_options_golden.py took on the commit before the
options record came in (tests/golden/realign_options.json)."""
import inspect
import itertools
import json
import os
import sys

import pytest

import test_realign_cpu as TR
from conftest import GOLDEN, ROOT
from vapor_amd import _lib as L
from vapor_amd import cli, drivers, junction, modes, polish, realign, revote

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_realign_options_golden as GEN  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------------------
# every combination of the flags
# ------------------------------------------------------------------------------------------------------------------------------
def refusal(ra, out, pol, jun, rev):
    """The parser's message for a combination, None for a legal one: its four rules in the order it states them."""
    if out and not ra:
        return "--realign-out needs --realign"
    if pol and not ra:
        return "--realign-polish needs --realign"
    if jun and not pol:
        return "--realign-junction needs --realign-polish"
    if rev and not pol:
        return "--realign-revote needs --realign-polish"
    return None


def argv_of(ra, out, pol, jun, rev):
    return (["--realign"] if ra else []) + (["--realign-polish"] if pol else []) + (["--realign-junction"] if jun else []) + \
        (["--realign-revote"] if rev else []) + (["--realign-out", "pre"] if out else [])


class Reached(Exception):
    """The run got as far as reading its input: every option was accepted and the mode is made."""


def test_every_combination_of_the_flags(capsys, monkeypatch, tmp_path):
    # the parameter lists, pinned once
    assert realign.Options._fields == ("trace", "polish", "junction", "revote") and realign.Options() == (False, False, False, False)
    assert list(inspect.signature(realign.Options).parameters) == ["trace", "polish", "junction", "revote"]
    assert list(inspect.signature(drivers.Realign.__init__).parameters)[1:] == ["ref_seq", "alt_seq", "reads", "name", "options"]
    assert list(inspect.signature(drivers.vapor_realign).parameters) == ["options", "name", "driver", "args"]
    assert list(inspect.signature(modes.realign).parameters) == ["options", "sink"]
    assert inspect.signature(modes.realign).parameters["options"].default == realign.Options()
    assert inspect.signature(drivers.Realign.__init__).parameters["options"].default == realign.Options()
    assert modes.REALIGN.options == realign.Options() and modes.REALIGN.sink is None and modes.SUPPORT.options is None
    with pytest.raises(AttributeError):
        realign.Options().polish = True
    with pytest.raises(AttributeError):
        drivers.Realign("A", "C", []).revote = True                    # (a view of the options, not a slot)

    made = []
    orig = modes.realign
    monkeypatch.setattr(modes, "realign", lambda *a, **k: made.append(orig(*a, **k)) or made[-1])

    def reached(*_a, **_k):
        raise Reached()
    monkeypatch.setattr(cli, "bed_info_readin", reached)
    monkeypatch.chdir(tmp_path)

    def one_score():
        got = yield drivers.Score("s1", "ACGT", "ACT", [("ACGT", 0)], 10)
        return got

    sections = ((polish, 6), (junction, 6), (revote, 8))
    own = {polish: polish.COLUMNS[7:], junction: junction.COLUMNS[13:], revote: revote.COLUMNS}
    n_legal = 0
    for ra, out, pol, jun, rev in itertools.product((False, True), repeat=5):
        flags = (out, pol, jun, rev)
        why = refusal(ra, out, pol, jun, rev)
        # realign.Options raises on exactly the combinations that ask for the junction or the second vote without the polish
        if (jun or rev) and not pol:
            with pytest.raises(ValueError):
                realign.Options(*flags)
        else:
            assert tuple(realign.Options(*flags)) == flags
        if why is not None:
            for cmd in ("bed", "vcf"):
                TR._refused([cmd] + TR.BASE + argv_of(ra, out, pol, jun, rev), why, capsys)
            continue
        del made[:]
        with pytest.raises(Reached):
            cli.main(["bed"] + TR.BASE + ["--no-figures"] + argv_of(ra, out, pol, jun, rev))
        if not ra:
            assert flags == (False,) * 4 and not made                 # (the plain run: no mode)
            continue
        n_legal += 1
        # the mode cli.main makes: built once, from the four arguments, with the sink the run writes to
        assert len(made) == 1 and made[0].options == realign.Options(*flags)
        want_sink = (polish.PolishWriter if pol else realign.TraceWriter) if out else type(None)
        assert type(made[0].sink) is want_sink and (not out or made[0].sink.stem == "pre")
        # modes.realign: the columns are realign's seven, then each asked section's own, in the order polish, junction, revote
        sink = object()
        for m, s in ((made[0], made[0].sink), (modes.realign(realign.Options(*flags), sink), sink), (modes.realign(realign.Options(*flags)), None)):
            asked = [x for x, on in zip((polish, junction, revote), (pol, jun, rev)) if on]
            assert m.name == "realign" and m.attr == "realign" and m.skip_dot and m.sink is s
            assert m.COLUMNS == realign.COLUMNS + tuple(c for x in asked for c in own[x])
            assert len(m.COLUMNS) == 7 + sum(n for (x, n), on in zip(sections, (pol, jun, rev)) if on)
            assert m.keys == m.COLUMNS and [i[0] for i in m.INFO] == list(m.COLUMNS) and all(len(i) == 4 for i in m.INFO)
            assert m.columns_many([None]) == [["."] * len(m.COLUMNS)] and m.pack(None) == [] and m.unpack([]) is None
        assert m.COLUMNS == (revote.over(junction if jun else polish).COLUMNS if rev else junction.COLUMNS if jun else
                             polish.COLUMNS if pol else realign.COLUMNS)
        # the one wrapper: the request carries exactly these flags, and the name iff it asks for traces
        gen = drivers.vapor_realign(made[0].options, "k", one_score)
        assert isinstance(next(gen), drivers.Score)
        req = gen.send([0.5])
        assert isinstance(req, drivers.Realign) and (req.trace, req.polish, req.junction, req.revote) == flags
        assert req.options is made[0].options and req.name == ("k" if out else None)
        assert (req.ref_seq, req.alt_seq, req.reads) == ("ACGT", "ACT", [("ACGT", 0)])
    assert n_legal == 10
    r = drivers.Realign("A", "C", [])
    assert (r.trace, r.polish, r.junction, r.revote, r.name) == (False, False, False, False, None)


# ------------------------------------------------------------------------------------------------------------------------------
# the floats between ranks: [n, diffs], then per section of the run 0, or 1 and the section's values
# ------------------------------------------------------------------------------------------------------------------------------
B3 = [3.0, 12.0, -30.0, 0.0]                                              # three reads' diffs
B0 = [0.0]                                                                # no read
NO = [0.0]                                                                # a section the payload carries nothing of
P = [1.0, 0.0, 3.0, 1200.0, 3.0, 5.0, 2.0, 4.0, 1.0]                      # polish: its eight statistics
J = [1.0, 0.0, 100.0, 155.0, 55.0, 2.0, 101.0, 151.0, 50.0, 1.0]          # junction: its nine integers
R = [1.0, 0.0, 3.0, 27.0, 36.0, 21.0, 40.0, 5.0, 20.0]                    # revote: status, n, d_pol x n, d_ref x n
P0 = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]                        # an empty pile
R0 = [1.0, -4.0, 0.0]                                                     # a second vote refused (E_ARG), of no read


def _payload(diffs, po=None, jn=None, rv=None):
    p = realign.Payload(diffs)
    if po is not None:
        p.polish = polish.Polish(po)
    if jn is not None:
        p.junction = junction.Junction(jn)
    if rv is not None:
        p.revote = revote.Revote(*rv)
    return p


STATS, VALS, VOTE = (0, 3, 1200, 3, 5, 2, 4, 1), (0, 100, 155, 55, 2, 101, 151, 50, 1), (0, (40, 5, 20), (27, 36, 21))
DESIGNED = {
    "all": lambda: _payload([12, -30, 0], STATS, VALS, VOTE),
    "none": lambda: _payload([12, -30, 0]),
    "polish": lambda: _payload([12, -30, 0], po=STATS),
    "junction": lambda: _payload([12, -30, 0], jn=VALS),
    "revote": lambda: _payload([12, -30, 0], rv=VOTE),
    "no read": lambda: _payload([], po=(0,) * 8, rv=(L.E_ARG, (), ())),
}
# per section list, the floats of every designed payload
WIRE = {
    "P": {"all": B3 + P, "none": B3 + NO, "polish": B3 + P, "junction": B3 + NO, "revote": B3 + NO, "no read": B0 + P0},
    "PJ": {"all": B3 + P + J, "none": B3 + NO + NO, "polish": B3 + P + NO, "junction": B3 + NO + J, "revote": B3 + NO + NO,
           "no read": B0 + P0 + NO},
    "PR": {"all": B3 + P + R, "none": B3 + NO + NO, "polish": B3 + P + NO, "junction": B3 + NO + NO, "revote": B3 + NO + R,
           "no read": B0 + P0 + R0},
    "PJR": {"all": B3 + P + J + R, "none": B3 + NO + NO + NO, "polish": B3 + P + NO + NO, "junction": B3 + NO + J + NO,
            "revote": B3 + NO + NO + R, "no read": B0 + P0 + NO + R0},
}


def _fields(p, attrs):
    got = {"diffs": list(p)}
    for a in attrs:
        obj = getattr(p, a)
        got[a] = None if obj is None else {"polish": lambda o: o.stats, "junction": lambda o: o.vals,
                                          "revote": lambda o: (o.status, o.d_ref, o.d_pol)}[a](obj)
    return got


@pytest.mark.parametrize("which", list(WIRE))
def test_the_floats_between_ranks_are_the_stated_ones(which):
    attrs = [{"P": "polish", "J": "junction", "R": "revote"}[c] for c in which]
    opts = realign.Options(False, "P" in which, "J" in which, "R" in which)
    surfaces = [modes.realign(opts), {"P": polish, "PJ": junction, "PR": revote, "PJR": revote.over(junction)}[which]]
    assert WIRE["PJR"]["all"] == [3, 12, -30, 0, 1, 0, 3, 1200, 3, 5, 2, 4, 1, 1, 0, 100, 155, 55, 2, 101, 151, 50, 1, 1, 0, 3, 27, 36, 21, 40, 5, 20]
    assert WIRE["PR"]["no read"] == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, -4, 0]
    for s in surfaces:
        assert s.pack(None) == [] and s.unpack([]) is None and s.unpack(None) is None
        for name, make in DESIGNED.items():
            p, flat = make(), WIRE[which][name]
            got = s.pack(p)
            assert got == flat and all(type(v) is float for v in got), (which, name)
            q = s.unpack(flat)
            assert type(q) is realign.Payload and _fields(q, attrs) == _fields(p, attrs), (which, name)
            assert s.pack(q) == flat and s.columns_many([q]) == s.columns_many([p])
            # what the run's sections do not carry stays unset, and an extra that was never set is no instance attribute
            assert all(getattr(q, a) is None for a in ("polish", "junction", "revote", "traces") if a not in attrs)
            assert set(vars(q)) == {a for a in attrs if getattr(p, a) is not None}
    bare = realign.unpack(realign.pack(realign.Payload([1, 2])))
    assert vars(bare) == {} and (bare.traces, bare.polish, bare.junction, bare.revote) == (None,) * 4


# ------------------------------------------------------------------------------------------------------------------------------
# what the runs write, against the commit before
# ------------------------------------------------------------------------------------------------------------------------------
def test_every_legal_run_writes_what_it_wrote_before(oracle, tmp_path):
    with open(os.path.join(GOLDEN, GEN.NAME)) as f:
        want = json.load(f)
    assert len(want) == 11 and sum(1 for k in want if k.startswith("bed ")) == 10
    assert [k for k in want if k.startswith("vcf ")] == ["vcf --realign --realign-polish --realign-junction --realign-revote --realign-out"]
    for k, v in want.items():
        files = {".fa", ".sam"} | ({".pol.fa"} if "--realign-polish" in k else set()) if "--realign-out" in k else set()
        assert set(v) == {"table"} | files | ({"annotated"} if k.startswith("vcf ") else set()), k     # (no .pol.fa without --realign-polish)
    got = GEN.digests(tmp_path)
    assert got == want, sorted(k for k in want if got.get(k) != want[k])
