"""Host logic of the wide route without a GPU: pipeline.score_requests splits off the requests longer than MAX_SEQ_LEN and
scores them through an engine's score_wide; an engine without it keeps today's ValueError.  The stand-in engine below is
test infrastructure: its numbers come from the C oracle."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fake_engine import FakeEngine

from vapor_amd import _lib as L

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


class WideFakeEngine(FakeEngine):
    """FakeEngine plus score_wide: the oracle's statistics record for every pair up to MAX_WIDE_SEQ_LEN (no DIR words)."""

    def score_wide(self, ss, pairs, want_hits=False):
        assert not want_hits
        st = np.zeros((len(pairs), 16), dtype=np.int64)
        for t, p in enumerate(pairs):
            s1, s2 = ss.seqs[int(p["seq1"])], ss.seqs[int(p["seq2"])]
            if max(len(s1), len(s2)) > L.MAX_WIDE_SEQ_LEN:
                st[t, 1] = st[t, 2] = -1
                st[t, 15] = L.E_ARG
                continue
            r = self.orc.pair_stats(int(p["k"]), s1, s2[int(p["off2"]):])
            if not int(p["flags"]) & L.PF_C1:
                r[3] = r[4] = 0
            if not int(p["flags"]) & L.PF_C2:
                r[5] = r[6] = r[9] = 0
            st[t] = r
        return st


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes().decode()


def _mutate(rng, s, rate=0.01):
    a = np.frombuffer(s.encode(), dtype=np.uint8).copy()
    pos = rng.random(len(a)) < rate
    a[pos] = ACGT[rng.integers(0, 4, int(pos.sum()))]
    return a.tobytes().decode()


def _requests():
    from vapor_amd.drivers import Score
    rng = np.random.default_rng(7)
    ref = _rand(rng, 6000)
    alt = ref[:3000] + _rand(rng, 66000) + ref[3000:]
    reads = [(_mutate(rng, alt)[m:], m) for m in (0, 4)]
    sref = _rand(rng, 3000)
    salt = sref[:1000] + sref[1400:]
    return [Score("s1", sref, salt, [(_mutate(rng, salt), 0)], 10),
            Score("s1", ref, alt, reads, 10),
            Score("del", ref, alt, reads, 20),
            Score("s2", ref, alt, reads, 10),
            Score("s2", sref, salt, [], 10)]


def test_long_requests_are_scored_on_the_wide_route(oracle):
    from vapor_amd import pipeline
    reqs = _requests()
    got = pipeline.score_requests(WideFakeEngine(oracle), reqs)
    assert got[0] == pipeline.score_requests(FakeEngine(oracle), reqs[:1])[0]
    assert got[4] == []

    def one(fn, r, x):
        a, b = fn(r.ref_seq, r.alt_seq, [x[0], x[1]], r.k)
        return None if (a == 0 or b == 0) else 1.0 - float(b) / float(a)
    for r, g in zip(reqs[1:4], got[1:4]):
        assert isinstance(g, list), g
        exp = []
        for x in r.reads:
            if r.kind == "s1":
                exp.append(one(oracle.score_abs_dis_m1b, r, x))
            elif r.kind == "s2":
                exp.append(one(oracle.score_within_10Perc_m1b, r, x))
            else:
                s1, s2 = one(oracle.score_abs_dis_m1b, r, x), one(oracle.score_within_10Perc_m1b, r, x)
                exp.append(min(s1, s2) if s1 is not None and s2 is not None else (s1 if s1 is not None else s2))
        assert g == exp, (r.kind, g, exp)
    assert any(v is not None for g in got[1:4] for v in g)


def test_an_engine_without_the_wide_route_keeps_the_value_error(oracle):
    from vapor_amd import pipeline
    reqs = _requests()
    got = pipeline.score_requests(FakeEngine(oracle), reqs)
    for g in got[1:4]:
        assert isinstance(g, ValueError)
    assert isinstance(got[0], list) and got[4] == []


def test_beyond_the_wide_cap_is_a_value_error(oracle):
    from vapor_amd import pipeline
    from vapor_amd.drivers import Score
    rng = np.random.default_rng(8)
    alt = _rand(rng, 20) * (L.MAX_WIDE_SEQ_LEN // 20 + 1)
    got = pipeline.score_requests(WideFakeEngine(oracle), [Score("s2", alt[:100], alt, [(alt[:30], 0)], 10)])
    assert isinstance(got[0], ValueError)


def test_engine_without_the_symbols_raises_not_implemented(monkeypatch):
    from vapor_amd.engine import Engine
    fake = type("NoWide", (), {})()
    monkeypatch.setattr(L, "load", lambda: fake)
    with pytest.raises(NotImplementedError):
        Engine._wide_entry("vapor_wide_batch")


def test_the_cpu_twin_has_no_wide_route(monkeypatch, oracle):
    """The twin exports the names (it answers the whole header) with a stub that refuses; the engine says NotImplemented."""
    import ctypes
    from vapor_amd.engine import Engine
    twin = ctypes.CDLL(oracle.build_twin())
    twin.vapor_wide_batch.restype = ctypes.c_int
    assert twin.vapor_wide_batch(None, None, 0, None, None, None, 0, None) == L.E_ARG
    twin.vapor_build_flags.restype = ctypes.c_char_p
    monkeypatch.setattr(L, "load", lambda: twin)
    for name in ("vapor_wide_batch", "vapor_clean_hits_wide"):
        with pytest.raises(NotImplementedError):
            Engine._wide_entry(name)


def test_header_cap_equals_the_python_constant():
    src = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    m = re.search(r"#define VAPOR_MAX_WIDE_SEQ_LEN (\d+)", src)
    assert m and int(m.group(1)) == L.MAX_WIDE_SEQ_LEN == 2 ** 20 - 1
    assert "vapor_wide_batch" in L.EXPORTS and "vapor_clean_hits_wide" in L.EXPORTS
