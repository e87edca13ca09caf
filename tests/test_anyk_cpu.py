"""The any-k route without a GPU: the new names of the reference's module surface, subkeys / key_modify against the goldens,
the test-local restatement of both match rules (anyk_model) against every golden, the limits, the routing of scorer requests
through a stand-in engine, and the CPU twin's refusal."""
import ctypes
import os
import re

import numpy as np
import pytest

import anyk_model as model
from conftest import ROOT, load_golden
from fake_engine import FakeEngine

from vapor_amd import _lib as L

GOLD = load_golden("kmerhits_anyk.json.gz")


def test_new_names_importable():
    from vapor_vali.Simple_function import key_modify, kmerhits, subkeys  # noqa: F401
    from vapor_vali import Simple_function as SF
    assert callable(SF.kmerhits) and callable(SF.subkeys) and callable(SF.key_modify)


def test_subkeys_and_key_modify_golden():
    from vapor_vali.Simple_function import key_modify, subkeys
    for c in GOLD["subkeys"]:
        try:
            got = {"ok": subkeys(c["key"], c["nth_base"], c["inversions"])}
        except Exception as e:  # noqa: BLE001
            got = {"error": type(e).__name__}
        assert got == c["out"], c
    for c in GOLD["key_modify"]:
        assert key_modify(c["key"]) == c["out"], c


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_model_equals_golden(case):
    if "error" in case["out"]:
        with pytest.raises(KeyError):
            model.kmerhits(case["s1"], case["s2"], case["k"], case["inversions"])
        return
    got = model.kmerhits(case["s1"], case["s2"], case["k"], case["inversions"])
    assert model.matches(case["out"]["ok"], got), case["name"]


def test_bit_parallel_distance_equals_dp():
    rng = np.random.default_rng(1)
    for k in (41, 45, 50, 57, 63, 64):
        keys = rng.choice(np.frombuffer(b"ACGTNn", dtype=np.uint8), size=(40, k))
        for _ in range(6):
            q = bytes(rng.choice(np.frombuffer(b"ACGTNn", dtype=np.uint8), size=k))
            d = model.lev_many(q, keys)
            assert d.tolist() == [model.lev_dp(q, bytes(r)) for r in keys]
        base = bytes(keys[0])
        near = [base[1:] + b"A", b"C" + base[:-1], base[:5] + base[6:] + b"G", base[:k // 2] + b"T" + base[k // 2:-1]]
        d = model.lev_many(base, np.frombuffer(b"".join(near), dtype=np.uint8).reshape(len(near), k))
        assert d.tolist() == [model.lev_dp(base, r) for r in near]


def test_limits_raise_value_error():
    from vapor_vali.Simple_function import kmerhits
    with pytest.raises(ValueError, match="VAPOR_MAX_ANY_K"):
        kmerhits("ACGT" * 20, "ACGT" * 20, 65)
    with pytest.raises(ValueError, match="VAPOR_MAX_ANY_K"):
        kmerhits("ACGT" * 20, "ACGT" * 20, 0)
    for nb in (0, 2, 3):
        with pytest.raises(ValueError, match="nth_base"):
            kmerhits("ACGT" * 20, "ACGT" * 20, 15, nb)
    with pytest.raises(ValueError, match="VAPOR_MAX_WIDE_SEQ_LEN"):
        kmerhits("A" * (L.MAX_WIDE_SEQ_LEN + 1), "ACGT", 15)


class AnykFakeEngine(FakeEngine):
    """FakeEngine plus score_anyk: records the pairs it was given and answers with the oracle's record (no DIR words)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.anyk_pairs = []

    def score_anyk(self, ss, pairs, want_hits=False):
        assert not want_hits
        st = np.zeros((len(pairs), 16), dtype=np.int64)
        for t, p in enumerate(pairs):
            self.anyk_pairs.append(int(p["k"]))
            s1, s2 = ss.seqs[int(p["seq1"])], ss.seqs[int(p["seq2"])]
            st[t] = self.orc.pair_stats(int(p["k"]), s1, s2[int(p["off2"]):])
        return st


def _requests(k):
    from vapor_amd.drivers import Score
    c = [c for c in GOLD["scorers"] if c["k"] == 15][0]
    return [Score(kind, c["ref"], c["alt"], [(c["read"], c["miss"])], k) for kind in ("s1", "s2", "s3", "del")]


def test_routing_with_and_without_the_route(oracle):
    from vapor_amd import pipeline
    with_route = AnykFakeEngine(oracle)
    assert pipeline.has_anyk(with_route)
    out = pipeline.score_requests(with_route, _requests(15))
    assert all(isinstance(v, list) for v in out), out
    assert with_route.anyk_pairs and set(with_route.anyk_pairs) == {15}
    without = FakeEngine(oracle)
    assert not pipeline.has_anyk(without)
    out = pipeline.score_requests(without, _requests(15))
    assert all(isinstance(v, ValueError) and "unsupported window size" in str(v) for v in out), out
    # a window size the CLI uses stays on the plan route
    with_route.anyk_pairs.clear()
    pipeline.score_requests(with_route, _requests(10))
    assert with_route.anyk_pairs == []


def test_scorer_call_routing(oracle, monkeypatch):
    from vapor_amd import pipeline
    from vapor_vali import Simple_function as SF
    c = [c for c in GOLD["scorers"] if c["k"] == 15][0]
    x = [c["read"], c["miss"], "r"]
    eng = AnykFakeEngine(oracle)
    monkeypatch.setattr(pipeline, "_engine", eng)
    a = SF.calcu_vapor_single_read_score_within_10Perc_m1b(c["ref"], c["alt"], x, 15)
    assert [float(v) for v in a] == [float(v) for v in c["s2"]["ok"]]
    assert eng.anyk_pairs == [15, 15]
    with pytest.raises(ValueError, match="VAPOR_MAX_ANY_K"):
        SF.calcu_vapor_single_read_score_within_10Perc_m1b(c["ref"], c["alt"], x, 65)
    monkeypatch.setattr(pipeline, "_engine", FakeEngine(oracle))
    with pytest.raises(ValueError, match="unsupported window size"):
        SF.calcu_vapor_single_read_score_within_10Perc_m1b(c["ref"], c["alt"], x, 15)


def test_twin_stub_refuses():
    from oracle import oracle as orc
    lib = ctypes.CDLL(orc.build_twin())
    fn = lib.vapor_anyk_batch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert fn(None, None, 0, None, None, None, 0, None) == L.E_ARG


def test_header_and_exports_agree():
    with open(os.path.join(ROOT, "include", "vapor_hip.h")) as f:
        h = f.read()
    assert re.search(r"\bint vapor_anyk_batch\(", h)
    assert "vapor_anyk_batch" in L.EXPORTS and "vapor_anyk_batch" in L.OPTIONAL_EXPORTS
    assert int(re.search(r"#define VAPOR_MAX_ANY_K (\d+)", h).group(1)) == L.MAX_ANY_K
    assert int(re.search(r"#define VAPOR_PF_FORWARD (\d+)u", h).group(1)) == L.PF_FORWARD
