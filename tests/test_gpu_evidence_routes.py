"""The routes of the four evidence readers (`--depth`, `--signatures`, `--links`, `--support`) through
seqio.InProcessBam's `*_many`, one test for all four kinds from their modules' reader surface: over one small file, a designed
region and a plain one, an empty window, a contig the file lacks and a region the device hands back by status - the kind's device
method is called once, the native host reader for the handed-back region only, the answers are the native reader's and the
module's statement over bamio's records, and with the smallest batches the device is called more often for the same answers.
The hand-back: for links a record whose aux area is malformed before its SA field (tests/test_gpu_links.py), which the host
reader answers; for the other three a region their rules refuse (tests/test_gpu_depth.py and its likes: status 2), which the
host reader refuses in the library's words."""
import pytest

from vapor_amd import bamio, depth, links, seqio, signature, support
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu

KINDS = {"depth": depth, "signatures": signature, "links": links, "support": support}
N = 4000


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _sa(*entries):
    return b"SAZ" + b"".join(e.encode() + b";" for e in entries) + b"\0"


def _rec(name, pos0, cigar, aux=b"", flag=0):
    import re
    qlen = sum(int(n) for n, c in re.findall(r"(\d+)([MIS=X])", cigar))
    return (name, 0, pos0, cigar, "ACGT" * (qlen // 4) + "C" * (qlen % 4), aux, 60, flag)


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    """One 4 kb contig, 41 records in blocks of 1 kb: a ladder of plain and soft-clipped records, a 60-base D at 1100, an I at
    2100, a molecule split between 1500 and 2500 (two SA tags), and a record clipped at 3500 whose aux area is malformed."""
    cigars = ("200M", "30S170M", "170M35S", "31S100M32S")
    rows = [_rec("r%d" % i, 40 + 110 * i, cigars[i % 4], flag=0x400 if i == 17 else 0) for i in range(34)]
    rows += [_rec("gap", 1000, "100M60D100M"), _rec("gap2", 1040, "60M60D140M"), _rec("ins", 2000, "100M50I100M"),
             _rec("split_l", 1350, "150M40S", _sa("c,2501,+,150S40M,60,0")), _rec("split_r", 2500, "40S150M", _sa("c,1351,+,150M40S,60,0")),
             _rec("split_x", 1380, "120M45S", _sa("zz,9,+,10M,60,0")),
             _rec("malformed", 3380, "120M40S", b"XYq\x01" + _sa("c,3901,+,120S40M,60,0"))]
    assert len(rows) == 41
    p = str(tmp_path_factory.mktemp("gpu_evidence_routes") / "small.bam")
    bamio.write_bam(p, [("c", N)], rows, block_size=1000)
    return p


def regions_of(kind):
    """(designed, plain, empty, handed back): (fields, partner or None) each."""
    if kind == "depth":
        return [((900, 1100, 1160, 1400), None), ((2000, 2400, 2900, 3300), None), ((500, 500, 500, 500), None), ((900, 1200, 1100, 1400), None)]
    if kind == "links":
        left, _right = links.regions("DEL", ["c", 1501, 2500], lambda c: N)
        plain, _ = links.regions("DEL", ["c", 921, 3000], lambda c: N)
        back, _ = links.regions("DEL", ["c", 3501, 3900], lambda c: N)
        return [(left[0][1], b"c"), (plain[0][1], b"c"), ((600,) * 2 + tuple(left[0][1][2:]), b"c"), (back[0][1], b"c")]
    mod = KINDS[kind]
    designed, plain = mod.regions("DEL", ["c", 1101, 1160], N)[0], mod.regions("INS", ["c", 2100, 50], N)[0]
    return [(designed, None), (plain, None), ((600, 600) + tuple(designed[2:]), None), (designed[:4] + (mod.TOL_MAX + 1,) + designed[5:], None)]


class Counting:
    """An engine that counts the calls of its bam_* methods and forwards them."""
    def __init__(self, eng):
        self.eng, self.calls = eng, []

    def __getattr__(self, name):
        f = getattr(self.eng, name)
        if not name.startswith("bam_"):
            return f

        def counted(*a, **k):
            self.calls.append(name)
            return f(*a, **k)
        return counted


@pytest.mark.parametrize("kind", list(KINDS))
def test_one_device_call_the_handed_back_region_to_the_host_and_equal_answers(kind, eng, path, monkeypatch):
    mod = KINDS[kind]
    designed, plain, empty, back = regions_of(kind)
    lo, hi = mod.WINDOW
    native_calls = []
    real_native = getattr(bamio.BamFile, mod.NATIVE)
    monkeypatch.setattr(bamio.BamFile, mod.NATIVE, lambda self, tid, row, *a, **k: native_calls.append(tuple(int(v) for v in row)[:len(back[0])])
                        or real_native(self, tid, row, *a, **k))
    be = seqio.InProcessBam()

    def many(regs, chroms):
        e = Counting(eng)
        args = [e, path, chroms, [f for f, _p in regs]] + ([[p for _f, p in regs]] if mod.LINKED else [])
        try:
            return getattr(be, mod.MANY)(*args), e.calls
        except ValueError as err:
            return err, e.calls

    def by_hand(b, f, p):
        """(the native reader's words, the statement's)"""
        more = (None, p) if mod.LINKED else ()
        row = list(f) + ([0, len(p)] if mod.LINKED else [])
        if mod.LINKED:
            recs = b.fetch_links("c", f[lo] + 1, f[hi], exclude_more=mod.EXCLUDE)
        else:
            recs = [(r[1], r[2]) for r in b.fetch_raw("c", f[lo] + 1, f[hi], exclude_more=mod.EXCLUDE)]
        return real_native(b, 0, row, *more), [int(v) for v in mod.statement(recs, f, p, 0)]
    b = bamio.BamFile(path)
    want = []
    for f, p in (designed, plain):
        host, stated = by_hand(b, f, p)
        assert host == stated and any(host), (kind, f, host, stated)
        want.append(host)
    zero = list(mod.ZERO)
    # the four regions and one on a contig the file lacks: one device call; the handed-back region alone goes to the host reader
    regs, chroms = [designed, empty, plain, designed, back], ["c", "c", "c", "zz", "c"]
    got, calls = many(regs, chroms)
    assert calls == [mod.DEVICE] and native_calls == [tuple(back[0])], (calls, native_calls)
    if kind == "links":
        host, stated = by_hand(b, *back)
        assert host == stated and host[0] >= 1 and host[1] == 0                # clipped there; its SA value is not read
        assert got == [want[0], zero, want[1], zero, host]
    else:
        assert isinstance(got, ValueError) and mod.ENTRIES[0] in str(got)      # the host reader refuses it in the library's words
    # without it: the host reader is not asked, and the answers are its own and the statement's
    native_calls.clear()
    got, calls = many(regs[:4], chroms[:4])
    assert calls == [mod.DEVICE] and not native_calls and got == [want[0], zero, want[1], zero]
    # the smallest batches: a call per region that is read, the same answers
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "0")
    again, calls = many(regs[:4], chroms[:4])
    assert calls == [mod.DEVICE] * 2 and not native_calls and again == got
    # and nothing but zeros needs no device at all
    nothing, calls = many([empty, designed], ["c", "zz"])
    assert nothing == [zero, zero] and not calls
    b.close()
