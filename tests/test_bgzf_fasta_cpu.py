"""Bgzipped reference FASTA (.fa.gz + .fai + .gzi) on the host: seqio.BgzfFasta against FaiFasta on the plain twin of the same
file, the opener's choice and refusals, damaged blocks, the CLI from files, and the CPU twin's refusal of the device call."""
import ctypes
import gzip
import os
import random
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import load_golden
from fake_engine import FakeEngine
from vapor_amd import cli, pipeline, seqio, synth

_IUPAC = "ACGTACGTACGTNacgtnRYKMSWBDHV"


def _contigs(seed=5):
    rnd = random.Random(seed)
    big = []
    for i in range(90000):
        if i % 9000 < 300:
            big.append("N")                                  # N runs
        elif i % 20000 < 2000:
            big.append(rnd.choice("acgtn"))                  # soft-masked stretches
        else:
            big.append(rnd.choice(_IUPAC))
    return {"chr1": "".join(big), "short": "ACGTN" * 5, "tiny": "ac", "chr2": "".join(rnd.choice("ACGT") for _ in range(7001))}


def _pair(tmp_path, contigs, line_width, block_size, crlf, gzi=True):
    """(BgzfFasta, FaiFasta of its plain twin)."""
    d = tmp_path / ("w%d_b%d_%d" % (line_width, block_size, crlf))
    d.mkdir(exist_ok=True)
    gz = str(d / "ref.fa.gz")
    seqio.write_bgzf_fasta(gz, contigs, line_width=line_width, block_size=block_size, crlf=crlf)
    plain = str(d / "ref.fa")
    with open(plain, "wb") as f:
        f.write(gzip.open(gz).read())
    with open(plain + ".fai", "w") as f:
        f.write(open(gz + ".fai").read())
    if not gzi:
        os.remove(gz + ".gzi")
    return seqio.open_fasta(gz), seqio.open_fasta(plain)


def _windows(fa_plain, rnd, n):
    """Random windows, plus those that end exactly on block and line boundaries, clipped ends, unknown contigs, empty ranges."""
    out = []
    names = list(fa_plain.index)
    for _ in range(n):
        c = rnd.choice(names)
        length = fa_plain.index[c][0]
        s = rnd.randint(-20, length + 20)
        out.append((c, s, s + rnd.randint(-3, 12000)))
    for c in names:
        length, _off, lb, _lw = fa_plain.index[c]
        out += [(c, 1, length), (c, -5, 3), (c, length - 2, length + 50), (c, lb, lb), (c, lb + 1, 2 * lb), (c, 5, 4)]
    out += [("chrNope", 1, 100), ("chr1", 0, 0)]
    return out


@pytest.mark.parametrize("line_width", [60, 70, 80])
@pytest.mark.parametrize("block_size", [65280, 1000])
@pytest.mark.parametrize("crlf", [False, True])
def test_fetch_and_lines_equal_the_plain_twin(tmp_path, line_width, block_size, crlf):
    contigs = _contigs()
    bz, fa = _pair(tmp_path, contigs, line_width, block_size, crlf)
    assert isinstance(bz, seqio.BgzfFasta) and isinstance(fa, seqio.FaiFasta)
    rnd = random.Random(line_width * 7 + block_size + crlf)
    wins = _windows(fa, rnd, 150)
    # windows whose raw text ends exactly where a block ends
    for k in range(1, min(len(bz.uoff), 40)):
        u = int(bz.uoff[k])
        for c, (length, off, lb, lw) in fa.index.items():
            if off <= u - 1 < off + length + length // lb * (lw - lb) + lw:
                r = u - 1 - off
                if r % lw < lb:
                    pos = r // lw * lb + r % lb + 1
                    wins += [(c, max(pos - 500, 1), pos), (c, pos, pos + 700)]
    for c, s, e in wins:
        assert bz.fetch(c, s, e) == fa.fetch(c, s, e), (c, s, e)
    for c, s, e in [w for w in wins if w[1] >= 0][:60] + [("chr1", 1, 10), ("tiny", 1, 2)]:
        region = "%s:%d-%d" % (c, s, e)
        assert bz.lines(region) == fa.lines(region)
    assert bz.lines("short") == fa.lines("short")
    assert bz.fetch("short", 1, 25) == contigs["short"] and bz.fetch("chr1", 1, 90000) == contigs["chr1"]


def test_a_missing_gzi_is_built_from_the_block_headers(tmp_path):
    contigs = _contigs(7)
    with_gzi, fa = _pair(tmp_path, contigs, 60, 1000, False)
    bz, _ = _pair(tmp_path, contigs, 60, 1000, False, gzi=False)
    assert not os.path.exists(bz.path + ".gzi")
    assert np.array_equal(bz.coff, with_gzi.coff) and np.array_equal(bz.uoff, with_gzi.uoff)
    for c, s, e in _windows(fa, random.Random(3), 100):
        assert bz.fetch(c, s, e) == fa.fetch(c, s, e)
    assert sorted(os.listdir(os.path.dirname(bz.path))) == ["ref.fa", "ref.fa.fai", "ref.fa.gz", "ref.fa.gz.fai"]


def test_gzi_layout_is_htslibs(tmp_path):
    """A little-endian uint64 count, then (compressed, uncompressed) uint64 pairs of every block after the first."""
    gz = str(tmp_path / "r.fa.gz")
    seqio.write_bgzf_fasta(gz, {"c": "ACGT" * 1000}, block_size=1000)
    raw = open(gz + ".gzi", "rb").read()
    n = struct.unpack_from("<Q", raw)[0]
    pairs = [struct.unpack_from("<QQ", raw, 8 + 16 * i) for i in range(n)]
    data = gzip.open(gz).read()
    assert len(raw) == 8 + 16 * n and [u for _c, u in pairs] == list(range(1000, len(data), 1000)) + [len(data)]
    blob = open(gz, "rb").read()
    for c, _u in pairs:
        assert blob[c:c + 4] == b"\x1f\x8b\x08\x04"


def test_eight_threads_fetch_at_once(tmp_path):
    bz, fa = _pair(tmp_path, _contigs(9), 60, 1000, False)
    wins = _windows(fa, random.Random(8), 400)
    with ThreadPoolExecutor(max_workers=8) as pool:
        got = list(pool.map(lambda w: bz.fetch(*w), wins))
    assert got == [fa.fetch(*w) for w in wins]


@pytest.mark.parametrize("flag", ["FALSE", "TRUE"])
def test_ref_seq_readin_on_the_inprocess_backend(tmp_path, flag):
    bz, fa = _pair(tmp_path, _contigs(4), 70, 1000, False)
    seqio.set_backend(seqio.InProcessBam())
    try:
        for c, s, e in _windows(fa, random.Random(2), 80):
            assert seqio.ref_seq_readin(bz.path, c, s, e, flag) == seqio.ref_seq_readin(fa.path, c, s, e, flag)
        assert isinstance(seqio.get_backend()._fasta(bz.path), seqio.BgzfFasta)
        assert type(seqio.get_backend()._fasta(fa.path)) is seqio.FaiFasta
    finally:
        seqio.set_backend(None)


def test_plain_gzip_is_refused_by_name(tmp_path):
    data = b">c\nACGTACGT\n"
    p = str(tmp_path / "ref.fa.gz")
    with open(p, "wb") as f:
        f.write(gzip.compress(data))
    with open(p + ".fai", "w") as f:
        f.write("c\t8\t3\t60\t61\n")
    with pytest.raises(ValueError, match="bgzip"):
        seqio.open_fasta(p)
    be = seqio.InProcessBam()
    with pytest.raises(ValueError, match="bgzip"):
        be.fetch_seq(p, "c", 1, 8)
    with pytest.raises(ValueError, match="bgzip"):
        seqio.BgzfFasta(p)


def _corrupt(path, k, what):
    bz = seqio.BgzfFasta(path)
    c = int(bz.coff[k])
    blob = bytearray(open(path, "rb").read())
    bsize = struct.unpack_from("<H", blob, c + 16)[0] + 1
    if what == "crc":
        blob[c + bsize - 8] ^= 0x5A
    else:
        struct.pack_into("<H", blob, c + 16, bsize - 1 - 40)
    open(path, "wb").write(bytes(blob))
    return int(bz.uoff[k]), int(bz.uoff[k + 1])


@pytest.mark.parametrize("what", ["crc", "bsize"])
def test_a_damaged_block_raises_and_returns_no_bases(tmp_path, what):
    contigs = _contigs(6)
    _bz, fa = _pair(tmp_path, contigs, 60, 1000, False)
    gz = os.path.join(os.path.dirname(fa.path), "ref.fa.gz")
    u0, u1 = _corrupt(gz, 20, what)
    bz = seqio.BgzfFasta(gz)
    length, off, lb, lw = fa.index["chr1"]
    r = u0 - off + 100                                       # a base of the damaged block (blocks of 1 000 bytes)
    inside = r // lw * lb + min(r % lw, lb - 1) + 1
    with pytest.raises(ValueError, match="BGZF"):
        bz.fetch("chr1", inside, inside + 10)
    with pytest.raises(ValueError, match="BGZF"):
        bz.fetch("chr1", max(inside - 3000, 1), inside + 3000)
    far = (u1 - off) // lw * lb + 2000                       # blocks after it still read
    assert bz.fetch("chr1", far, far + 500) == fa.fetch("chr1", far, far + 500)
    assert bz.fetch("chr1", 1, 100) == fa.fetch("chr1", 1, 100)


# ---- the CLI from files: the same table from the bgzipped reference as from the plain one ---------------------------------
@pytest.fixture()
def fake(oracle):
    e = FakeEngine(oracle)
    pipeline.set_engine(e)
    yield e
    pipeline.set_engine(None)
    seqio.set_backend(None)


LOCUS = load_golden("locus_bed.json.gz")["cases"]
VCF = load_golden("locus_vcf.json.gz")["cases"]
_VCF_WORLDS = {c["name"]: c["world"] for c in VCF if c["world"] is not None}


def _sorted_world(w):
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    return w


def _both_refs(world, tmp_path):
    dp, dz = tmp_path / "plain", tmp_path / "bgz"
    dp.mkdir()
    dz.mkdir()
    fa, bam = synth.write_world_files(world, str(dp))
    fz, bamz = synth.write_world_files(world, str(dz), bgzip_reference=True)
    assert fz.endswith(".fa.gz") and gzip.open(fz).read() == open(fa, "rb").read()
    assert open(fz + ".fai").read() == open(fa + ".fai").read()
    assert open(bamz, "rb").read() == open(bam, "rb").read()
    return (fa, bam, dp), (fz, bamz, dz)


@pytest.mark.parametrize("case", [c for c in LOCUS if not [p for p in c["per_locus"] if "error" in p["scores"]]][:3],
                         ids=lambda c: c["name"])
def test_bed_cli_from_a_bgzipped_reference(fake, case, tmp_path):
    world = _sorted_world(synth.world_from_json(case["world"]))
    bed = tmp_path / "in.bed"
    bed.write_text(case["bed"])
    got = []
    for ref, bam, d in _both_refs(world, tmp_path):
        seqio.set_backend(seqio.InProcessBam())
        try:
            out = d / "out.vapor"
            assert cli.main(["bed", "--sv-input", str(bed), "--reference", ref, "--pacbio-input", bam,
                             "--output-path", str(d / "figs"), "--output-file", str(out), "--no-figures"]) == 0
            got.append(out.read_bytes())
        finally:
            seqio.set_backend(None)
    assert got[0] == got[1] and len(got[0].splitlines()) == len(case["vapor_text"].splitlines())


@pytest.mark.parametrize("case", [c for c in VCF if c["world"] is not None][:2], ids=lambda c: c["name"])
def test_vcf_cli_from_a_bgzipped_reference(fake, case, tmp_path):
    world = _sorted_world(synth.world_from_json(_VCF_WORLDS[case["name"]]))
    got = []
    for ref, bam, d in _both_refs(world, tmp_path):
        vcf = d / "in.vcf"
        vcf.write_text(case["vcf"])
        seqio.set_backend(seqio.InProcessBam())
        try:
            assert cli.main(["vcf", "--sv-input", str(vcf), "--reference", ref, "--pacbio-input", bam,
                             "--output-path", str(d / "figs"), "--output-file", "unused", "--no-figures"]) == 0
            got.append((d / "in.vcf.vapor").read_bytes())
        finally:
            seqio.set_backend(None)
    assert got[0] == got[1] and len(got[0].splitlines()) > 1


def test_default_world_files_are_unchanged(tmp_path):
    """The option writes the bgzipped reference; without it the files are what they were: plain FASTA + .fai."""
    w = synth.make_world(seed=2, n_loci=3, svtypes=("DEL",), span_range=(100, 300), read_len=800, n_reads=3)
    fa, _bam = synth.write_world_files(w, str(tmp_path))
    assert fa.endswith("ref.fa") and not os.path.exists(fa + ".gz")
    text = open(fa).read()
    assert text.startswith(">") and "\r" not in text and all(len(ln) <= 60 for ln in text.splitlines())


# ---- the CPU twin exports the device call and refuses it ------------------------------------------------------------------
def test_cpu_twin_refuses_the_device_call(oracle):
    from vapor_amd import _lib
    lib = _lib.bind(ctypes.CDLL(oracle.build_twin()))
    for name in ("vapor_fasta_windows_device", "vapor_fasta_last_stats"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    vb = np.zeros(1, dtype=np.uint64)
    off = np.zeros(2, dtype=np.int64)
    tr = np.zeros(1, dtype=np.uint8)
    st = np.zeros(1, dtype=np.int32)
    text = np.zeros(16, dtype=np.uint8)
    vp = ctypes.c_void_p
    assert lib.vapor_fasta_windows_device(None, 0, 1, vb.ctypes.data_as(vp), vb.ctypes.data_as(vp), text.ctypes.data_as(vp), 16,
                                          off.ctypes.data_as(vp), tr.ctypes.data_as(vp), st.ctypes.data_as(vp)) == _lib.E_ARG
    out = np.zeros(6, dtype=np.float64)
    assert lib.vapor_fasta_last_stats(None, out.ctypes.data_as(vp), 6) == _lib.E_ARG
