"""Reference windows of a bgzipped FASTA cut on the device (vapor_fasta_windows_device: bgzf_inflate_kernel, fasta_window_kernel)
against the host reader (seqio.BgzfFasta, itself pinned on FaiFasta of the plain twin in tests/test_bgzf_fasta_cpu.py): the
texts byte for byte and the traits, over line widths 60/70/80, CRLF, blocks of 65 280 and of 1 000 bytes, windows that share
blocks and windows that end on block boundaries; the distinct blocks inflated; a damaged block and a non-ASCII byte (their
windows go to the host, their neighbours do not); then `vapor bed` / `vapor vcf` from a bgzipped reference against the plain one."""
import os
import random
import struct

import numpy as np
import pytest

from vapor_amd import _lib as L
from vapor_amd import bamio, cli, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _contigs(seed):
    rnd = random.Random(seed)
    big = []
    for i in range(150000):
        if i % 11000 < 400:
            big.append("N")
        elif i % 23000 < 3000:
            big.append(rnd.choice("acgtn"))
        elif i % 37000 < 50:
            big.append(rnd.choice("RYKMSWBDHV"))
        else:
            big.append(rnd.choice("ACGT"))
    return {"chr1": "".join(big), "short": "ACGTN" * 5, "tiny": "ac", "chr2": "".join(rnd.choice("ACGT") for _ in range(20001))}


def _host_traits(text: str) -> int:
    b = text.encode("latin-1")
    t = 0
    if any(97 <= c <= 122 for c in b):
        t |= L.FASTA_TR_LOWER
    if b.translate(None, b"ACGTN"):
        t |= L.FASTA_TR_NOT_ACGTN
    if b.translate(None, b"ACGTNacgtn"):
        t |= L.FASTA_TR_NOT_ACGTN_ANY_CASE
    if any(c >= 0x80 for c in b):
        t |= L.FASTA_TR_HIGH
    return t


def _windows(bz, rnd, n):
    """(chrom, start, end): random windows of up to 12 kb, runs of neighbours that overlap (shared blocks), windows that end
    exactly on a block boundary."""
    out = []
    names = [c for c in bz.index]
    for _ in range(n):
        c = rnd.choice(names)
        length = bz.index[c][0]
        s = rnd.randint(1, length)
        out.append((c, s, s + rnd.randint(0, 12000)))
        if rnd.random() < 0.3:
            out.append((c, s + rnd.randint(0, 3000), s + rnd.randint(3000, 9000)))
    length, off, lb, lw = bz.index["chr1"]
    for k in range(1, len(bz.uoff) - 1):
        r = int(bz.uoff[k]) - 1 - off
        if 0 <= r < length // lb * lw and r % lw < lb:
            pos = r // lw * lb + r % lw + 1
            out += [("chr1", max(pos - 800, 1), pos), ("chr1", pos + 1, pos + 900)]
    return out


def _device(eng, bz, wins):
    rng = [bz.raw_range(*w) for w in wins]
    keep = [i for i, r in enumerate(rng) if r is not None]
    first = np.asarray([rng[i][0] for i in keep], dtype=np.int64)
    last = np.asarray([rng[i][1] for i in keep], dtype=np.int64)
    vb, ve = bz.virtual(first), bz.virtual(last)
    assert (vb >= 0).all() and (ve >= 0).all()
    texts, traits, status = eng.fasta_windows_device(bz._fd, vb, ve, int((last - first).sum()))
    blocks = set()
    for a, b in zip(first.tolist(), last.tolist()):
        blocks.update(range(int(bz.block_of(a)), int(bz.block_of(b - 1)) + 1))
    return keep, texts, traits, status, blocks


@pytest.mark.parametrize("line_width,block_size,crlf", [(60, 65280, False), (70, 1000, False), (80, 1000, True), (60, 1000, True), (80, 65280, False)])
def test_device_windows_equal_the_host_reader(eng, tmp_path, line_width, block_size, crlf):
    assert check_device_windows(eng, tmp_path, line_width, block_size, crlf, 700) >= 900


def check_device_windows(eng, tmp_path, line_width, block_size, crlf, n_draws):
    """The body of the test above at n_draws random windows (and the block-boundary windows of chr1); returns how many windows there were."""
    gz = seqio.write_bgzf_fasta(str(tmp_path / "ref.fa.gz"), _contigs(line_width + block_size), line_width, block_size, crlf)
    bz = seqio.BgzfFasta(gz)
    wins = _windows(bz, random.Random(block_size + line_width), n_draws)
    keep, texts, traits, status, blocks = _device(eng, bz, wins)
    assert status.tolist() == [0] * len(keep)
    for q, i in enumerate(keep):
        exp = bz.fetch(*wins[i])
        assert texts[q] == exp, (wins[i], len(texts[q]), len(exp))
        assert int(traits[q]) == _host_traits(exp), wins[i]
    st = eng.fasta_last_stats()
    assert st["windows"] == len(keep) and st["blocks"] == len(blocks)
    assert st["inflated_bytes"] >= 0.9 * sum(len(bz.block(k)) for k in blocks) and st["compressed_bytes"] > 0 and st["kernel_ms"] > 0
    # fastpath._window_traits and the isascii check say what the traits say
    from vapor_amd import fastpath
    for q in range(0, len(keep), 7):
        up, nocomp = fastpath._window_traits(texts[q])
        t = int(traits[q])
        assert nocomp == bool(t & L.FASTA_TR_NOT_ACGTN_ANY_CASE)
        if not t & L.FASTA_TR_NOT_ACGTN:
            assert up
    return len(wins)


def test_a_foreign_subfield_in_front_of_bc_in_every_block(eng, tmp_path, monkeypatch):
    """XLEN 12 in every block.  Two contigs of 100 kb in blocks of 20 000 bytes: a stretch holds several blocks, and some windows
    end exactly on a block boundary or start right behind one."""
    import test_bamio as TB
    rnd = random.Random(12)
    TB.foreign_subfield_writer(monkeypatch)
    gz = seqio.write_bgzf_fasta(str(tmp_path / "ref.fa.gz"), {"chr1": "".join(rnd.choice("ACGT") for _ in range(100000)),
                                                             "chr2": "".join(rnd.choice("ACGTN") for _ in range(100000))}, 60, 20000)
    monkeypatch.undo()
    assert all(xlen == 12 for _off, _bsize, xlen in TB._blocks(open(gz, "rb").read()))
    bz = seqio.BgzfFasta(gz)
    wins = _windows(bz, random.Random(13), 9)
    on_boundary = sum(1 for w in wins if int(bz.raw_range(*w)[1]) in bz.uoff.tolist() or int(bz.raw_range(*w)[0]) in bz.uoff.tolist())
    assert 18 <= len(wins) <= 24 and on_boundary >= 4
    keep, texts, traits, status, blocks = _device(eng, bz, wins)
    assert len(keep) == len(wins) and status.tolist() == [0] * len(keep)
    for q, i in enumerate(keep):
        exp = bz.fetch(*wins[i])
        assert texts[q] == exp and int(traits[q]) == _host_traits(exp), wins[i]
    assert eng.fasta_last_stats()["blocks"] == len(blocks) > 5


def test_a_damaged_block_sends_exactly_its_windows_to_the_host(eng, tmp_path):
    gz = seqio.write_bgzf_fasta(str(tmp_path / "ref.fa.gz"), _contigs(3), 60, 1000)
    bz = seqio.BgzfFasta(gz)
    k = 40
    c = int(bz.coff[k])
    blob = bytearray(open(gz, "rb").read())
    bsize = struct.unpack_from("<H", blob, c + 16)[0] + 1
    blob[c + bsize - 8] ^= 0x33                               # its CRC-32
    open(gz, "wb").write(bytes(blob))
    bz = seqio.BgzfFasta(gz)
    wins = _windows(bz, random.Random(4), 300)
    keep, texts, traits, status, _blocks = _device(eng, bz, wins)
    n_bad = 0
    for q, i in enumerate(keep):
        a, b = bz.raw_range(*wins[i])
        hit = int(bz.block_of(a)) <= k <= int(bz.block_of(b - 1))
        if hit:
            n_bad += 1
            assert status[q] == L.FASTA_BLOCK and texts[q] is None, wins[i]
            with pytest.raises(ValueError, match="CRC32"):
                bz.fetch(*wins[i])
        else:
            assert status[q] == 0 and texts[q] == bz.fetch(*wins[i]), wins[i]
    assert n_bad >= 3 and (status != 0).sum() == n_bad


def test_a_non_ascii_byte_is_left_to_the_host_which_raises(eng, tmp_path):
    seq = bytearray(b"ACGT" * 3000)
    seq[5000] = 0xE9
    body = b">c\n" + b"".join(bytes(seq[i:i + 60]) + b"\n" for i in range(0, len(seq), 60))
    gz = str(tmp_path / "ref.fa.gz")
    with open(gz, "wb") as f:
        for u in range(0, len(body), 1000):
            f.write(bamio._bgzf_block(body[u:u + 1000]))
        f.write(bamio._BGZF_EOF)
    with open(gz + ".fai", "w") as f:
        f.write("c\t%d\t3\t60\t61\n" % len(seq))
    bz = seqio.open_fasta(gz)                                # (no .gzi: the table from the block headers)
    wins = [("c", 4900, 5100), ("c", 1, 4000), ("c", 5002, 9000), ("c", 5001, 5001)]
    keep, texts, traits, status, _b = _device(eng, bz, wins)
    assert status.tolist() == [L.FASTA_NON_ASCII, 0, 0, L.FASTA_NON_ASCII]
    assert traits[0] & L.FASTA_TR_HIGH and texts[0] is None
    assert texts[1] == bz.fetch("c", 1, 4000) and texts[2] == bz.fetch("c", 5002, 9000)
    with pytest.raises(UnicodeDecodeError):
        bz.fetch("c", 4900, 5100)


# ---- the CLI: bgzipped reference against the plain one ------------------------------------------------------------------
@pytest.fixture()
def spy(monkeypatch):
    """Every fasta_windows_device call of the run: (windows, windows answered, the engine's last stats)."""
    calls = []
    orig = Engine.fasta_windows_device

    def wrapped(self, *a, **k):
        got = orig(self, *a, **k)
        calls.append((len(got[0]), int((got[2] == 0).sum()), self.fasta_last_stats()))
        return got
    monkeypatch.setattr(Engine, "fasta_windows_device", wrapped)
    monkeypatch.setenv("VAPOR_QC_SEED", "7")
    return calls


def _tables(w, tmp_path, mode, text, figures=False):
    out = {}
    for bgz in (False, True):
        d = tmp_path / ("bgz" if bgz else "plain")
        d.mkdir(exist_ok=True)
        fa, bam = synth.write_world_files(w, str(d), block_size=0xFF00, bgzip_reference=bgz)
        inp = d / ("in." + mode)
        inp.write_text(text)
        res = d / "out.vapor"
        seqio.set_backend(seqio.InProcessBam())
        try:
            assert cli.main([mode, "--sv-input", str(inp), "--reference", fa, "--pacbio-input", bam, "--output-path", str(d / "figs"),
                             "--output-file", str(res)] + ([] if figures else ["--no-figures"])) == 0
        finally:
            seqio.set_backend(None)
        out[bgz] = (d / "in.vcf.vapor" if mode == "vcf" else res).read_bytes()
    return out


def _world(seed, n):
    w = synth.make_world(seed=seed, n_loci=n, svtypes=("DEL", "INV", "INS", "TANDUP", "DEL"), span_range=(80, 2500), read_len=6000, n_reads=24)
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    return w


@pytest.mark.parametrize("mode", ["bed", "vcf"])
def test_cli_from_a_bgzipped_reference_is_byte_identical(spy, tmp_path, mode):
    w = _world(71, 60)
    t = _tables(w, tmp_path, mode, synth.bed_text(w) if mode == "bed" else synth.vcf_text(w))
    assert t[True] == t[False] and t[False].count(b"\n") >= (61 if mode == "bed" else 50)
    assert spy and sum(c[1] for c in spy) >= 40                       # the fast route's windows came from the device
    for n, _ok, st in spy:
        assert st["windows"] == n and st["blocks"] > 0 and st["inflated_bytes"] > st["compressed_bytes"] > 0


def test_cli_with_figures_from_a_bgzipped_reference(spy, tmp_path):
    w = _world(72, 12)
    t = _tables(w, tmp_path, "bed", synth.bed_text(w), figures=True)
    assert t[True] == t[False] and t[False].count(b"\n") >= 13


def test_cli_long_insertions_from_a_bgzipped_reference(spy, tmp_path):
    from test_gpu_wide_cli import _world as wide_world
    w = wide_world()
    t = _tables(w, tmp_path, "vcf", synth.vcf_text(w))
    assert t[True] == t[False] and t[False].count(b"\n") >= 6
