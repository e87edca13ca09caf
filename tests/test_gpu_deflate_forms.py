"""Both device readers (vapor_fasta_windows_device, vapor_bam_chop_device: one bgzf_inflate_kernel behind them) on BGZF blocks that
are legal DEFLATE but nothing zlib's encoder writes - tests/deflate_forms.py encodes every block: codes of 15 bits with the widest
extra fields, the widest dynamic header behind a fixed-code block, blocks of matches with the next header right behind them,
stored blocks (empty ones too) between Huffman blocks, free token choices with distance 1, overlapping and 32 K-distant matches,
a block that ends at byte 65 536 with a 258-byte match.  Every block must be inflated ON THE DEVICE (status 0: handing a valid
block to the host route is the failure looked for) and the FASTA texts are compared with the source strings themselves."""
import random

import numpy as np
import pytest

import deflate_forms
import test_bamio as TB
import test_gpu_bgzf_fasta as TF
from test_gpu_bamdev import compare
from vapor_amd import bamio, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _contigs(seed, scale=1):
    """About 200 kb (times scale): random bases with homopolymer runs, tandem repeats and N stretches (distance 1, distances below the length),
    and copies of stretches 17 - 30 kb back (long matches at the widest distances)."""
    rnd = random.Random(seed)

    def contig(n):
        out = []
        size = 0
        while size < n:
            r = rnd.random()
            if r < 0.55:
                piece = "".join(rnd.choices("ACGT", k=rnd.randint(50, 900)))
            elif r < 0.65:
                piece = rnd.choice("ACGTN") * rnd.randint(5, 700)
            elif r < 0.8:
                piece = "".join(rnd.choices("ACGT", k=rnd.randint(2, 70))) * rnd.randint(3, 40)
            elif r < 0.85:
                piece = "".join(rnd.choices("acgtn", k=rnd.randint(10, 300)))
            elif size > 31000:
                whole = "".join(out)
                a = size - rnd.randint(17000, 30000)
                piece = whole[a:a + rnd.randint(150, 1500)]
                out = [whole]
            else:
                continue
            out.append(piece)
            size += len(piece)
        return "".join(out)[:n]
    return {"chr1": contig(120000 * scale), "chr2": contig(70001 * scale), "tiny": "ac", "chr3": contig(9999)}


def _cover(contigs, step=9000):
    """Windows (chrom, start, end), 1-based and closed, that together cover every base of every contig."""
    return [(c, s, min(s + step - 1, len(seq))) for c, seq in contigs.items() for s in range(1, len(seq) + 1, step)]


def _check_fasta(eng, gz, contigs):
    bz = seqio.BgzfFasta(gz)
    wins = _cover(contigs)
    keep, texts, _traits, status, blocks = TF._device(eng, bz, wins)
    assert len(keep) == len(wins)
    assert status.tolist() == [0] * len(wins), [(wins[i], int(s)) for i, s in enumerate(status) if s]
    for q, (c, s, e) in enumerate(wins):
        assert texts[q] == contigs[c][s - 1:e], (c, s, e)
    n_blocks = len(TB._blocks(open(gz, "rb").read())) - 1             # (the end-of-file block holds no text)
    assert len(blocks) == n_blocks and eng.fasta_last_stats()["blocks"] == n_blocks
    return n_blocks


@pytest.mark.parametrize("block_size", [1500, 65280])
def test_fasta_blocks_of_every_family_are_inflated_on_the_device(eng, tmp_path, monkeypatch, block_size):
    # (200 kb are 136 blocks of 1 500 bytes; of 65 280 bytes they would be four - 400 kb are seven, one and more a family)
    contigs = _contigs(block_size, 1 if block_size == 1500 else 2)
    log = []
    monkeypatch.setattr(bamio, "_bgzf_block", deflate_forms.bgzf_block_maker(block_size, deflate_forms.FAMILIES, log))
    gz = seqio.write_bgzf_fasta(str(tmp_path / "ref.fa.gz"), contigs, 60, block_size)
    monkeypatch.undo()
    # every family reached the file (size_edge: a block whose last token is a match that ends with it, where the text has one)
    assert {fam for fam, _n in log} == set(deflate_forms.FAMILIES)
    if block_size == 65280:
        assert max(n for _fam, n in log) > 2 * 1280                     # (a stream the LDS copy is topped up for again and again)
    n_blocks = _check_fasta(eng, gz, contigs)
    assert n_blocks == len(log) >= 6


def test_a_fasta_block_of_65536_bytes_that_ends_with_a_258_byte_match(eng, tmp_path, monkeypatch):
    rnd = random.Random(65536)
    # lines of 60 bases + newline; the last 3 kb in front of byte 65 536 repeat one line, so the block's last 258 bytes stand 61 back
    line = "".join(rnd.choices("ACGT", k=60))
    n_lines = 65536 // 61 + 30
    seq = "".join(rnd.choices("ACGT", k=(n_lines - 80) * 60)) + line * 80
    contigs = {"c": seq}
    log = []
    monkeypatch.setattr(bamio, "_bgzf_block", deflate_forms.bgzf_block_maker(7, ("size_edge",), log))
    gz = seqio.write_bgzf_fasta(str(tmp_path / "ref.fa.gz"), contigs, 60, 65536)
    monkeypatch.undo()
    raw = open(gz, "rb").read()
    first = TB._blocks(raw)[0]
    assert log[0][0] == "size_edge" and int.from_bytes(raw[first[0] + first[1] - 4:first[0] + first[1]], "little") == 65536
    # the first block's last token is a match of 258 bytes from 61 back that ends at byte 65 536
    text = (">c\n" + "".join(seq[i:i + 60] + "\n" for i in range(0, len(seq), 60))).encode()
    assert deflate_forms.final_match(text[:65536]) == (258, 61)
    assert _check_fasta(eng, gz, contigs) == 2


def test_bam_blocks_of_long_codes_match_queue_and_mixed_forms(eng, tmp_path, monkeypatch):
    log = []
    monkeypatch.setattr(bamio, "_bgzf_block", deflate_forms.bgzf_block_maker(62, ("long_codes", "match_queue", "mixed"), log))
    w = synth.make_world(seed=62, n_loci=10, svtypes=("DEL", "INS"), span_range=(100, 1500), read_len=5000, n_reads=22)
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    fa, bam = synth.write_world_files(w, str(tmp_path), block_size=30000)
    monkeypatch.undo()
    assert {fam for fam, _n in log} == {"long_codes", "match_queue", "mixed"} and len(log) > 10
    status, n = compare(eng, bam, [(l.chrom, max(l.start - 300, 1), l.start + 700, 300) for l in w.loci])
    assert status.tolist() == [0] * len(w.loci) and n > 60
