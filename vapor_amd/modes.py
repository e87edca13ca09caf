"""The run modes of `vapor bed | vcf` that append columns to every row: `--refine`, `--phased` (and `--phase-vcf`, the same mode
with another source of tags), `--both-ends`, `--depth`, `--signatures`, `--links`, `--support` and `--realign`.  At most one holds for a run (the parser refuses every pair); None is the plain
run.  A Mode is everything cli.py and the VCF writer need to know about one; what the option computes stays in
its own module - refine.py, phase.py, bothends.py, depth.py, signature.py, links.py, support.py, realign.py - which gives the mode its columns and the way they travel between ranks;
depth.py to support.py also say how their regions are read (their reader surface), and the parser states the rule once (cli.MODE_OPTIONS)."""
from __future__ import annotations

from . import bothends, depth, junction, links, phase, polish, revote, signature, support
from . import realign as _realign
from . import refine as _refine


class Mode:
    """`name`; `COLUMNS`, the table header's names, and `INFO`, their ##INFO lines as (ID, Type, Number, Description); `keys`,
    the INFO keys of a record in column order, and `skip_dot`, whether a key whose value is '.' is left out; `attr`, the
    attribute of a driver's result that carries the locus's payload; `pack` / `unpack`, the payload as a list of floats for the
    gather across ranks and back (nothing and None for a locus without one); `columns_many`, the fields of every row from the
    payloads.  `phased`: the drivers and the array route run with phased=True.  `chunk_gens`: None, or a hook
    (jobs, rest, gens, engine) -> (gens, held) that may replace a chunk's generators before they run (cli._both_ends_gens).
    `chunk_payloads`: None, or a hook (jobs, todo, engine) -> {t: payload} for a mode whose payload is not a property of a
    driver's result but of the chunk: called once for all of a chunk's loci, whatever route scores them - the four evidence modes'
    is one function over their module's reader surface (cli._evidence_payloads).
    `--refine`'s own: `margin_step` = (M, T), and `ci_of` (cli.vcf_ci_readin: the bounds of a VCF record's candidates).
    `sink`: None, or an object with take(job index, key, payload) that is shown every locus a rank scores, from the chunk's
    thread (`--realign-out`: realign.TraceWriter).  `options`: `--realign`'s realign.Options, what its Realign requests ask for;
    None for every other mode."""
    chunk_gens = None
    chunk_payloads = None
    sink = None
    options = None

    def __init__(self, name, src, attr, keys=None, skip_dot=True, phased=False, margin_step=None, ci_of=None):
        self.name, self.attr, self.skip_dot, self.phased = name, attr, skip_dot, phased
        self.COLUMNS, self.INFO, self.keys = src.COLUMNS, src.INFO, keys or src.COLUMNS
        self.pack, self.unpack, self.columns_many = src.pack, src.unpack, src.columns_many
        self.margin_step, self.ci_of = margin_step, ci_of or {}


def refine(margin, step, ci_of=None) -> Mode:
    """(the record's keys keep the spelling of the reference's own VaPor_GS .. VaPor_REC, and a '.' is written)"""
    return Mode("refine", _refine, "info", ("VaPor_RPOS", "VaPor_REND", "VaPor_QS0", "VaPor_GS0"), False, margin_step=(margin, step),
                ci_of=ci_of)


PHASED = Mode("phased", phase, "phase", phased=True)
BOTH_ENDS = Mode("both-ends", bothends, "views")
DEPTH = Mode("depth", depth, "depth")
SIGNATURES = Mode("signatures", signature, "signatures")
LINKS = Mode("links", links, "links")
SUPPORT = Mode("support", support, "support")


def realign(options=_realign.Options(), sink=None) -> Mode:
    """`--realign` with what the run asks beside it: realign's seven columns, then those of the sections the
    options name, in the order polish, junction, revote (4.25 - 4.27); `sink`, where the loci's traces go (`--realign-out`, 4.24:
    realign.TraceWriter, polish.PolishWriter with `--realign-polish`)."""
    m = Mode("realign", _realign.Chain(x.SECTION for x in (polish, junction, revote) if getattr(options, x.SECTION.attr)), "realign")
    m.options, m.sink = options, sink
    return m


REALIGN = realign()
