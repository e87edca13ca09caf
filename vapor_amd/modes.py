"""The run modes of `vapor bed | vcf` that append columns to every row: `--refine`, `--phased` (and `--phase-vcf`, the same mode
with another source of tags), `--both-ends`, `--depth`, `--signatures`, `--links`, `--support` and `--realign`.  At most one holds for a run (the parser refuses every pair); None is the plain
run.  A Mode is everything cli.py and the VCF writer need to know about one; what the option computes stays in
its own module - refine.py, phase.py, bothends.py, depth.py, signature.py, links.py, support.py, realign.py - which gives the mode its columns and the way they travel between ranks;
depth.py to support.py also say how their regions are read (their reader surface), and the parser states the rule once (cli.MODE_OPTIONS)."""
from __future__ import annotations

from . import bothends, depth, junction, links, phase, polish, realign, revote, signature, support
from . import junction as _junction            # (realign_revote's `junction` argument hides the module's name)
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
    thread (`--realign-out`: realign.TraceWriter)."""
    chunk_gens = None
    chunk_payloads = None
    sink = None
    polish = False                             # (`--realign-polish`: the Realign requests ask for the consensus too)
    junction = False                           # (`--realign-junction`: ... and for the one jump of the polished allele)
    revote = False                             # (`--realign-revote`: ... and for every read's distance to the polished allele)

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
REALIGN = Mode("realign", realign, "realign")


def realign_out(sink) -> Mode:
    """`--realign --realign-out PREFIX`: REALIGN's columns, with the sink the loci's traces go to."""
    m = Mode("realign", realign, "realign")
    m.sink = sink
    return m


def realign_polish(sink=None) -> Mode:
    """`--realign --realign-polish`: REALIGN's columns followed by polish's six; with `--realign-out` the sink
    the loci's traces and polished alleles go to (polish.PolishWriter)."""
    m = Mode("realign", polish, "realign")
    m.sink = sink
    m.polish = True
    return m


def realign_junction(sink=None) -> Mode:
    """`--realign --realign-polish --realign-junction`: realign_polish's columns followed by junction's six,
    with realign_polish's sink."""
    m = Mode("realign", junction, "realign")
    m.sink = sink
    m.polish = True
    m.junction = True
    return m


def realign_revote(sink=None, junction=False) -> Mode:
    """`--realign --realign-polish --realign-revote`: realign_polish's columns - with `junction`
    (`--realign-junction` as well) realign_junction's - followed by revote's eight, with realign_polish's sink."""
    m = Mode("realign", revote.over(_junction if junction else polish), "realign")
    m.sink = sink
    m.polish = True
    m.junction = bool(junction)
    m.revote = True
    return m
