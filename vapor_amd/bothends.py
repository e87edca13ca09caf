"""`--both-ends` (not in the reference): the seven extra columns of a row, from the per-view score lists that
drivers.vapor_both_ends leaves on a locus's score list (drivers.BothEnds.views)."""
from __future__ import annotations

from typing import List, Optional

INFO = (
    ("VaPoR_BE_N", "Integer", "1", "Number of views of the junction that were scored, the primary one included (--both-ends)"),
    ("VaPoR_BE_QS", "Float", "1", "VaPoR_QS of the reads of all scored views (--both-ends)"),
    ("VaPoR_BE_GS", "Float", "1", "VaPoR_GS of the reads of all scored views (--both-ends)"),
    ("VaPoR_BE_GT", "String", "1", "Genotype with the highest likelihood from the reads of all scored views (--both-ends)"),
    ("VaPoR_BE_GQ", "Float", "1", "Genotype quality from the reads of all scored views (--both-ends)"),
    ("VaPoR_BE_Rec", "Float", ".", "Similarity scores of the reads of all scored views, in view order (--both-ends)"),
    ("VaPoR_BE_SQS", "String", ".", "VaPoR_QS of every view of the junction in table order, '.' for a view that was not scored (--both-ends)"),
)
COLUMNS = tuple(i[0] for i in INFO)


class Views(list):
    """A locus's views with `keys` (`--dedup-qname`, DESIGN.md 4.18 rule V): per view the name keys (seqio.name_key) of the reads
    behind its scores, None for a view that was not scored."""
    keys = None


def pool(views, keys=None) -> List[float]:
    """The pooled score list of a locus: the concatenation of the scored views' lists in table order.  With keys (rule V of
    `--dedup-qname`) a score is skipped when its read's key belongs to a read that contributed a score in an earlier scored view."""
    if keys is None:
        return [x for v in views if v is not None for x in v]
    out, seen = [], set()
    for v, ks in zip(views, keys):
        if v is None:
            continue
        mine = set()
        for x, k in zip(v, ks):
            if k not in seen:
                out.append(x)
                mine.add(k)
        seen |= mine
    return out


def pack(views) -> List[float]:
    """A locus's views as one list of floats (they travel between ranks as a second table of "scores"): the number of views,
    per view its number of scores or -1 for a view that was not scored, then all scores; nothing for a locus without views.
    Views with keys (`--dedup-qname`): -1.0 follows, then per score of every scored view its key as two floats, the high and the
    low 32 bits; without keys the record is what it was."""
    if views is None:
        return []
    out = [float(len(views))] + [float(-1 if v is None else len(v)) for v in views]
    for v in views:
        out += [float(x) for x in (v or ())]
    keys = getattr(views, "keys", None)
    if keys is not None:
        out.append(-1.0)
        for v, ks in zip(views, keys):
            if v is not None:
                if len(ks) != len(v):
                    raise ValueError("both-ends: %d keys for %d scores" % (len(ks), len(v)))
                for k in ks:
                    out += [float(int(k) >> 32), float(int(k) & 0xFFFFFFFF)]
    return out


def unpack(flat) -> Optional[list]:
    if flat is None or len(flat) == 0:
        return None
    n = int(flat[0])
    lens = [int(x) for x in flat[1:1 + n]]
    at = 1 + n
    views = []
    for m in lens:
        if m < 0:
            views.append(None)
        else:
            views.append([float(x) for x in flat[at:at + m]])
            at += m
    if at < len(flat):                       # (the views' keys follow)
        if float(flat[at]) != -1.0:
            raise ValueError("both-ends: malformed view record")
        at += 1
        views = Views(views)
        views.keys = []
        for v in views:
            if v is None:
                views.keys.append(None)
                continue
            views.keys.append([(int(flat[at + 2 * i]) << 32) | int(flat[at + 2 * i + 1]) for i in range(len(v))])
            at += 2 * len(v)
    return views


def columns_many(views_list) -> List[List[str]]:
    """The seven fields of every row: '.' seven times for a locus without junction branch; else the number of scored views, the
    row routines (finish.row_tails: result_organize_ins, SF:1219-1231, and gt_estimate_log_likelihood, SF:2054-2069) over the
    concatenation of the scored views' lists in table order (pool: with `--dedup-qname` without the scores of molecules an
    earlier view has counted), and the views' own QS, comma-separated, '.' for a view that was not scored."""
    from .finish import row_tails
    lists, where = [], []
    for views in views_list:
        if views is None:
            where.append(None)
            continue
        where.append((len(lists), len(views)))
        lists.append(pool(views, getattr(views, "keys", None)))
        lists += [list(v) if v is not None else [] for v in views]
    tails = row_tails(lists)
    out = []
    for views, w in zip(views_list, where):
        if w is None:
            out.append(["."] * 7)
            continue
        t = tails[w[0]]
        sqs = [("." if v is None else str(tails[w[0] + 1 + i][0])) for i, v in enumerate(views)]
        out.append([str(sum(1 for v in views if v is not None))] + [str(x) for x in t] + [",".join(sqs)])
    return out
