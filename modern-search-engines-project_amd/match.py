"""Match modes (DESIGN K19): results that hold ALL of a query's words, or at least m of them.

    need("75%", 4)                                         # -> 3: how many of 4 slots a page must fill
    groups = slots(ix, ids, expansions)                    # a query's slots: its words, a pattern's expansions as ONE slot
    sets = match_sets(engine, [groups], [3], within=...)   # DeviceSets, for every consumer of term_sets' rows
    retriever.search(query, match="all")                   # the chain does the three for every query of a chunk

A slot is a list of term ids and is filled by a page that holds any of them; a page matches when it fills at least `need` of
the query's slots, inside within= and inside what operators, phrases and proximity built.  The counting is msr_match_sets
(include/msretr_match.h): one launch per call.  Everything but match_sets is pure Python: nothing else here needs a GPU.
"""
import ctypes as C
import re

import numpy as np

from ._abi import MSR_MATCH_MAX_GROUPS

_PERCENT = re.compile(r"^(-?)(\d{1,3})%$")
_OFF = ("any", None)


def check_value(value):
    """ValueError unless `value` is a match value: "any" / None (off), "all", an int other than 0 (m; -m: all but m), or a
    percentage string "p%" / "-p%" with p in 1 .. 100 ("75%": three quarters, rounded down; "-25%": all but a quarter, rounded
    down).  A bool, 0, "0%", a float and any other string are refused."""
    if value is None or (isinstance(value, str) and value in ("any", "all")):
        return
    if isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_)) and int(value) != 0:
        return
    if isinstance(value, str):
        m = _PERCENT.match(value)
        if m and 1 <= int(m.group(2)) <= 100:
            return
    raise ValueError(f'match must be "any", "all", a whole number other than 0 or a percentage like "75%" / "-25%" '
                     f"(got {value!r})")


def is_on(value):
    """True unless the (checked) value is "any" or None."""
    return not (value is None or (isinstance(value, str) and value == "any"))


def need(value, n_slots):
    """How many of a query's n_slots slots a page must fill -> None (matching is off: "any" / None, or a query without
    slots), else an int in [1, n_slots].  "all": G; m > 0: m; -m: G - m; "p%": floor(p G / 100); "-p%": G - floor(p G / 100);
    every result clamped to [1, G] -- never below 1, never above the number of slots, Lucene's minimum_should_match rule.
    Anything else raises ValueError (check_value)."""
    check_value(value)
    G = int(n_slots)
    if not is_on(value) or G <= 0:
        return None
    if isinstance(value, str):
        if value == "all":
            m = G
        else:
            sign, p = _PERCENT.match(value).groups()
            part = int(p) * G // 100
            m = G - part if sign else part
    else:
        m = int(value) if int(value) > 0 else G + int(value)
    return max(1, min(G, m))


def slots(ix, ids, expansions=None):
    """A query's slots -> a list of groups, each a list of term ids.  ids: the query's typed term ids after fuzzy correction
    (CorpusIndex.term_ids: an unknown word is an id < 0), before any expansion was appended; expansions: None, or per pattern
    the list of term ids it was expanded to.
      - every distinct id of [0, n_terms) is one slot, first occurrence first;
      - every occurrence of an id the vocabulary lacks is a slot of its own, [-1]: it fills nothing, so match="all" on a query
        with an unknown word returns nothing, as `+word` does (fuzzy=True runs before this and may have replaced the word);
      - each pattern's expansions are ONE slot, behind the words, in pattern order (a pattern that expanded to nothing is an
        empty slot that no page fills);
      - words with idf <= 0 are left out, with the fallback of facets.counting_terms: if every known word would be left out,
        all are kept.  The city term that text.preprocess_query appends to every query is such a word: the user did not type
        it, requiring it would be wrong and would stream the longest list of the index.  A TYPED `tübingen` is therefore not
        required either -- the two cannot be told apart once the query is preprocessed."""
    n_terms, idf = int(ix.n_terms), ix.idf
    seen, valid, unknown = set(), [], 0
    for t in ids:
        t = int(t)
        if 0 <= t < n_terms:
            if t not in seen:
                seen.add(t)
                valid.append(t)
        else:
            unknown += 1
    positive = [t for t in valid if float(idf[t]) > 0]
    groups = [[t] for t in (positive or valid)] + [[-1] for _ in range(unknown)]
    for terms in expansions or ():
        groups.append(list(dict.fromkeys(int(t) for t in terms)))
    return groups


def slot_names(groups, name_of, unknown_words=()):
    """The slots as term strings, for a result's `.match`: name_of(term id) -> the term; the [-1] slots take the words of
    unknown_words in order (None where there is none left)."""
    words = iter(unknown_words)
    return [[next(words, None)] if g == [-1] else [name_of(t) for t in g] for g in groups]


def _row_groups(groups, df, n_terms):
    """A row's groups as the value that two queries with the same slots share, in the order the kernel reads them: ids the
    index lacks or whose list is empty are dropped from their group (the group stays), each group's ids sorted, the groups
    ordered by summed document frequency, shortest first (then by their ids) -- the short lists decide early which spans
    can still match."""
    clean = []
    for g in groups:
        ids = sorted({int(t) for t in g if 0 <= int(t) < n_terms and df[int(t)] > 0})
        clean.append((int(sum(int(df[t]) for t in ids)), tuple(ids)))
    clean.sort()
    return tuple(ids for _, ids in clean)


def match_sets(engine, groups, need, within=None):
    """Per-query document sets of match modes, built on the device (msr_match_sets): query q's set is the documents of
    within[q] that fill at least need[q] of the slots groups[q] (slots(); need(): None = matching is off for that query).
    within: None, a DocSet (every query), a list of DocSet / None per query, or a DeviceSets (Conditions.sets: what operators,
    phrases and proximity built) -- its rows become the base rows.  -> DeviceSets, tied to the engine's index, for every
    consumer of term_sets' result (bm25_topk / dense_topk / dense_topk_grouped / facet_counts / the Retriever's chain).
    Queries with equal (slots as sets of ids, need, base) share one row -- compared on the host, never on bits.  A query with
    matching off gets its base's row, or -1, and costs no kernel row; a call in which no query matches makes no launch.  A
    row of more than MSR_MATCH_MAX_GROUPS slots raises ValueError.  ONE upload (a blocking copy on the caller's stream) and
    ONE launch, under the engine's request lock; nothing is read back -- but a DeviceSets base keeps its row numbers on the
    device, and they come back first (4 bytes per query, a wait for the stream)."""
    import torch
    from . import _abi
    from .docset import DeviceSets, DocSet, pack_within
    with engine.lock:
        ix = engine.index
        if ix.term_off is None or ix.n_terms <= 0:
            raise _abi.MsrError(-2, "match_sets: the index has no postings")
        groups, need = list(groups), list(need)
        Q = len(groups)
        if len(need) != Q:
            raise ValueError(f"match_sets: {Q} slot lists and {len(need)} needs")
        for q in range(Q):
            if need[q] is not None and len(groups[q]) > MSR_MATCH_MAX_GROUPS:
                raise ValueError(f"match_sets: a query may hold at most MSR_MATCH_MAX_GROUPS = {MSR_MATCH_MAX_GROUPS} slots "
                                 f"(query {q} has {len(groups[q])})")
        stride = max(1, (ix.n_docs + 31) // 32)
        base_bits, n_base, base_of = None, 0, [-1] * Q
        if isinstance(within, DeviceSets):
            within.check(ix)
            if len(within) != Q:
                raise ValueError(f"within: {len(within)} entries for {Q} queries")
            if within.stride != stride:
                raise ValueError(f"within: rows of {within.stride} words, {stride} expected")
            base_bits, n_base = within.bits, int(within.n_sets)
            base_of = [int(v) for v in within.q_set.cpu().tolist()]
        elif isinstance(within, DocSet):
            base_bits, _, n_base, _ = engine.pack_within(within, Q)
            base_of = [0] * Q
        elif within is not None:
            words, base_q, n_base, _ = pack_within(within, Q, ix)
            base_of = base_q.tolist()
            if n_base:
                base_bits = torch.from_numpy(words.view(np.int32)).to(engine.device)
        if not n_base:
            base_of = [-1] * Q
        df, n_terms = engine._doc_freq(), int(ix.n_terms)
        rows, row_of, q_row, keep_base = [], {}, [], False
        for q in range(Q):
            if need[q] is None or int(need[q]) <= 0:
                q_row.append(None)
                keep_base = keep_base or base_of[q] != -1
                continue
            ordered = _row_groups(groups[q], df, n_terms)
            key = (ordered, int(need[q]), base_of[q])
            r = row_of.get(key)
            if r is None:
                r = row_of[key] = len(rows)
                rows.append((ordered, int(need[q]), base_of[q]))
            q_row.append(r)
        first = n_base if keep_base else 0                   # base rows that queries without matching still name come first
        q_set = [(base_of[q] if keep_base else -1) if r is None else first + r for q, r in enumerate(q_row)]
        bits = torch.empty((first + len(rows), stride), dtype=torch.int32, device=engine.device)
        if first:
            bits[:first] = base_bits[:first]
        if rows:
            R = len(rows)
            g_off, t_off, terms = [0], [0], []
            for ordered, _, _ in rows:
                for g in ordered:
                    terms.extend(g)
                    t_off.append(len(terms))
                g_off.append(len(t_off) - 1)
            host = np.asarray(g_off + t_off + [m for _, m, _ in rows] + [b for _, _, b in rows] + terms, np.int32)
            dev = torch.from_numpy(host).to(engine.device)
            a, b = R + 1, R + 1 + len(t_off)
            p_goff, p_toff, p_need, p_base, p_terms = dev[:a], dev[a:b], dev[b:b + R], dev[b + R:b + 2 * R], dev[b + 2 * R:]
            null = C.c_void_p(0)
            ptr = lambda t: C.c_void_p(t.data_ptr())
            engine._check(engine.lib.msr_match_sets(engine.handle, R, ptr(p_goff), ptr(p_toff), ptr(p_terms) if terms else null,
                                                    ptr(p_need), ptr(base_bits) if n_base else null, n_base, stride,
                                                    ptr(p_base) if n_base else null, ptr(bits[first:]), stride, engine._stream()))
        return DeviceSets(ix, bits, torch.tensor(q_set, dtype=torch.int32, device=engine.device), first + len(rows), stride)
