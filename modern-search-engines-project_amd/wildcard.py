"""Prefix and wildcard query terms, the host's policy (DESIGN K16; the lookup itself is msr_wildcard_terms,
DeviceEngine.wildcard_terms).

A pattern is a query token with `*` (any run of code points, none included) or `?` (exactly one): `bibliothek*`,
`*bibliothek`, `t?bingen`, `uni*thek`.  It is anchored at both ends and matched against the vocabulary AS INDEXED -- with a
lemmatising tokenizer it matches lemmas, not surface forms.  The terms it matches, the most frequent first (document
frequency descending, then term id), at most `limit` of them, join the query as ordinary scoring terms, each with its own
idf, behind the terms that were typed.  A pattern is never a required or an excluded term, never part of a phrase or a
proximity condition, and never corrected by fuzzy=True.  Pure Python: nothing here needs a GPU.
"""
from ._abi import MSR_FUZZY_MAX_LEN, MSR_MAX_QUERY_TERMS, MSR_WILD_MAX_LEN
from .fuzzy import lookable

MIN_LITERALS = 2              # a pattern with fewer literal code points (`*`, `a*`, `??`) is not looked up: it names half the vocabulary
STAR, ANY = "*", "?"
assert MSR_WILD_MAX_LEN == MSR_FUZZY_MAX_LEN


def literals(pattern):
    """The number of literal code points of a pattern (neither `*` nor `?`)."""
    return sum(1 for c in pattern if c != STAR and c != ANY)


def encodable(pattern):
    """True if the device can take the pattern: a string of 1 .. MSR_WILD_MAX_LEN symbols, none above fuzzy.MAX_CODE_POINT
    -- what fuzzy.lookable asks of a word (the two lengths are one constant in the kernels)."""
    return lookable(pattern)


def usable(pattern):
    """True if expand() looks the pattern up: encodable, with at least MIN_LITERALS literal code points."""
    return encodable(pattern) and literals(pattern) >= MIN_LITERALS


def _as_pattern(token):
    """The pattern a whitespace-delimited token stands for, or None: only letters, `*` and `?`; ONE trailing `?` is
    punctuation and goes first (`tübingen?` is a word, `t?bingen?` the pattern `t?bingen`); then at least one `*` or `?`."""
    if not token or not all(c == STAR or c == ANY or c.isalpha() for c in token):
        return None
    if token.endswith(ANY):
        token = token[:-1]
    return token if (STAR in token or ANY in token) else None


def parse_wildcards(processed_query: str):
    """Patterns of a query that has been through preprocess_query -> (scoring_text, patterns).  A whitespace-delimited token
    that consists only of letters, `*` and `?` and, after ONE trailing `?` has been stripped as punctuation, still holds a
    `*` or `?` is a pattern: it is removed from the scoring text and comes back, lower-cased, in `patterns` (in order,
    repeats kept).  A token with a digit, a hyphen or a quote is left as it is; text between a pair of quotes (paired from the
    left, as parse_phrases pairs them) is never looked at, so this runs on the text that still has its quotes -- in front of
    parse_phrases / parse_proximity, which it leaves every quote, and of parse_operators.  `+uni*` / `-uni*` raise ValueError:
    a required or excluded pattern is not supported, and the token would go wrong silently otherwise (the tokenizer drops the
    star).  Without a pattern the text comes back unchanged."""
    at = [i for i, ch in enumerate(processed_query) if ch == '"']
    quoted = list(zip(at[0::2], at[1::2]))                   # [a, b]: an opening quote and its closing quote
    out, patterns, pos, n = [], [], 0, len(processed_query)
    changed = False
    while pos < n:
        if processed_query[pos].isspace():
            out.append(processed_query[pos])
            pos += 1
            continue
        end = pos                                            # the token: up to white space, quoted stretches swallowed whole
        has_quote = False
        while end < n and not processed_query[end].isspace():
            hit = next((b for a, b in quoted if a == end), None)
            if hit is not None:
                has_quote, end = True, hit + 1
            else:
                has_quote |= processed_query[end] == '"'
                end += 1
        tok = processed_query[pos:end]
        pat = None
        if not has_quote:
            if len(tok) >= 2 and tok[0] in "+-" and _as_pattern(tok[1:]) is not None:
                raise ValueError("required and excluded patterns are not supported")
            pat = _as_pattern(tok)
        if pat is None:
            out.append(tok)
        else:
            patterns.append(pat.lower())
            changed = True
        pos = end
    if not changed:
        return processed_query, []
    return " ".join("".join(out).split()), patterns


def expand(lookup, name_of, ids, patterns, limit):
    """The expansion policy for a chunk of queries.  ids: per query its typed term ids; patterns: per query its pattern
    strings (None or empty: none).  lookup(patterns) -> per pattern ([term id, ...] in the lookup's order, at most `limit`
    of them, total) -- called ONCE, with every distinct usable() pattern of the chunk in first-occurrence order, and not at
    all when there is none.  name_of(term id) -> the term string.
    -> (ids, expansions): new id lists in which a query's expansions stand BEHIND its typed ids, in pattern order, then in
    the lookup's order -- an id the query already holds is not added twice, and appending stops when the query holds
    MSR_MAX_QUERY_TERMS unique ids (the engine refuses more; the unknown id -1 is one of them, as DeviceEngine.pack_queries
    counts it) -- and per query {pattern: {"terms": [the term strings that were added or already there, in order], "total":
    all matches}}, with "skipped": True for a pattern that was not looked up (fewer than MIN_LITERALS literal code points,
    or not encodable: "terms" [] and "total" 0) and "truncated": True where the cut at MSR_MAX_QUERY_TERMS left matches
    out.  The inputs are not modified."""
    limit = int(limit)
    Q = len(ids)
    pats = [[str(p).lower() for p in (patterns[q] or ())] if patterns is not None else [] for q in range(Q)]
    ask = list(dict.fromkeys(p for ps in pats for p in ps if usable(p)))
    found = {}
    if ask:
        found = {p: ([int(t) for t in terms][:limit], int(total)) for p, (terms, total) in zip(ask, lookup(ask))}
    new_ids, expansions = [], []
    for q in range(Q):
        row = [int(i) for i in ids[q]]
        have = set(row)
        info = {}
        for p in pats[q]:
            if p in info:
                continue
            if p not in found:
                info[p] = {"terms": [], "total": 0, "skipped": True}
                continue
            terms, total = found[p]
            used, cut = [], False
            for t in terms:
                if t not in have:
                    if len(have) >= MSR_MAX_QUERY_TERMS:
                        cut = True
                        break
                    have.add(t)
                    row.append(t)
                used.append(name_of(t))
            info[p] = {"terms": used, "total": total}
            if cut:
                info[p]["truncated"] = True
        new_ids.append(row)
        expansions.append(info)
    return new_ids, expansions
