"""Query-biased snippets (DESIGN K14): the host side of msr_best_windows.

    term_weights(ix, ids) -> [int]          a term's integer weight in a window: its idf in 1/1024ths
    query_row(ix, term_ids) -> [int] | None the row of a query: its distinct known ids, at most MSR_PHRASE_MAX_TERMS
    render(title, text, start, mask, span, spans_fn) -> (snippet, highlights)
                                            a window of token positions -> the passage of the page and where its terms stand

The engine answers WHICH window of a document's indexed token stream is the best one (DeviceEngine.best_windows: the start,
a bit per position of the window that holds a query term, a bit per query term that stands in it); strings never reach the
GPU.  render maps the token positions back to characters by tokenising the page again, lazily, up to the window's end."""
from ._abi import MSR_PHRASE_MAX_TERMS, MSR_PROX_MAX_SPAN, MSR_SNIPPET_MAX_WEIGHT
from .index import _np
from .index_build import normalise_document_text
from .text import simple_tokenize_spans

WEIGHT_SCALE = 1024
SNIPPET_TOKENS = 30                                          # the default window, in tokens of the indexed stream


def _idf_host(ix):
    """The index's idf column on the host (copied once per column: an index built on the device holds a device tensor)."""
    got = getattr(ix, "_idf_host", None)
    if got is None or got[0] is not ix.idf:
        got = ix._idf_host = (ix.idf, _np(ix.idf))
    return got[1]


def term_weights(ix, ids):
    """max(1, min(MSR_SNIPPET_MAX_WEIGHT, round(1024 * max(idf, 0)))) per id: an integer, so that kernel and oracle agree bit
    for bit.  A term with a negative idf (more than half of the pages hold it: the city that preprocess_query appends) gets
    the minimum, 1 -- it still counts as a hit, but never decides a window against any other term."""
    idf = _idf_host(ix)
    return [max(1, min(MSR_SNIPPET_MAX_WEIGHT, round(WEIGHT_SCALE * max(float(idf[int(t)]), 0.0)))) for t in ids]


def query_row(ix, term_ids):
    """The query's distinct known ids (inside [0, n_terms)) in first-occurrence order.  With more than MSR_PHRASE_MAX_TERMS of
    them the heaviest stay (term_weights; of two equal ones the earlier), still in first-occurrence order.  None if nothing
    is left: the query has no row, and its results keep the reference's snippet."""
    n_terms, seen = int(ix.n_terms), []
    for t in term_ids:
        t = int(t)
        if 0 <= t < n_terms and t not in seen:
            seen.append(t)
    if len(seen) > MSR_PHRASE_MAX_TERMS:
        w = term_weights(ix, seen)
        keep = sorted(sorted(range(len(seen)), key=lambda j: (-w[j], j))[:MSR_PHRASE_MAX_TERMS])
        seen = [seen[j] for j in keep]
    return seen or None


def display_text(title, text):
    """-> (normalised string, display string).  The token stream was built from normalise_document_text(title, text), so a
    token's character range is a range of THAT string.  The display string is the raw f"{title or ''} {text or ''}" (cut to
    the same 1 000 000 characters) when the ranges hold for it too: its lower-casing has the same length (lower-casing never
    drops a character, so an equal length means every character kept its place) and it holds no `tuebingen` / `tubingen`
    spelling in any case (the normalisation replaces those by a string of another length).  Otherwise it is the normalised
    string itself: lower-cased, but exact."""
    raw = f"{title or ''} {text or ''}"
    low = raw.lower()
    norm = normalise_document_text(title, text)
    if len(low) == len(raw) and "tuebingen" not in low and "tubingen" not in low:
        return norm, raw[:1_000_000]
    return norm, norm


def render(title, text, start, mask, span, spans_fn=None, context_chars=0):
    """(snippet, highlights) of the window of `span` tokens that starts at token `start` of the page's indexed stream; `mask`
    bit k = token start + k is highlighted (out_start / out_mask of msr_best_windows).  spans_fn(text) yields (term, begin,
    end) per token of the normalised string (default text.simple_tokenize_spans; it must be the index's tokenizer) and is
    consumed only up to the window's end.
    Which string is shown: display_text -- the raw title + " " + text where token ranges hold for it, else the normalised
    string.  The snippet runs from the first window token's begin to the last window token's end (the window is cut at the
    page's last token), widened by up to context_chars characters on either side, stopping at white space so that no word is
    cut; "..." stands in front unless it starts the string and behind unless it ends it.  highlights: one [begin, end) pair
    of offsets INTO THE SNIPPET STRING per set bit of mask, ascending.  ValueError if the page has no token `start` (the text
    is not what the stream was built from) or a set bit lies past the page's last token."""
    start, mask, span = int(start), int(mask), int(span)
    if start < 0 or not 1 <= span <= MSR_PROX_MAX_SPAN or mask < 0 or mask >> span:
        raise ValueError(f"render: start {start}, span {span}, mask {mask:#x}")
    norm, shown = display_text(title, text)
    at = []                                                  # (begin, end) of the window's tokens
    for i, (_, b, e) in enumerate((spans_fn or simple_tokenize_spans)(norm)):
        if i >= start:
            at.append((b, e))
            if len(at) == span:
                break
    if not at:
        raise ValueError(f"render: the page has no token {start}")
    if mask >> len(at):
        raise ValueError(f"render: mask {mask:#x} names a token past the page's last one (the window holds {len(at)})")
    b0, e0 = at[0][0], at[-1][1]
    if context_chars > 0:
        lo, hi = max(0, b0 - int(context_chars)), min(len(shown), e0 + int(context_chars))
        while 0 < lo < b0 and not shown[lo - 1].isspace():   # inward to a word's first character
            lo += 1
        while e0 < hi < len(shown) and not shown[hi].isspace():
            hi -= 1
        b0, e0 = lo, hi
    head = "..." if b0 > 0 else ""
    snippet = head + shown[b0:e0] + ("..." if e0 < len(shown) else "")
    shift = len(head) - b0
    return snippet, [[b + shift, e + shift] for k, (b, e) in enumerate(at) if mask >> k & 1]
