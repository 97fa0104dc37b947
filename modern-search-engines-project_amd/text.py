"""Host-side text helpers of the query path (strings never reach the GPU).

Mirrors, by behaviour, /root/reference/search_api.py:155-166 (preprocess_query), :168-201
(extract_domain_topic), reranker/reranker_api.py:170-176 (extract_domain), :239-260
(create_sliding_windows) and the batch line format of search_api.py:290.
"""
import re
import threading
from urllib.parse import urlparse

from ._abi import MSR_PHRASE_MAX_TERMS, MSR_PROX_MAX_SPAN

CITY = "tübingen"


def preprocess_query(query: str) -> str:
    """Lower-case, map the ASCII spellings of the city to 'tübingen', append the city when the query does
    not mention it (search_api.py:155-166)."""
    q = query.strip().lower()
    if "tuebingen" in q or "tubingen" in q or CITY in q:
        q = q.replace("tuebingen", CITY).replace("tubingen", CITY)
    else:
        q = f"{q} {CITY}"
    return q.replace("tuebingen", CITY).replace("tubingen", CITY).strip().lower()


def extract_domain(url) -> str:
    try:
        return urlparse(url).netloc.lower()
    except Exception:
        return "defaultdomain"


def extract_domain_topic(url) -> str:
    if not url or url == "#":
        return "unknown"
    try:
        domain = re.sub(r"^www\.", "", urlparse(url).netloc.lower())
        parts = domain.split(".")
        main = (parts[0] if len(parts) == 2 else parts[-2]) if len(parts) >= 2 else domain
        main = re.sub(r"[^a-zA-Z0-9-]", "", main)
        return main if main else "unknown"
    except Exception:
        return "unknown"


def create_sliding_windows(tokens, window_size=512, step_size=450):
    """Token windows used to cut documents into chunks (config.py:10-11; embedder.py:65-87)."""
    if len(tokens) <= window_size:
        return [tokens]
    windows = [tokens[i:i + window_size] for i in range(0, len(tokens) - window_size + 1, step_size)]
    last = len(tokens) - window_size
    if last >= 0 and last % step_size != 0:
        windows.append(tokens[last:last + window_size])
    return windows


_WORD = re.compile(r"[^\W\d_]+", re.UNICODE)


def simple_tokenize(text: str):
    """Stand-in for BM25._tokenize (bm25_indexer.py:149-155).  The reference lemmatises with spaCy
    `en_core_web_sm` and drops stop words; spaCy and its model are not available offline, so this only
    lower-cases and keeps alphabetic tokens.  Pass `tokenizer=` to BM25 / Retriever to plug in the real
    one; with identical term lists the engine's results are identical to the reference's."""
    return [m.group(0).lower() for m in _WORD.finditer(text)]


def simple_tokenize_spans(text: str):
    """simple_tokenize with each token's place: a generator of (term, begin, end), text[begin:end] being the match the term
    came from -- the same matches in the same order, so token i of a document's indexed stream is the i-th item.  Lazy: the
    snippet renderer (snippets.render) stops at its window's end and a long page is never tokenised whole."""
    for m in _WORD.finditer(text):
        yield m.group(0).lower(), m.start(), m.end()


def parse_operators(processed_query: str):
    """Search-box operators of a query that has been through preprocess_query -> (scoring_text, must_words, not_words).
    A whitespace-delimited token that starts with `+` or `-` FOLLOWED BY A LETTER is an operator token: `+word` -- the page
    must contain the word -- keeps the word (without its sign) in the scoring text; `-word` -- the page must not contain
    it -- is removed from the scoring text.  Anything else is left as it is: a sign inside a token (`uni-tuebingen`,
    `c++`), a lone `+` or `-`, a doubled sign (`++a`, `--a`, `+-a`), a sign before a digit (`-123`).  The words come back
    as written (sign stripped); the caller tokenises them like the query -- a word of several tokens requires (or excludes)
    all of them.  Because this runs after preprocess_query, the appended city is a plain scoring term, and `-tuebingen`
    excludes the city's pages instead of scoring them."""
    keep, must, must_not = [], [], []
    for tok in processed_query.split():
        if len(tok) >= 2 and tok[0] in "+-" and tok[1].isalpha():
            if tok[0] == "+":
                must.append(tok[1:])
                keep.append(tok[1:])
            else:
                must_not.append(tok[1:])
        else:
            keep.append(tok)
    return " ".join(keep), must, must_not


def parse_phrases(processed_query: str):
    """Quoted phrases of a query that has been through preprocess_query -> (text_without_quotes, must_phrases, not_phrases),
    the phrases as the text between their quotes.  `"a b c"` -- the page must hold the words next to each other, in this
    order, in its indexed token stream -- keeps its words in the scoring text (a `+` in front of the opening quote means the
    same and is dropped); `-"a b"` -- the page must not hold the phrase -- is removed from the scoring text.  The sign counts
    only at the start of a whitespace-delimited token.  Quotes pair up from the left; an unbalanced last quote is left as it
    is; empty quotes are dropped.  Runs before parse_operators (which sees the text without quotes); the caller tokenises each
    phrase like the query, and a phrase that tokenises to nothing is dropped there.  Without a pair of quotes the text comes
    back unchanged."""
    at = [i for i, ch in enumerate(processed_query) if ch == '"']
    if len(at) < 2:
        return processed_query, [], []
    out, must, must_not, pos = [], [], [], 0
    for a, b in zip(at[0::2], at[1::2]):
        inner = processed_query[a + 1:b].strip()
        sign = processed_query[a - 1] if a >= 1 and processed_query[a - 1] in "+-" and (a == 1 or processed_query[a - 2].isspace()) else ""
        out.append(processed_query[pos:a - len(sign)])
        if sign == "-":
            if inner:
                must_not.append(inner)
        else:
            if inner:
                must.append(inner)
            out.append(" " + inner + " ")
        pos = b + 1
    out.append(processed_query[pos:])
    return " ".join("".join(out).split()), must, must_not


class Near:
    """A proximity condition (DESIGN K13): the terms stand within a window of the page's indexed token stream.  terms: a
    string (tokenised like the query by the facade that takes it), a list of term strings, or at engine level a list of term
    ids.  ordered=False: one occurrence of every distinct term inside a window of (number of distinct terms + slop) tokens,
    in any order -- up to `slop` other tokens among them; ordered=True: the terms in this order, the first and the last at
    most (number of terms + slop) tokens apart -- slop 0 is the exact phrase.  An immutable value; equal conditions compare
    and hash equal.  ValueError: a negative slop; a list of more than MSR_PHRASE_MAX_TERMS terms; a window of more than
    MSR_PROX_MAX_SPAN tokens (both known once the terms are a list: with_terms checks what a string could not)."""
    __slots__ = ("terms", "slop", "ordered")

    def __init__(self, terms, slop=0, ordered=False):
        if isinstance(slop, bool) or int(slop) != slop or slop < 0:
            raise ValueError(f"Near: slop must be a whole number >= 0, got {slop!r}")
        set_ = object.__setattr__
        set_(self, "terms", terms if isinstance(terms, str) else tuple(terms))
        set_(self, "slop", int(slop))
        set_(self, "ordered", bool(ordered))
        if not isinstance(terms, str):
            if len(self.terms) > MSR_PHRASE_MAX_TERMS:
                raise ValueError(f"a proximity condition may hold at most {MSR_PHRASE_MAX_TERMS} terms (MSR_PHRASE_MAX_TERMS), "
                                 f"got {len(self.terms)}")
            if self.span > MSR_PROX_MAX_SPAN:
                raise ValueError(f"a proximity window may span at most {MSR_PROX_MAX_SPAN} tokens (MSR_PROX_MAX_SPAN), got "
                                 f"{self.span} = {self.span - self.slop} terms + slop {self.slop}")

    def __setattr__(self, name, value):
        raise AttributeError("Near is immutable")

    @property
    def span(self):
        """The window in tokens: L + slop when ordered, the number of distinct terms + slop otherwise (terms as a list)."""
        if isinstance(self.terms, str):
            raise ValueError("Near.span: the terms are still a string (tokenise them first: with_terms)")
        return (len(self.terms) if self.ordered else len(set(self.terms))) + self.slop

    def with_terms(self, terms):
        """The same condition over other terms (the tokens of the string, the ids of the terms)."""
        return Near(terms, self.slop, self.ordered)

    def __len__(self):
        return len(self.terms)

    def _key(self):
        return (self.terms, self.slop, self.ordered)

    def __eq__(self, other):
        return isinstance(other, Near) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        terms = self.terms if isinstance(self.terms, str) else list(self.terms)
        return f"Near({terms!r}, slop={self.slop}, ordered={self.ordered})"


_SLOP = re.compile(r"~(>?)(\d+)(?=\s|$)")


def parse_proximity(processed_query: str):
    """parse_phrases with one addition -> (text_without_quotes, must, must_not): a closing quote DIRECTLY followed by `~N` or
    `~>N` (digits only, then whitespace or the end of the text) turns that phrase into a proximity condition, and the suffix
    is removed from the text.  `"a b"~N` -> Near("a b", N, ordered=False): the words within a window, in any order, with up
    to N other tokens among them; `"a b"~>N` -> Near("a b", N, ordered=True): the words in this order, with up to N other
    tokens between the first and the last.  A `~` followed by anything else is left in the text and the phrase stays exact.
    Entries without a suffix come back as plain strings; pairing of the quotes, the sign in front and what stays in the scoring
    text are parse_phrases' (a text without a suffix gives exactly its output).  A slop too wide for the words (Near's
    ValueError) shows once the phrase is tokenised."""
    at = [i for i, ch in enumerate(processed_query) if ch == '"']
    if len(at) < 2:
        return processed_query, [], []
    out, must, must_not, pos = [], [], [], 0
    for a, b in zip(at[0::2], at[1::2]):
        inner = processed_query[a + 1:b].strip()
        sign = processed_query[a - 1] if a >= 1 and processed_query[a - 1] in "+-" and (a == 1 or processed_query[a - 2].isspace()) else ""
        out.append(processed_query[pos:a - len(sign)])
        m = _SLOP.match(processed_query, b + 1)
        entry = Near(inner, int(m.group(2)), ordered=m.group(1) == ">") if m else inner
        if sign == "-":
            if inner:
                must_not.append(entry)
        else:
            if inner:
                must.append(entry)
            out.append(" " + inner + " ")
        pos = m.end() if m else b + 1
    out.append(processed_query[pos:])
    return " ".join("".join(out).split()), must, must_not


def format_result_line(query_num, rank, url, score) -> str:
    """search_api.py:290"""
    return f"{query_num}\t{rank}\t{url}\t{score:.3f}"


def read_queries_file(path):
    """queries.txt: 'query_num<TAB>query_text' per line (search_api.py:214-235)."""
    out = []
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            parts = line.split("\t")
            if len(parts) >= 2:
                out.append((parts[0].strip(), parts[1].strip()))
    return out


class LineFormatter:
    """The batch lines of search_api.py:290 for whole batches: the URLs as one UTF-8 blob + offsets (built once), the
    formatting in native code (msr_format_lines, include/msretr.h: a HOST function, no GPU involved).  Byte for byte what
    "\n".join(format_result_line(...)) + "\n" gives."""

    def __init__(self, urls, n_docs=None):
        import numpy as np
        from . import _abi
        self._lib = _abi.load()
        n = len(urls) if urls is not None else int(n_docs or 0)
        enc = [u.encode("utf-8") if u else b"" for u in urls] if urls is not None else []
        self.blob = b"".join(enc)
        self.off = np.zeros(n + 1, np.int64)
        if enc:
            np.cumsum(np.fromiter((len(b) for b in enc), np.int64, n), out=self.off[1:])
        self.n_docs = n
        self.max_url = int(np.diff(self.off).max()) if n else 0
        self._buf = self._cbuf = None
        self.lock = threading.Lock()

    def format(self, query_nums, doc, score, n):
        """query_nums: list of str; doc int32 [Q, S], score float64 [Q, S], n int32 [Q] (host arrays) -> the lines as a
        bytes-like view of the formatter's own buffer (valid until the next call; bytes(...) for a copy).  A formatter that
        several threads share (a Retriever's, which its BatchLines keep after their request) is called, and its view used,
        under `lock`."""
        import ctypes as C

        import numpy as np
        doc = np.ascontiguousarray(doc, np.int32); score = np.ascontiguousarray(score, np.float64)
        n = np.ascontiguousarray(n, np.int32)
        Q = len(query_nums)
        assert doc.shape == score.shape and doc.ndim == 2 and doc.shape[0] == Q and n.shape == (Q,)
        qb = [str(x).encode("utf-8") for x in query_nums]
        qblob = b"".join(qb)
        qoff = np.zeros(Q + 1, np.int64)
        if Q:
            np.cumsum(np.fromiter((len(b) for b in qb), np.int64, Q), out=qoff[1:])
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        args = (C.c_char_p(qblob), ptr(qoff), Q, ptr(doc), ptr(score), ptr(n), int(doc.shape[1]), C.c_char_p(self.blob),
                ptr(self.off), self.n_docs, max(1, self.max_url))
        need = -int(self._lib.msr_format_lines(*args, None, 0))
        if need <= 0:
            return memoryview(b"")
        if self._buf is None or len(self._buf) < need:         # one output buffer per formatter, grown when needed (a fresh
            self._buf = bytearray(need + need // 4)             # bytearray of several MB costs more than filling it)
            self._cbuf = (C.c_char * len(self._buf)).from_buffer(self._buf)
        got = int(self._lib.msr_format_lines(*args, self._cbuf, len(self._buf)))
        if got < 0:
            raise RuntimeError(f"msr_format_lines failed ({got})")
        return memoryview(self._buf)[:got]
