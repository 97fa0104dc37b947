"""Plain-loop oracle of the prefix and wildcard lookup (msr_wildcard_terms, DESIGN K16), the hand-made cases and the
random-case generator its tests share.  Nothing here filters or takes a shortcut for heads and tails: glob_match() fills the
whole table, expected() tries every pattern on every term."""
import numpy as np

from fuzzy_ref import image, pack_words  # noqa: F401  (the vocabulary image and the packing are K15's)

MAX_LEN = 32                                                 # MSR_WILD_MAX_LEN


def glob_match(p, t):
    """True if pattern p matches the WHOLE of t: `*` any run of zero or more code points, `?` exactly one, anything else
    itself; no escape.  The full (len(p) + 1) x (len(t) + 1) table: m[i][j] = p[:i] matches t[:j]."""
    n, L = len(p), len(t)
    m = [[False] * (L + 1) for _ in range(n + 1)]
    m[0][0] = True
    for i in range(1, n + 1):
        for j in range(L + 1):
            if p[i - 1] == "*":
                m[i][j] = m[i - 1][j] or (j > 0 and m[i][j - 1])
            elif j > 0:
                m[i][j] = m[i - 1][j - 1] and (p[i - 1] == "?" or p[i - 1] == t[j - 1])
    return m[n][L]


def expected(vocab, weights, patterns, limit):
    """-> (out_term [P][limit], out_n [P], out_total [P]) as the header defines them.  vocab: the term strings by term id;
    weights: one int per term.  A term of weight 0 or of more than MAX_LEN code points is no match; a pattern of 0 or of more
    than MAX_LEN symbols has an empty row.  Order: weight descending, then term id."""
    terms, ns, totals = [], [], []
    for p in patterns:
        cand = []
        if 1 <= len(p) <= MAX_LEN:
            for t, (s, wt) in enumerate(zip(vocab, weights)):
                if wt > 0 and len(s) <= MAX_LEN and glob_match(p, s):
                    cand.append((-int(wt), t))
        cand.sort()
        first = cand[:limit]
        terms.append([c[1] for c in first] + [-1] * (limit - len(first)))
        ns.append(len(first))
        totals.append(len(cand))
    return (np.asarray(terms, np.int32).reshape(len(patterns), limit), np.asarray(ns, np.int32), np.asarray(totals, np.int32))


# ------------------------------------------------------------------------------------------------ known answers
# (pattern, {term: matches})
KNOWN = [
    ("a*a", {"a": False, "aa": True, "aba": True, "ab": False, "abaa": True}),
    ("*ab*ab", {"abab": True, "ababab": True, "aab": False, "ab": False, "xabyab": True, "abxaby": False}),
    ("a*ba", {"aba": True, "abba": True, "ababa": True, "ab": False, "ba": False, "abab": False}),
    ("??", {"a": False, "ab": True, "abc": False, "": False}),
    ("?*", {"": False, "a": True, "abc": True}),
    ("*?", {"": False, "a": True, "abc": True}),
    ("*", {"": True, "a": True, "abc": True}),
    ("**", {"": True, "a": True, "abc": True}),
    ("a**b", {"ab": True, "axb": True, "a": False, "b": False, "abx": False}),
    ("t?bingen", {"tübingen": True, "tubingen": True, "tbingen": False, "tuebingen": False}),
    ("mensa", {"mensa": True, "mensas": False, "mens": False, "amensa": False}),
    ("*a*", {"a": True, "xax": True, "xx": False, "": False}),
    ("a*b*c", {"abc": True, "aXbYc": True, "acb": False, "abcb": False, "abcbc": True}),
    ("*?a", {"a": False, "ba": True, "bba": True, "ab": False}),
    ("a?*", {"a": False, "ab": True, "abc": True, "ba": False}),
]


# ------------------------------------------------------------------------------------------------ the hand vocabulary
def hand():
    """-> (vocab, weights, patterns): the terms and patterns the issue of K16 lists.  Term ids are positions in vocab."""
    long31, long32, long33 = "a" * 30 + "b", "a" * 31 + "b", "a" * 32 + "b"
    vocab = [
        "a", "ab", long31, long32, long33,                   # lengths 1, 2, 31, 32, 33 (the last: never a match)
        "geist",                                             # weight 0, the only term "geist" / "gei?t" could match
        "x\ufffey", "x\ufffe",                               # code point 0xFFFE, reached through `?`
        "tübingen", "tubingen", "bär", "bar",                # umlaut and ASCII twins with different weights
        "haus", "maus", "laus", "raus",                      # tied on weight: the id decides
        "aa", "aba", "abab", "ababab", "aab", "abba", "ababa", "abc", "b", "ba", "xax",
        "mensa", "mensen", "universität", "universitätsbibliothek", "stadtbibliothek", "bibliothek", "bibliotheken",
        "a*b", "wer?",                                       # terms that hold the metacharacters themselves
    ]
    weights = [5, 7, 3, 4, 9,
               0,
               2, 2,
               50, 9, 6, 6,
               8, 8, 8, 8,
               1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
               40, 12, 30, 3, 4, 20, 2,
               1, 1]
    assert len(vocab) == len(weights)
    patterns = [p for p, _ in KNOWN] + [
        "geist", "gei?t", "x?y", "x?", "?aus", "*aus", "b?r", "bibliothek*", "*bibliothek", "uni*thek", "*bib*", "a?b", "wer?",
        "a",                                                 # 1 symbol
        "a" * 30 + "?",                                      # 31 symbols
        "a" * 31 + "?", "*" * 31 + "b", "?" * 32,            # 32 symbols
        "a" * 32 + "*", "*" * 33,                            # 33 symbols: an empty row
        "",                                                  # 0 symbols: an empty row
        "a*", "*b", "ab*ab", "*a*b*", "?*?", "a" * 29 + "*b",
    ]
    return vocab, weights, patterns


# ------------------------------------------------------------------------------------------------ the random case
ALPHABET = "abcä"


def random_case(seed=5, n_terms=3000, n_patterns=64):
    """-> (vocab, weights, patterns): distinct terms over ALPHABET of 1 .. 8 code points with random weights (zeros, repeats
    and 2^31 - 1 among them); the patterns are terms with runs replaced by `*` and characters by `?`, plus random patterns."""
    rng = np.random.default_rng(seed)
    seen, vocab = set(), []
    while len(vocab) < n_terms:
        s = "".join(ALPHABET[i] for i in rng.integers(0, 4, int(rng.integers(1, 9))))
        if s not in seen:
            seen.add(s)
            vocab.append(s)
    weights = [int(v) for v in rng.choice([0, 0, 1, 1, 2, 3, 3, 7, 7, 100, 2 ** 31 - 1], n_terms)]
    patterns = []
    for i in range(n_patterns):
        kind = i % 4
        if kind < 3:                                         # a term with 1 .. 3 runs starred and some characters questioned
            s = list(vocab[int(rng.integers(0, n_terms))])
            for _ in range(1 + kind):
                a = int(rng.integers(0, len(s) + 1))
                b = min(len(s), a + int(rng.integers(0, 3)))
                s[a:b] = ["*"]
            s = ["?" if c != "*" and rng.random() < 0.2 else c for c in s]
            patterns.append("".join(s))
        else:                                                # anything over the alphabet and the metacharacters
            patterns.append("".join((ALPHABET + "*?*")[j] for j in rng.integers(0, 7, int(rng.integers(1, 7)))))
    return vocab, weights, patterns
