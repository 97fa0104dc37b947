"""Plain-loop oracle of the typo-tolerant lookup (msr_fuzzy_terms, DESIGN K15), the hand-made cases and the random-case
generator its tests share.  Nothing here filters or bands: osa() fills the whole matrix, expected() compares every word with
every term."""
import numpy as np

MAX_LEN = 32                                                 # MSR_FUZZY_MAX_LEN


def osa(a, b):
    """Optimal string alignment distance of two strings over code points: insertion, deletion, substitution and a swap of two
    adjacent code points cost 1 each; no substring is edited twice.  The full (len(a) + 1) x (len(b) + 1) matrix."""
    n, m = len(a), len(b)
    d = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        d[i][0] = i
    for j in range(m + 1):
        d[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            best = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                best = min(best, d[i - 2][j - 2] + 1)
            d[i][j] = best
    return d[n][m]


def expected(vocab, weights, words, maxes, limit):
    """-> (out_term [W][limit], out_dist [W][limit], out_n [W], out_total [W]) as the header defines them.  vocab: the term
    strings by term id; weights: one int per term.  A term of weight 0 or of more than MAX_LEN code points is no candidate; a
    word of length 0 or of more than MAX_LEN code points, or a tolerance outside {0, 1, 2}, has an empty row."""
    terms, dists, ns, totals = [], [], [], []
    for w, m in zip(words, maxes):
        cand = []
        if 1 <= len(w) <= MAX_LEN and m in (0, 1, 2):
            for t, (s, wt) in enumerate(zip(vocab, weights)):
                if wt > 0 and len(s) <= MAX_LEN:
                    d = osa(w, s)
                    if d <= m:
                        cand.append((d, -int(wt), t))
        cand.sort()
        first = cand[:limit]
        terms.append([c[2] for c in first] + [-1] * (limit - len(first)))
        dists.append([c[0] for c in first] + [-1] * (limit - len(first)))
        ns.append(len(first))
        totals.append(len(cand))
    return (np.asarray(terms, np.int32).reshape(len(words), limit), np.asarray(dists, np.int32).reshape(len(words), limit),
            np.asarray(ns, np.int32), np.asarray(totals, np.int32))


def image(vocab, weights):
    """(char_off int64, chars uint16, weight uint32) of a list of term strings, as they are (nothing excluded)."""
    off = np.zeros(len(vocab) + 1, np.int64)
    np.cumsum([len(s) for s in vocab], out=off[1:])
    chars = np.asarray([ord(c) for s in vocab for c in s], np.uint16)
    return off, chars, np.asarray(weights, np.uint32)


def pack_words(words):
    """(word_off int32, word_chars uint16) of a list of words."""
    off = np.zeros(len(words) + 1, np.int32)
    np.cumsum([len(w) for w in words], out=off[1:])
    return off, np.asarray([ord(c) for w in words for c in w], np.uint16)


# ------------------------------------------------------------------------------------------------ known answers
KNOWN = [
    ("ca", "abc", 3), ("ab", "ba", 1), ("tubingen", "tübingen", 1),
    ("", "", 0), ("", "abc", 3), ("ab", "", 2),
    ("mensa", "mensa", 0),
    ("amensa", "maensa", 1),            # a swap at the first position
    ("mensa", "mensa"[:3] + "as", 1),   # ... and at the last
    ("mensa", "emnsax", 2),             # swap plus insert
    ("bär", "bar", 1), ("a", "ä", 1),
    ("abcdef", "badcfe", 3), ("kitten", "sitting", 3),
]


# ------------------------------------------------------------------------------------------------ the hand vocabulary
def hand():
    """-> (vocab, weights, words): the terms and words the issue of K15 lists.  Term ids are positions in vocab."""
    long31, long32, long33 = "a" * 30 + "b", "a" * 31 + "b", "a" * 32 + "b"
    vocab = [
        "a", "ab", long31, long32, long33,                   # lengths 1, 2, 31, 32, 33 (the last: weight 0 below)
        "geist",                                             # weight 0, equal to a query word
        "x\ufffey", "x\ufffe",                               # code point 0xFFFE
        "tübingen", "tubingen", "bär", "bar",                # umlaut and ASCII twins
        "mensa", "menso", "mense", "mansa", "mesna",         # tied on distance from "mensb" / "mensa", different weights
        "haus", "maus", "laus", "raus",                      # tied on distance AND weight from "kaus": the id decides
        "b", "ba", "abc", "geis", "geister",
    ]
    weights = [5, 7, 3, 4, 0,
               0,
               2, 2,
               50, 9, 6, 6,
               40, 10, 30, 20, 1,
               8, 8, 8, 8,
               1, 2, 3, 4, 5]
    words = ["a", "b", "ab", "ba", "abd", "mensb", "mensa", "kaus", "geist", "tubingen", "bar", "x\ufffe", "xy",
             long32, long33, "a" * 32, "a" * 31, "", "zzzzzz"]
    assert len(vocab) == len(weights)
    return vocab, weights, words


# ------------------------------------------------------------------------------------------------ the random case
ALPHABET = "abcä"


def random_case(seed=7, n_terms=3000, n_words=64):
    """-> (vocab, weights, words, maxes): distinct terms over ALPHABET of 1 .. 8 code points with random weights (zeros and
    repeats among them); the words are terms, edited terms and random strings, tolerances 0 .. 2."""
    rng = np.random.default_rng(seed)
    seen, vocab = set(), []
    while len(vocab) < n_terms:
        s = "".join(ALPHABET[i] for i in rng.integers(0, 4, int(rng.integers(1, 9))))
        if s not in seen:
            seen.add(s)
            vocab.append(s)
    weights = [int(v) for v in rng.choice([0, 0, 1, 1, 2, 3, 3, 7, 7, 100, 2 ** 31 - 1], n_terms)]
    words, maxes = [], []
    for i in range(n_words):
        kind = i % 4
        if kind == 0:                                        # a long term, edited once: few candidates
            s = list(vocab[int(rng.integers(0, n_terms))] + "abäc")
            s[int(rng.integers(0, len(s)))] = "c"
            words.append("".join(s)[:8]); maxes.append(1 + i // 4 % 2)
        elif kind == 1:                                      # a short word: many candidates
            words.append("".join(ALPHABET[j] for j in rng.integers(0, 4, int(rng.integers(1, 5))))); maxes.append(2)
        elif kind == 2:                                      # nothing near: longer than every term
            words.append("".join(ALPHABET[j] for j in rng.integers(0, 4, 11 + i % 3))); maxes.append(i % 3)
        else:                                                # a term itself, tolerance 0 or 1
            words.append(vocab[int(rng.integers(0, n_terms))]); maxes.append(i // 4 % 2)
    return vocab, weights, words, maxes
