"""Vectorised oracles and case generators for the two vocabulary lookups at the edges their first tests leave out (DESIGN K15,
K16; csrc/msr_vocabscan.h): long terms with an edit at every position, a wide alphabet with a signature collision, heads and
tails of every length, and a vocabulary of 258 spans that drives the merge through several rounds.  No GPU here.

osa_all / glob_all fill the same full tables as fuzzy_ref.osa / wildcard_ref.glob_match -- no band, no filter, no head or tail
shortcut -- for ONE word or pattern against every term at once: the term axis (and a row's columns) are numpy axes, the rows
stay a Python loop.  test_vocabscan_cases.py holds them against the plain loops and asserts what the generators promise."""
import numpy as np

from fuzzy_ref import MAX_LEN, osa

SPAN, WAVE, MG_CAP = 1024, 64, 2048                          # MSR_FUZZY_SPAN_TERMS, a wavefront, msr_vocabscan.h's MG_CAP


# ------------------------------------------------------------------------------------------------ the oracles
def sig_bit(c):
    """The bit of the 64-bit character-set signature code point c sets (msr_vocabscan.h sig_bit, restated)."""
    return ((c * 0x9E3779B1) & 0xFFFFFFFF) >> 26


def signature(s):
    v = 0
    for c in s:
        v |= 1 << sig_bit(ord(c))
    return v


def pack(terms):
    """-> (codes uint16 [width][T], column t the code points of term t, 0xFFFF behind its end; lens int64 [T]); width: the
    longest term present (at least 1).  The term axis is the contiguous one: a row of a table is a few long vector operations."""
    lens = np.fromiter(map(len, terms), np.int64, len(terms))
    width = max(int(lens.max(initial=0)), 1)
    codes = np.full((len(terms), width), 0xFFFF, np.uint16)
    codes[np.arange(width)[None, :] < lens[:, None]] = np.frombuffer("".join(terms).encode("utf-16-le"), np.uint16)
    return np.ascontiguousarray(codes.T), lens


def osa_all(word, terms):
    """fuzzy_ref.osa(word, t) for every t of terms (a list, or its pack()) -> int64 [T].  Row i of the full table for all terms
    and all columns at once (d[j][t]); the insertion, which runs along the row, is a running minimum of d - j."""
    codes, lens = terms if isinstance(terms, tuple) else pack(terms)
    width, T = codes.shape
    a = [ord(c) for c in word]
    J = np.arange(width + 1, dtype=np.int8)[:, None]
    prev2, prev = None, np.broadcast_to(J, (width + 1, T)).copy()
    for i in range(1, len(a) + 1):
        x = np.empty((width + 1, T), np.int8)                # the cell without the insertion
        x[0] = i
        np.minimum(prev[1:] + 1, prev[:-1] + (codes != a[i - 1]), out=x[1:])
        if i > 1 and width > 1:                              # a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1], j >= 2
            swap = (codes[:-1] == a[i - 1]) & (codes[1:] == a[i - 2])
            np.minimum(x[2:], prev2[:-2] + 1, out=x[2:], where=swap)
        x -= J
        np.minimum.accumulate(x, axis=0, out=x)
        x += J
        prev2, prev = prev, x
    return prev[lens, np.arange(T)].astype(np.int64)


def glob_all(pattern, terms):
    """wildcard_ref.glob_match(pattern, t) for every t of terms (a list, or its pack()) -> bool [T].  Row i of the full table
    for all terms and all columns at once (m[j][t]); a star's row is a running OR."""
    codes, lens = terms if isinstance(terms, tuple) else pack(terms)
    width, T = codes.shape
    m = np.zeros((width + 1, T), bool)
    m[0] = True
    for c in pattern:
        if c == "*":
            m = np.logical_or.accumulate(m, axis=0)
        else:
            cur = np.zeros_like(m)
            cur[1:] = m[:-1] if c == "?" else m[:-1] & (codes == ord(c))
            m = cur
    return m[lens, np.arange(T)]


def _live(packed, weights):
    w = np.asarray(weights, np.int64)
    return w, (w > 0) & (packed[1] <= MAX_LEN)


def fuzzy_candidates(vocab, weights, words, maxes, packed=None):
    """Per word ALL its candidates in the lookup's order -> list of int64 [n][3] (distance, weight, term id): fuzzy_ref.expected
    without the cut."""
    packed = pack(vocab) if packed is None else packed
    w, live = _live(packed, weights)
    out, dist = [], {}
    for word, m in zip(words, maxes):
        if 1 <= len(word) <= MAX_LEN and m in (0, 1, 2):
            if word not in dist:                             # (a word asked at several tolerances: one table)
                dist[word] = osa_all(word, packed)
            d = dist[word]
            idx = np.flatnonzero(live & (d <= m))
            idx = idx[np.lexsort((idx, -w[idx], d[idx]))]
            out.append(np.stack([d[idx], w[idx], idx], axis=1))
        else:
            out.append(np.zeros((0, 3), np.int64))
    return out


def wild_candidates(vocab, weights, patterns, packed=None):
    """Per pattern ALL its matches in the lookup's order -> list of int64 [n][2] (weight, term id)."""
    packed = pack(vocab) if packed is None else packed
    w, live = _live(packed, weights)
    out = []
    for p in patterns:
        if 1 <= len(p) <= MAX_LEN:
            idx = np.flatnonzero(live & glob_all(p, packed))
            idx = idx[np.lexsort((idx, -w[idx]))]
            out.append(np.stack([w[idx], idx], axis=1))
        else:
            out.append(np.zeros((0, 2), np.int64))
    return out


def cut(cands, limit, with_dist):
    """The lookups' outputs of candidate lists: (out_term, out_dist, out_n, out_total) or, without distances, (out_term, out_n,
    out_total), as fuzzy_ref.expected / wildcard_ref.expected give them."""
    n = len(cands)
    term, dist = np.full((n, limit), -1, np.int32), np.full((n, limit), -1, np.int32)
    for i, c in enumerate(cands):
        k = min(limit, len(c))
        term[i, :k] = c[:k, -1]
        if with_dist:
            dist[i, :k] = c[:k, 0]
    total = np.asarray([len(c) for c in cands], np.int32).reshape(n)
    cnt = np.minimum(total, limit).astype(np.int32)
    return (term, dist, cnt, total) if with_dist else (term, cnt, total)


def rounds_of(limit, n_spans):
    """The merge's rounds at this limit: [(first span, one behind the last)], as merge_rows cuts them."""
    per = (MG_CAP - limit) // limit
    return [(s0, min(s0 + per, n_spans)) for s0 in range(0, n_spans, per)]


# ------------------------------------------------------------------------------------------------ the alphabet
def _alphabet():
    """Letters with pairwise different signature bits, the required ones first, and one more that shares its bit with the
    first: -> (base letters, new letters, (A, B) with sig_bit equal, A a base letter, B in neither list)."""
    must = "äöüß\ufffe\u8001"
    more = "abcdefghijklmnopqrstuvwxyzéèàçñåøæœþðšžčřěůłćńśźđγδλπσφψω"
    seen, letters = set(), []
    for c in must + more:
        if sig_bit(ord(c)) not in seen:
            seen.add(sig_bit(ord(c)))
            letters.append(c)
    assert all(c in letters for c in must) and len(letters) >= 40, (len(letters), letters)
    a = letters[0]
    b = next(chr(c) for c in range(0x8002, 0xFFFE) if not 0xD800 <= c <= 0xDFFF and sig_bit(c) == sig_bit(ord(a)))
    return "".join(letters[:36]), "".join(letters[36:40]), (a, b)


BASE_LETTERS, NEW_LETTERS, COLLIDE = _alphabet()
ALPHABET = BASE_LETTERS + NEW_LETTERS + COLLIDE[1]
BASE_LENGTHS = (1, 2, 3, 15, 16, 17, 29, 30, 31, 32)
SINGLE_KINDS = ("sub", "sub_collide", "del", "ins", "swap")


# ------------------------------------------------------------------------------------------------ fuzzy: edit families
def edit_families(seed=15, variants=3):
    """-> dict(vocab, weights, words, maxes, meta, bases).  Per base string (three per length of BASE_LENGTHS, letters all
    different, COLLIDE[0] among them from length 2 up) and per position its seven edits stand side by side -- substitution by
    a new letter, deletion, double insertion, substitution by the colliding letter, insertion, double deletion, swap -- so
    every 64-term wave of a family holds the lengths n - 2 .. n + 2; then sampled double edits (distance 2) and triple edits
    (distance 3: never found).  meta[t] = (family, n, kind, position, distance by construction or None).  Results of 33 and 34
    code points are terms like the others.  The words: every base at tolerance 0, 1 and 2, and edited strings at tolerance 2 (one of them at 1 too)."""
    rng = np.random.default_rng(seed)
    A, B = COLLIDE
    X1, X2, X3, _ = NEW_LETTERS
    vocab, meta, bases, words, maxes = [], [], [], [], []

    def add(s, *m):
        vocab.append(s)
        meta.append(m)

    for v in range(variants):
        for n in BASE_LENGTHS:
            b = [BASE_LETTERS[i] for i in rng.permutation(len(BASE_LETTERS))[:n]]
            if A not in b and (n >= 2 or v == 0):
                b[int(rng.integers(0, n))] = A
            if v and n >= 2 and "\ufffe" not in b:          # 0xFFFE in the last slot (variant 1) or the first (variant 2)
                p = n - 1 if v == 1 else 0
                b[p if b[p] != A else (p + 1) % n] = "\ufffe"
            b = "".join(b)
            assert len(set(b)) == n
            f = len(bases)
            bases.append(b)
            add(b, f, n, "base", 0, 0)
            for p in range(n + 1):
                if p < n:
                    add(b[:p] + X1 + b[p + 1:], f, n, "sub", p, 1)
                    add(b[:p] + b[p + 1:], f, n, "del", p, 1)
                add(b[:p] + X1 + X2 + b[p:], f, n, "insins", p, 2)
                if p < n:
                    add(b[:p] + B + b[p + 1:], f, n, "sub_collide", p, 1)
                add(b[:p] + X2 + b[p:], f, n, "ins", p, 1)
                if p + 1 < n:
                    add(b[:p] + b[p + 2:], f, n, "deldel", p, 2)
                    add(b[:p] + b[p + 1] + b[p] + b[p + 2:], f, n, "swap", p, 1)
            spots = sorted({p for p in (0, 1, n // 2 - 1, n // 2, n - 4, n - 3) if 0 <= p and p + 3 < n})
            for p in spots:                                  # double edits: the second one two or three slots on
                q = p + 2 + (p & 1)
                add(b[:p] + b[p + 1] + b[p] + b[p + 2:q] + X1 + b[q + 1:], f, n, "swap+sub", p, 2)
                add(b[:p] + X1 + b[p + 1:q] + X2 + b[q + 1:], f, n, "sub+sub", p, 2)
                add(b[:p] + X1 + b[p + 1:q] + B + b[q + 1:], f, n, "sub+collide", p, 2)
            add(X1 + b[:-1], f, n, "ins0+del_end", 0, 2 if n >= 2 else None)
            if n >= 3:                                       # triple edits
                add(X1 + b[1:n // 2] + X2 + b[n // 2 + 1:-1] + X3, f, n, "sub3", 0, 3)
                add(b[1:-1] + X1 + X2, f, n, "del0+sub_end+ins", 0, 3 if n >= 4 else None)
            if n >= 5:
                add(b[1] + b[0] + X1 + b[3:-1] + X2, f, n, "swap+sub+sub", 0, 3)
            if n + 3 <= 34:
                add(X1 + X2 + b + X3, f, n, "ins3", 0, 3)
            add(b, f, n, "dead", 0, None)                    # the base once more, weight 0
            words += [b, b, b]
            maxes += [0, 1, 2]
            edited = [b[:-1] + X1,                                           # the last slot
                      (b[:1] + b[2] + b[1] + b[3:]) if n >= 3 else b + X2,   # a swap across the first register pair
                      (X2 + b) if n < MAX_LEN else b[1:],                    # an insertion in front (32 out of 31)
                      (b[:n - 3] + b[n - 2] + b[n - 3] + b[n - 1:]) if n >= 15 else b[:n // 2] + B + b[n // 2 + 1:]]
            words += edited + edited[:1]                     # ... and one of them at tolerance 1: a short row
            maxes += [2] * len(edited) + [1]
    weights = [0 if m[2] == "dead" else int(w) for m, w in zip(meta, rng.choice([1, 1, 2, 2, 2, 3, 5], len(vocab)))]
    return dict(vocab=vocab, weights=weights, words=words, maxes=maxes, meta=meta, bases=bases)


# ------------------------------------------------------------------------------------------------ wildcard: long cases
def _questioned(pattern, slot):
    """pattern with its slot-th symbol that is not a star replaced by `?`."""
    at = [i for i, c in enumerate(pattern) if c != "*"][slot]
    return pattern[:at] + "?" + pattern[at + 1:]


def wild_long_cases(seed=16):
    """-> dict(vocab, weights, patterns, kinds): kinds[i] = (kind, term length, head length, tail length) of patterns[i]
    ('general' and 'plain' patterns: lengths 0).  Terms of 1 .. 32 code points over ALPHABET (and one of 33): three long terms
    of 32, 31 and 30 different letters, each with every single-letter variant, every prefix and every suffix; runs of a, b, c
    that force the general matcher to go back; short random terms."""
    rng = np.random.default_rng(seed)
    X1 = NEW_LETTERS[0]
    longs = ["".join(BASE_LETTERS[i] for i in rng.permutation(len(BASE_LETTERS))[:n]) for n in (32, 31, 30)]
    runs = ["aab" * 10, "aab" * 10 + "a", "ab" * 16, "a" * 31 + "b", "ab" * 15 + "b", "abc" * 10 + "ab", "ba" * 15 + "c",
            "a" * 15 + "b" + "a" * 15 + "c", "abab" * 7 + "abc", "b" + "ab" * 15, "aab" * 9 + "abb" + "b", "c" + "ab" * 14 + "bc",
            "ab" * 14 + "cab", "a" * 30, "a" * 32, "abcabcab", "abab", "aab", "ab", "b", "a"]
    vocab = list(longs)
    for t in longs:
        vocab += [t[:p] + X1 + t[p + 1:] for p in range(len(t))]
    vocab += [longs[0][:n] for n in range(1, 32)] + [longs[0][32 - n:] for n in range(1, 32)]
    vocab += runs + [longs[0] + X1]
    while len(vocab) < 640:
        vocab.append("".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), int(rng.integers(1, 9)))))
    order = rng.permutation(len(vocab))
    vocab = [vocab[i] for i in order]
    weights = [int(w) for w in rng.choice([0, 1, 1, 2, 2, 3, 7], len(vocab))]
    for t in longs + runs:                                   # the terms the patterns are made for are live
        weights[vocab.index(t)] = max(weights[vocab.index(t)], 1)

    patterns, kinds = [], []

    def add(p, *k):
        patterns.append(p)
        kinds.append(k)

    for t in longs:
        L = len(t)
        for h in range(L + 1):
            add(t[:h] + "*", "head", L, h, 0)
            add("*" + t[L - h:], "tail", L, 0, h)
            for s in range(h):                               # one `?` in every slot of every head and tail
                add(_questioned(t[:h] + "*", s), "head?", L, h, 0)
                add(_questioned("*" + t[L - h:], s), "tail?", L, 0, h)
            for both in (L - 1, L, L + 1):
                tl = both - h
                if 0 <= tl <= L:
                    p = t[:h] + "*" + t[L - tl:]
                    add(p, "both", L, h, tl)
                    # ... and in the combined ones: beside the star, in the middle, at the far ends -- as h runs, every slot
                    at = {L - 1: (h - 1, h), L: (h // 2, h + tl // 2), L + 1: (0, both - 1)}[both]
                    if h:
                        add(_questioned(p, at[0]), "both?", L, h, tl)
                    if tl:
                        add(_questioned(p, at[1]), "both?", L, h, tl)
    t = longs[0]
    add(t, "plain", 32, 32, 0)
    add("?" * 32, "plain", 32, 32, 0)
    add(t[:31] + X1, "plain", 32, 32, 0)
    for s in range(32):
        add(_questioned(t, s), "plain", 32, 32, 0)
    general = ["*ab*ab*b", "a*?b*?c", "*a**b*", "*aab*aab*ab", "aab*aba*b", "a?b*b?a*?ab", "?a*ba*ab*a?", "?a*ba*ab*?b", "*ab?*c",
               "*a?b*?c", "a*b?a*bc", "*b*b*b*b*b*b*b*b*b*b*b", "*b*b*b*b*b*b*b*b*b*b", "a*a*a*a*a*a*a*a*a*a*a*a*a*a*a*a*",
               "*a*a*a*a*a*a*a*a*a*a*a*a*a*a*a*b", "*a?a?a?a*b", "*?b?b*?c", "ab*ba*ab", "*abc*abc*abc*ab", "*abc*cab*", "*ba*c",
               "?ab*ab?*b", "?b*ab*b?", "a*ab*ab*ab*ab*ab*ab*ab*ab*ab*aa", "*ab*ab*ab*ab*ab*ab*ab*ab*ab*ab*b", "*?*?*?*",
               "*" + "?" * 30 + "*", "*" + "?" * 31, "?" * 15 + "*" + "?" * 16, "?" * 15 + "*b*" + "?" * 14, "*c*b*", "*cab",
               "*b*a*c", "a*" + "a" * 15 + "*c", "a*b*" + "a" * 14 + "?c", "*" + "a" * 16 + "*" + "a" * 14, "*a*" + "a" * 29]
    for p in general:
        add(p, "general", 0, 0, 0)
    for t in runs[:13]:                                      # a head, a middle cut from further right, a tail; `?` in each
        L = len(t)
        for h, a, b, tl in ((3, 9, 14, 4), (1, 20, 26, 3), (0, 12, 15, 0), (5, 5, 9, 6), (4, L - 9, L - 4, 4), (2, L - 6, L - 2, 5),
                            (7, 3, 8, 2)):
            p = t[:h] + "*" + t[a:b] + "*" + t[L - tl:]
            add(p, "general", 0, 0, 0)
            add(_questioned(p, h + 1), "general", 0, 0, 0)
            if h:
                add(_questioned(_questioned(p, h - 1), len(p) - 3), "general", 0, 0, 0)
    return dict(vocab=vocab, weights=weights, patterns=patterns, kinds=kinds, longs=longs)


# ------------------------------------------------------------------------------------------------ both: many spans
N_SPANS_TERMS = 257 * SPAN + 1                               # 258 spans, the last of one term
ROW_WORDS = {"first": "mensaqul", "middle": "neckarfb", "last": "schlogit", "each": "tubingkz", "better_later": "wilhemsj",
             "worse_later": "jakobusp", "dense": "hfrdeckl", "one_257": "gasometr", "one_256": "lustnauv", "none": "zzzzzzzz"}
X_SPANS = (2, 3, 4, 126, 127, 128) + tuple(range(200, 210)) + (253, 254, 255, 256)


def _near(word, rng):
    """Neighbours of `word` that keep its first two letters -> (distance 1 strings, distance 2 strings), by the plain oracle."""
    pool, n = "abcdefghijklmnopqrstuvw", len(word)
    one = set()
    for p in range(2, n):
        one.update(word[:p] + c + word[p + 1:] for c in pool[:8])
        one.add(word[:p] + word[p + 1:])
        one.add(word[:p] + pool[p] + word[p:])
        if p + 1 < n:
            one.add(word[:p] + word[p + 1] + word[p] + word[p + 2:])
    one = sorted(s for s in one if len(s) <= 8)
    two = set()
    for s in one[::3]:
        for p in range(2, len(s)):
            two.add(s[:p] + pool[(p + 9) % len(pool)] + s[p + 1:])
    d1 = [s for s in one if osa(word, s) == 1]
    d2 = sorted(s for s in two if osa(word, s) == 2)
    return [d1[i] for i in rng.permutation(len(d1))], [d2[i] for i in rng.permutation(len(d2))]


def many_spans(seed=17):
    """-> dict(vocab, weights, words, maxes, patterns, tags): a vocabulary of 258 spans, every term live and at most 8 code
    points -- digit strings, behind an `x` in the spans X_SPANS -- with the neighbours of ROW_WORDS planted so that one call
    holds every kind of row of the merge (tags[i] names the kind of word i and of pattern i; the patterns behind the tagged
    ones have tag None).  A row's pattern is its word's first two letters and a star: it matches what was planted for the word."""
    rng = np.random.default_rng(seed)
    V = N_SPANS_TERMS
    xs = set(X_SPANS)
    vocab = [("x%06d" if (t >> 10) in xs else "%06d") % t for t in range(V)]
    weights = rng.choice(np.asarray([1, 1, 2, 2, 3]), V).tolist()
    taken = set()

    def plant(span, s, w):
        while True:
            t = span * SPAN + int(rng.integers(0, min(SPAN, V - span * SPAN)))
            if t not in taken:
                break
        taken.add(t)
        vocab[t], weights[t] = s, w

    near = {k: _near(w, rng) for k, w in ROW_WORDS.items()}
    for tag, spans in (("first", (0, 5, 126)), ("middle", (127, 190, 253)), ("last", (254, 255, 256))):
        d1, d2 = near[tag]
        for i, s in enumerate(spans):
            plant(s, d1[i], 2 + i)
            plant(s, d2[i], 1 + i)
        plant(spans[1], ROW_WORDS[tag], 1)
    d1, d2 = near["each"]                                    # eight per round, the keys of the rounds interleaved
    for i in range(24):
        plant((10 + i, 130 + i, 254 + i % 3)[i % 3], (d1 + d2)[i], 1 + (i * 5) % 4)
    d1, d2 = near["better_later"]
    for i in range(20):
        plant(1 + i, d2[i], 1)
    for i in range(10):
        plant(140 + i, d1[i], 5)
    for s in (254, 255, 256):
        plant(s, ROW_WORDS["better_later"], 9)
    d1, d2 = near["worse_later"]
    for i in range(20):
        plant(1 + i, d1[i], 5 + i % 2)
    for i in range(10):
        plant(140 + i, d2[i], 2)
    for s in (254, 255, 256):
        plant(s, d2[10 + s % 3], 1)
    d1, d2 = near["dense"]
    both = d1 + d2
    for s in list(range(0, 132)) + list(range(250, 257)):    # 18 in each of 139 spans
        for i in range(18):
            plant(s, both[int(rng.integers(0, len(both)))], int(rng.integers(1, 5)))
    taken.add(V - 1)
    vocab[V - 1], weights[V - 1] = near["one_257"][0][0], 3  # the only term of span 257
    plant(256, near["one_256"][1][0], 2)
    tags = list(ROW_WORDS)
    words = [ROW_WORDS[k] for k in tags] + [ROW_WORDS["dense"]]
    maxes = [2] * len(tags) + [1]
    patterns = [ROW_WORDS[k][:2] + "*" for k in tags] + ["x*", "*", "x*7", "??????", "*9?", "hf*k?"]
    return dict(vocab=vocab, weights=weights, words=words, maxes=maxes, patterns=patterns,
                tags=tags + [None] * (len(patterns) - len(tags)))
