"""Shared cases and the plain numpy reference of the document sets built from posting lists (msr_term_sets, DESIGN K11).

    term_set_mask(z, must, must_not, base_mask) -> bool [N]     the conventions of msretr.h, in numpy
    corpus(N) -> TermCorpus                                      a hand-made postings-only CorpusIndex with named edge terms
    row_cases(c) -> [RowCase]                                    rows (must, must_not, base) and the edge each one claims

The corpus sizes straddle a bitset word (32), a skip-table tile (1024) and the kernel's span (S = MSR_TERMSET_SPAN_DOCS); the
corpus of 2 S + 37 documents holds every named term."""
from dataclasses import dataclass, field

import numpy as np

from msretr._abi import MSR_TERMSET_SPAN_DOCS as S
from msretr.index import CorpusIndex

HEAVY_DF = 2048                                              # posting lists at least this long get a skip-table row
SIZES = [1, 31, 32, 33, 1023, 1024, 1025, S - 1, S, S + 1, 2 * S + 37]
BIG = 2 * S + 37


def term_set_mask(z, must, must_not, base_mask=None):
    """bool [N]: base AND every must term's documents AND NOT any must_not term's.  A must term outside [0, n_terms) or with
    an empty list empties the set; such a must_not term is ignored; base_mask None = every document."""
    off, post = np.asarray(z["term_off"], np.int64), np.asarray(z["post_doc"], np.int64)
    V, N = len(off) - 1, int(z["n_docs"])
    out = np.ones(N, bool) if base_mask is None else np.array(base_mask, bool, copy=True)
    for t in must:
        if not 0 <= t < V or off[t] == off[t + 1]:
            return np.zeros(N, bool)
        has = np.zeros(N, bool)
        has[post[off[t]:off[t + 1]]] = True
        out &= has
    for t in must_not:
        if 0 <= t < V:
            out[post[off[t]:off[t + 1]]] = False
    return out


def brute_force(z, must, must_not, base_mask=None):
    """The same with python sets, term by term (the check of the reference itself)."""
    off, post = [int(v) for v in z["term_off"]], [int(v) for v in z["post_doc"]]
    V, N = len(off) - 1, int(z["n_docs"])
    docs = lambda t: set(post[off[t]:off[t + 1]]) if 0 <= t < V else None
    keep = set(range(N)) if base_mask is None else {d for d in range(N) if base_mask[d]}
    for t in must:
        keep &= docs(t) or set()
    for t in must_not:
        keep -= docs(t) or set()
    return keep


@dataclass
class TermCorpus:
    n_docs: int
    ix: CorpusIndex
    z: dict
    term: dict                                               # name -> term id
    docs: dict                                               # name -> int64 array of the term's documents
    bases: list = field(default_factory=list)                # [(name, bool [N])] base rows, in row order


@dataclass
class RowCase:
    must: list
    must_not: list
    base: int                                                # row_base value (-1, a row, or n_base)
    claim: str


def corpus(N, seed=0):
    rng = np.random.default_rng(1000 + N + seed)
    named = [("all", np.arange(N)), ("even", np.arange(0, N, 2)), ("empty", np.zeros(0, np.int64)),
             ("rnd30", np.nonzero(rng.random(N) < 0.3)[0]), ("rnd1", np.nonzero(rng.random(N) < 0.01)[0])]
    for d in (0, 31, 32, 1023, 1024, S - 1, S, N - 1):
        if d < N and f"one_{d}" not in dict(named):
            named.append((f"one_{d}", np.array([d])))
    named.append(("one_last", np.array([N - 1])))
    named.append(("last_word", np.arange(((N - 1) // 32) * 32, N)))      # entirely in the last (partial, if N % 32) word
    if N >= 3 * (HEAVY_DF - 1):
        named.append(("n2047", np.sort(rng.choice(N, HEAVY_DF - 1, replace=False))))
        named.append(("n2048", np.sort(rng.choice(N, HEAVY_DF, replace=False))))
    if N > 2 * S:
        named.append(("skipper", np.array([3, 700, S - 1, 2 * S, 2 * S + 1, N - 1])))     # nothing in the span [S, 2 S)
    off, post = [0], []
    for _, d in named:
        post.append(np.asarray(d, np.int64))
        off.append(off[-1] + len(d))
    post = np.concatenate(post).astype(np.int32)
    V = len(named)
    ix = CorpusIndex(doc_ids=np.arange(N, dtype=np.int64) * 3 + 7, doc_len=np.full(N, 10, np.int32),
                     term_off=np.asarray(off, np.int64), post_doc=post, post_tf=np.ones(len(post), np.int32),
                     idf=np.linspace(0.5, 2.0, V).astype(np.float32), avgdl=10.0, total_docs=N)
    ix.vocab = {name: i for i, (name, _) in enumerate(named)}
    z = {"term_off": np.asarray(off, np.int64), "post_doc": post, "n_docs": N}
    bases = [("base_odd", np.arange(N) % 2 == 1), ("base_last_word", np.arange(N) >= ((N - 1) // 32) * 32),
             ("base_rnd", rng.random(N) < 0.5)]
    return TermCorpus(N, ix, z, dict(ix.vocab), {n: np.asarray(d, np.int64) for n, d in named}, bases)


def row_cases(c):
    """The rows every corpus is asked for; names a corpus lacks (it is too small for them) are left out."""
    t, V, nb = c.term, len(c.term), len(c.bases)
    has = lambda *names: all(n in t for n in names)
    R = []
    add = lambda must, must_not, base, claim: R.append(RowCase([t.get(x, x) if isinstance(x, str) else x for x in must],
                                                               [t.get(x, x) if isinstance(x, str) else x for x in must_not],
                                                               base, claim))
    add([], [], -1, "no lists: every document, bits at or above N zero")
    add(["all"], [], -1, "must of the every-document term (skip-table path when N >= 2048)")
    add([], ["all"], -1, "not of the every-document term: empty row")
    add(["even"], [], -1, "every other document")
    add([], ["even"], -1, "complement of every other document")
    add(["rnd30", "even"], ["rnd1"], -1, "two must terms and a not term")
    add(["empty"], [], -1, "must term with an empty list: empty row")
    add([], ["empty"], -1, "not term with an empty list: ignored")
    add([-1], [], -1, "unknown must id -1: empty row")
    add([V], [], -1, "unknown must id n_terms: empty row")
    add(["even"], [-1, V, -7, V + 1000], -1, "unknown not ids: ignored")
    add(["rnd30"], ["rnd30"], -1, "a term in both lists: empty row")
    add(["rnd30", "rnd30", "even", "rnd30"], ["rnd1", "rnd1"], -1, "repeated terms")
    add(["one_last"], [], -1, "one posting at document N - 1")
    add([], ["one_last"], -1, "not of the one posting at document N - 1")
    add(["last_word"], [], -1, "a list entirely in the last word")
    add([], ["last_word"], -1, "not of a list entirely in the last word")
    add(["rnd1", "all"], [], -1, "a must term that empties most spans, then the every-document term (early exit)")
    add(["empty", "all"], [], -1, "an empty must list in front of the every-document term (early exit)")
    add(["one_0", "all", "even"], [], -1, "one posting at document 0, then long lists")
    for d in (0, 31, 32, 1023, 1024, S - 1, S):
        if has(f"one_{d}"):
            add([f"one_{d}"], [], -1, f"one posting at document {d}")
            add(["all"], [f"one_{d}"], -1, f"not of one posting at document {d}")
    if has("n2047", "n2048"):
        add(["n2047"], [], -1, "2047 postings: binary-search path, below the skip-table threshold")
        add(["n2048"], [], -1, "2048 postings: skip-table path, at the threshold")
        add(["n2047", "n2048"], [], -1, "both sides of the threshold")
        add(["all"], ["n2047", "n2048"], -1, "not lists on both sides of the threshold")
    if has("skipper"):
        add(["skipper"], [], -1, "a list with no posting in a whole span")
        add(["all"], ["skipper"], -1, "not of a list with no posting in a whole span")
    many = [n for n in ("all", "even", "rnd30") if has(n)]
    add([many[i % len(many)] for i in range(70)], [("rnd1", "empty", -1)[i % 3] for i in range(70)], -1,
        "70 must terms and 70 not terms")
    # bases
    add(["rnd30"], [], 0, "base row 0")
    add([], ["rnd30"], 2, "base row 2")
    add(["all"], [], 1, "a base with bits only in the last word")
    add([], [], 1, "base alone, no lists")
    add(["all"], [], nb, "row_base == n_base: empty row")
    add([], [], -2, "row_base below -1: empty row")
    add(["even"], ["rnd1"], -1, "row_base -1 beside restricted rows")
    return [r for r in R if all(isinstance(x, (int, np.integer)) for x in r.must + r.must_not)]


def base_mask(c, r):
    """The mask row_base value r stands for: None = every document."""
    if r == -1:
        return None
    return c.bases[r][1] if 0 <= r < len(c.bases) else np.zeros(c.n_docs, bool)


def random_rows(c, n, seed=5):
    """n rows of mixed operators: lists of 0 .. 4 terms from the corpus and the unknown ids, any base."""
    rng = np.random.default_rng(seed)
    V, nb = len(c.term), len(c.bases)
    pool = list(range(V)) + [-1, V]
    rows = []
    for i in range(n):
        must = [int(pool[j]) for j in rng.integers(0, len(pool), rng.integers(0, 4))]
        if i % 3 == 0:                                       # most random intersections are empty: keep a third non-trivial
            must = [c.term[x] for x in (("all",), ("even",), ("rnd30", "even"), ())[i // 3 % 4]]
        must_not = [int(pool[j]) for j in rng.integers(0, len(pool), rng.integers(0, 5))]
        if i % 3 == 0:
            must_not = [t for t in must_not if t not in (c.term["all"],)]
        rows.append(RowCase(must, must_not, int(rng.integers(-1, nb + 1)), f"random row {i}"))
    return rows
