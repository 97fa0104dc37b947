"""Candidate lists and corpora for the rerank kernels.

TEST INFRASTRUCTURE ONLY, CPU, deterministic from a seed (numpy).

Fuse cases hand the fuse kernel what the gather would have produced -- cand_doc [M], cand_bm25 [M], cand_n,
cos [M, 10] float32, meta [M, 3] = (rows, url group + 2, first row) -- at the places a fuse goes wrong: exact ties inside a
document (dyadic cosines with cmin = 0, cmax = 1 and smoothing 0, so blend = cosine exactly), clamps of the positional
weight, degenerate min-max, the sort's power-of-two edges, URL groups, repeated slots of one document with different BM25
scores, many exactly equal final scores.  `wrong_fuse` restates the fuse with one deliberate mistake each; test_rerank_exact.py
shows every mistake changes the output of at least one case, so a kernel compared with `==` on these cases cannot make it.

The gather corpus holds documents of 0, 1, 2, 9, 10, 11 and 300 rows, a zero row, rows of norm 1e-3 and 1e3,
near-duplicate rows, and uses the corpus' first and last rows; `gather_bar` is the error bound of the gather's f32
arithmetic (derivation in tests/test_gpu_rerank.py).
"""
import json
import os

import numpy as np

from oracle import rerank_ref

DIM = 768
M = 1024                                   # candidate slots per query in every case (the fuse kernel's largest list)
MAXC = rerank_ref.MAX_CHUNKS_PER_DOC       # 10 cosine slots per candidate
U32 = 2.0 ** -24                           # f32 unit roundoff
U64 = 2.0 ** -53
DEFAULT_PRM = (0.15, rerank_ref.MAX_BOOST, rerank_ref.MAX_DECAY)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _empty(n=0, prm=DEFAULT_PRM, name=""):
    return dict(name=name, doc=np.full(M, -1, np.int32), bm=np.zeros(M), n=int(n), cos=np.zeros((M, MAXC), np.float32),
                meta=np.zeros((M, 3), np.int32), prm=tuple(prm))


def _put(c, m, doc, bm, cos, group=None, first=None):
    """slot m <- document `doc` with BM25 `bm` and the cosines `cos` (its rows); group defaults to the document."""
    cos = np.asarray(cos, np.float32)
    c["doc"][m], c["bm"][m] = doc, bm
    c["cos"][m] = 0.0
    c["cos"][m, :len(cos)] = cos
    c["meta"][m] = (len(cos), (doc if group is None else group) + 2, doc * 16 if first is None else first)


def _garbage(c, rng):
    """junk in the slots past cand_n: the fuse kernel must not read them."""
    n = max(0, min(c["n"], M))
    k = M - n
    if k:
        c["doc"][n:] = rng.integers(-5, 1 << 30, k)
        c["bm"][n:] = rng.standard_normal(k) * 1e6
        c["cos"][n:] = np.float32(np.nan)
        c["meta"][n:] = rng.integers(-3, 1 << 20, (k, 3))
        c["meta"][n:, 0] = rng.integers(0, MAXC + 1, k)


# ------------------------------------------------------------------ the reference's own cosines
def fixture_cases():
    """tests/golden/rerank_chain.json: per executed case the kept documents (stage 0 rows, ordered (doc, chunk)), their BM25
    score (first occurrence in doc_ids), the reference's f32 cosines and its stages."""
    with open(os.path.join(GOLDEN, "rerank_chain.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    out = []
    for c in cases:
        s0 = c["stages"][0]
        docs, n_rows = [], []
        for d in s0["doc_id"]:
            if docs and docs[-1] == d:
                n_rows[-1] += 1
            else:
                docs.append(d)
                n_rows.append(1)
        old_of = {}
        for d, s in zip(c["doc_ids"], c["similarities"]):
            old_of.setdefault(int(d), float(s))
        out.append(dict(case=c["case"], docs=docs, n_rows=n_rows, bm25=[old_of[d] for d in docs], cos=s0["new_similarity"],
                        chunk_id=s0["chunk_id"], stages=c["stages"]))
    return out


def fixture_fuse_case(f, seed=0):
    """A fixture as the fuse kernel's input: the kept documents in shuffled slots, each its own URL group, first row = the
    index of its first row in stage 0 (so the winning chunk maps back through f['chunk_id'])."""
    rng = np.random.default_rng(seed)
    c = _empty(len(f["docs"]), name=f"fixture{f['case']}")
    off = np.concatenate([[0], np.cumsum(f["n_rows"])])
    for m, i in enumerate(rng.permutation(len(f["docs"]))):
        _put(c, m, f["docs"][i], f["bm25"][i], np.float32(f["cos"][off[i]:off[i + 1]]), first=int(off[i]))
    _garbage(c, rng)
    return c


# ------------------------------------------------------------------ adversarial fuse cases
def random_case(rng, n, name, prm=DEFAULT_PRM, n_pool=None, group_size=3, p_dup=0.05, p_no_rows=0.03, p_no_url=0.03,
                rows=(1, MAXC), bm_scale=30.0, cand_n=None):
    """n filled slots: documents drawn from a pool (so some repeat), URL groups of up to `group_size` documents interleaved
    across the slots, some groups without urlsDB row (-1), some documents without chunk rows; a repeated document keeps its
    rows, cosines and group but gets a different BM25 score in every slot."""
    n_pool = n_pool or max(4, 3 * n)
    pool = rng.choice(1 << 20, n_pool, replace=False)
    per = {}
    for d in pool:
        r = 0 if rng.random() < p_no_rows else int(rng.integers(rows[0], rows[1] + 1))
        g = -1 if rng.random() < p_no_url else int(rng.integers(0, max(1, n_pool // group_size))) if group_size > 1 else int(d)
        per[int(d)] = (rng.uniform(-1, 1, r).astype(np.float32), g, int(rng.integers(0, 1 << 24)))
    c = _empty(n if cand_n is None else cand_n, prm, name)
    picked = []
    for m in range(n):
        d = int(picked[rng.integers(len(picked))]) if picked and rng.random() < p_dup else int(rng.choice(pool))
        picked.append(d)
        cs, g, first = per[d]
        _put(c, m, d, float(rng.standard_normal() * bm_scale), cs, group=g, first=first)
    _garbage(c, rng)
    return c


def dyadic_tie_cases():
    """cmin = 0, cmax = 1, smoothing 0, equal BM25: blend = cosine exactly, every value dyadic."""
    prm = (0.0, rerank_ref.MAX_BOOST, rerank_ref.MAX_DECAY)
    out = []
    c = _empty(0, prm, "dyadic_equal_maxima")
    rows = [[0.0, 1.0],                                   # the anchors: cmin, cmax
            [0.5, 0.5, 0.5],                              # equal maxima everywhere
            [0.25, 0.75, 0.5, 0.75, 0.75],                # equal maxima at 1, 3, 4
            [0.125, 0.375, 0.375],                        # equal maxima at the end
            [0.625] * MAXC,                               # ten equal rows
            [0.0, 0.0, 0.03125],                          # best row last: 0.03125 - 0.05 clamps to 0.0 = ties row 0
            [0.0, 0.0, 0.0, 0.0, 0.046875],
            [1.0, 1.0],                                   # boost clamped at 1.0, ties the second row
            [0.96875, 1.0, 0.96875],                      # boost of a middle maximum clamped at 1.0
            [0.9375, 0.9375, 0.9375, 0.9375]]
    for i, r in enumerate(rows):
        _put(c, i, 7 + 3 * i, 1.0, r)
    c["n"] = len(rows)
    out.append(c)
    # the same documents in reversed slots, plus single-row documents that tie the others' final scores
    c2 = _empty(0, prm, "dyadic_ties_reversed")
    k = 0
    for i, r in reversed(list(enumerate(rows))):
        _put(c2, k, 7 + 3 * i, 1.0, r)
        k += 1
    for j, v in enumerate([0.5, 0.75, 0.375, 0.0, 1.0, 0.6]):
        _put(c2, k, 1000 - j, 1.0, [v])
        k += 1
    c2["n"] = k
    out.append(c2)
    return out


def degenerate_cases(rng):
    out = []
    c = _empty(0, name="all_cos_equal")                   # cmax == cmin: new = 0
    for m in range(200):
        _put(c, m, 3 * m + 1, float(rng.standard_normal()), np.full(int(rng.integers(1, 11)), 0.25, np.float32))
    c["n"] = 200
    out.append(c)
    c = _empty(0, name="all_bm25_equal")                  # bmax == bmin: old = 0
    for m in range(200):
        _put(c, m, 3 * m + 1, 4.5, rng.uniform(-1, 1, int(rng.integers(1, 11))))
    c["n"] = 200
    out.append(c)
    c = _empty(0, name="both_equal")
    for m in range(200):
        _put(c, m, 1000 - m, 4.5, np.full(int(rng.integers(1, 11)), -0.5, np.float32))
    c["n"] = 200
    out.append(c)
    c = _empty(0, name="one_kept")                        # one document; its URL group's others and rowless docs around
    _put(c, 0, 50, 2.0, [0.1, 0.7, 0.3])
    _put(c, 1, 51, 9.0, [0.9], group=50)
    _put(c, 2, 52, 1.0, [])
    _put(c, 3, 53, 3.0, [0.2], group=-1)
    c["n"] = 4
    out.append(c)
    c = _empty(0, name="none_kept")                       # n = 0, rows = 0, outputs -1 / -inf
    _put(c, 0, 5, 1.0, [])
    _put(c, 1, 6, 1.0, [0.5], group=-1)
    _put(c, 2, -1, 1.0, [0.5])
    _put(c, 3, 8, 1.0, [0.5], group=7)                    # the group's minimum, 7, has no rows: drops the group
    _put(c, 4, 7, 1.0, [])
    c["n"] = 5
    out.append(c)
    out.append(_empty(0, name="cand_n_zero"))
    return out


def url_group_cases(rng):
    out = []
    c = _empty(0, name="groups_random_slots")             # 60 groups of 1 .. 6 documents, slots shuffled
    slots, d = [], 100
    for g in range(60):
        for _ in range(int(rng.integers(1, 7))):
            slots.append((d, g * 1000 + 17))
            d += int(rng.integers(1, 4))
    for m, i in enumerate(rng.permutation(len(slots))):
        doc, g = slots[i]
        _put(c, m, doc, float(rng.standard_normal()), rng.uniform(-1, 1, int(rng.integers(1, 11))), group=g)
    c["n"] = len(slots)
    out.append(c)
    c = _empty(0, name="group_min_without_rows")          # the minimum of a group has 0 rows: the whole group goes
    k = 0
    for g in range(40):
        base = 10 * g
        _put(c, k, base + 5, float(rng.standard_normal()), rng.uniform(-1, 1, 3), group=g); k += 1
        _put(c, k, base + 1, float(rng.standard_normal()), [] if g % 2 else rng.uniform(-1, 1, 2), group=g); k += 1
        _put(c, k, base + 3, float(rng.standard_normal()) * 50, rng.uniform(-1, 1, 4), group=g); k += 1
    c["n"] = k
    out.append(c)
    c = _empty(0, name="url_group_minus_one")             # group -1 (meta[1] = 1) and a raw 0 (nobody owns it)
    for m in range(300):
        _put(c, m, m, float(rng.standard_normal()), rng.uniform(-1, 1, int(rng.integers(1, 11))), group=-1 if m % 3 == 0 else m)
        if m % 7 == 0:
            c["meta"][m, 1] = 0
    c["n"] = 300
    out.append(c)
    # the URL duplicates hold the extreme cosines and BM25 scores: a min-max that includes them changes every score
    c = _empty(0, name="duplicates_hold_extremes")
    for g in range(50):
        _put(c, 2 * g, 10 * g + 1, float(rng.uniform(0, 1)), rng.uniform(-0.5, 0.5, 4), group=g)
        _put(c, 2 * g + 1, 10 * g + 2, 5.0 if g == 7 else float(rng.uniform(0, 1)), [0.9, -0.9] if g == 3 else [0.1], group=g)
    c["n"] = 100
    out.append(c)
    return out


def duplicate_slot_cases(rng):
    """Repeated slots of one document with different BM25 scores: the first slot counts (msretr.h).  The repeats sit at
    slots all over the list, so an unstable sort by (group, doc) puts a later one first for some documents."""
    out = []
    for t in range(3):
        c = _empty(0, name=f"duplicate_slots_{t}")
        docs = rng.choice(1 << 16, 150, replace=False)
        rows = {int(d): rng.uniform(-1, 1, int(rng.integers(1, 11))) for d in docs}
        seq = [int(d) for d in docs] + [int(d) for d in rng.choice(docs, 850)]
        rng.shuffle(seq)
        for m, d in enumerate(seq):
            _put(c, m, d, float(rng.standard_normal() * 10), rows[d])
        c["n"] = len(seq)
        out.append(c)
    return out


def equal_final_scores_case(rng):
    """1024 documents, 1022 of them with the same single cosine and BM25: equal final scores, ascending document order."""
    c = _empty(M, name="equal_final_scores")
    docs = rng.choice(1 << 20, M, replace=False)
    _put(c, 0, int(docs[0]), 0.0, [0.0])
    _put(c, 1, int(docs[1]), 1.0, [1.0])
    for m in range(2, M):
        _put(c, m, int(docs[m]), 0.5, [0.375])
    perm = rng.permutation(M)
    for k in ("doc", "bm", "cos", "meta"):
        c[k] = c[k][perm]
    return c


def param_cases(rng):
    out = []
    for s in (0.0, 0.3, 1.0):
        out.append(random_case(rng, 400, f"smoothing_{s}", prm=(s, 0.1, 0.05)))
    for b, d in ((0.0, 0.0), (0.5, 0.25), (0.2, 1.5), (1.0, 0.0)):
        out.append(random_case(rng, 400, f"boost_{b}_decay_{d}", prm=(0.15, b, d)))
    out.append(random_case(rng, 400, "bm25_negative", bm_scale=1.0))
    out[-1]["bm"][:400] = -np.abs(out[-1]["bm"][:400]) - 7.0
    out.append(random_case(rng, 400, "bm25_huge", bm_scale=1e150))
    for r in range(1, MAXC + 1):
        out.append(random_case(rng, 300, f"rows_{r}", rows=(r, r), p_no_rows=0.0))
    return out


def size_cases(rng):
    out = [random_case(rng, n, f"n_{n}") for n in (1, 63, 64, 65, 511, 512, 513, 1000, 1024)]
    out.append(random_case(rng, M, "cand_n_above_M", cand_n=5000))
    out.append(random_case(rng, 700, "cand_n_negative", cand_n=-3))
    return out


def fuse_cases(seed=11):
    rng = np.random.default_rng(seed)
    cases = [fixture_fuse_case(f, seed=i) for i, f in enumerate(fixture_cases())]
    cases += dyadic_tie_cases() + degenerate_cases(rng) + url_group_cases(rng) + duplicate_slot_cases(rng)
    cases += [equal_final_scores_case(rng)] + param_cases(rng) + size_cases(rng)
    return cases


# ------------------------------------------------------------------ restated fuses, each with one mistake
BUGS = ("last_max_pre", "last_max_post", "ties_by_slot", "ties_desc_doc", "minmax_best_row", "minmax_with_dups",
        "ratio_max_chunks", "bm25_last_dup")


def wrong_fuse(c, bug=None):
    """The fuse restated independently of rerank_ref.fuse_from_gather, with the mistake `bug` (None: none) -> the same
    six outputs."""
    s, boost, decay = c["prm"]
    doc, bm, cos, meta = c["doc"], c["bm"], c["cos"], c["meta"]
    n = max(0, min(int(c["n"]), M))
    valid = [m for m in range(n) if doc[m] >= 0 and meta[m, 1] >= 2]
    win = {}
    for m in valid:
        g, w = int(meta[m, 1]), win.get(int(meta[m, 1]))
        if w is None or doc[m] < doc[w] or (bug == "bm25_last_dup" and doc[m] == doc[w]):
            win[g] = m
    kept = sorted((m for m in win.values() if meta[m, 0] > 0), key=lambda m: int(doc[m]))
    rows = {m: [float(x) for x in cos[m, :meta[m, 0]]] for m in kept}
    pool = [x for m in kept for x in rows[m]]
    bpool = [float(bm[m]) for m in kept]
    if bug == "minmax_best_row":
        pool = [max(rows[m]) for m in kept]
    if bug == "minmax_with_dups":
        for m in valid:
            if m not in kept and meta[m, 0] > 0:
                pool += [float(x) for x in cos[m, :meta[m, 0]]]
                bpool.append(float(bm[m]))
    out_doc = np.full(M, -1, np.int32); out_score = np.full(M, -np.inf); out_orig = np.zeros(M); out_chunk = np.full(M, -1, np.int32)
    if not kept:
        return out_doc, out_score, out_orig, out_chunk, 0, 0
    cmin, cmax, bmin, bmax = min(pool), max(pool), min(bpool), max(bpool)
    first = lambda v: max(range(len(v)), key=lambda i: (v[i], -i))
    last = lambda v: max(range(len(v)), key=lambda i: (v[i], i))
    res = []
    for m in kept:
        old = 0.0 if bmax == bmin else (float(bm[m]) - bmin) / (bmax - bmin)
        v = [(0.0 if cmax == cmin else (x - cmin) / (cmax - cmin)) * (1 - s) + old * s for x in rows[m]]
        if len(v) > 1:
            b = last(v) if bug == "last_max_pre" else first(v)
            ratio = b / ((MAXC if bug == "ratio_max_chunks" else len(v)) - 1)
            v[b] = max(0.0, min(1.0, v[b] + (boost - (boost + decay) * ratio)))
        b = last(v) if bug == "last_max_post" else first(v)
        tie = {"ties_by_slot": m, "ties_desc_doc": -int(doc[m])}.get(bug, int(doc[m]))
        res.append(((-v[b], tie), int(doc[m]), v[b], old, int(meta[m, 2]) + b))
    res.sort(key=lambda r: r[0])
    for r, (_, d, sc, o, ch) in enumerate(res):
        out_doc[r], out_score[r], out_orig[r], out_chunk[r] = d, sc, o, ch
    return out_doc, out_score, out_orig, out_chunk, len(res), sum(len(rows[m]) for m in kept)


def fuse_ref(c):
    return rerank_ref.fuse_from_gather(c["doc"], c["bm"], c["n"], c["cos"], c["meta"], *c["prm"])


def same_fuse(a, b):
    """The six outputs equal: documents, chunk rows and counts as integers, score and orig as float64 bits."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(np.asarray(a[1], np.float64).view(np.int64), np.asarray(b[1], np.float64).view(np.int64))
            and np.array_equal(np.asarray(a[2], np.float64).view(np.int64), np.asarray(b[2], np.float64).view(np.int64))
            and np.array_equal(a[3], b[3]) and int(a[4]) == int(b[4]) and int(a[5]) == int(b[5]))


# ------------------------------------------------------------------ the gather's corpus
def gather_corpus(seed=5, n_random=1500):
    """-> dict(emb [C, 768] f32, doc_off [N + 1] i32, url_group [N] i32, special (names -> document), queries [Q0, 768] f32).
    Documents 0 .. 6 have 2, 0, 1, 9, 10, 11, 300 rows (the corpus' first row is document 0's); document 3 holds a zero
    row, rows of norm 1e-3 and 1e3 and a near-duplicate pair; then n_random documents of 0 .. 12 rows and a last document
    of 3 rows (the corpus' last row).  URL groups pair neighbouring random documents, some have none (-1)."""
    rng = np.random.default_rng(seed)
    n_rows = [2, 0, 1, 9, 10, 11, 300] + [int(x) for x in rng.integers(0, 13, n_random)] + [3]
    off = np.concatenate([[0], np.cumsum(n_rows)]).astype(np.int32)
    C = int(off[-1])
    emb = (rng.standard_normal((C, DIM)) * rng.uniform(0.3, 3.0, (C, 1))).astype(np.float32)
    r3 = int(off[3])
    emb[r3] = 0.0
    emb[r3 + 1] *= np.float32(1e-3) / np.linalg.norm(emb[r3 + 1].astype(np.float64))
    emb[r3 + 2] *= np.float32(1e3) / np.linalg.norm(emb[r3 + 2].astype(np.float64))
    emb[r3 + 4] = emb[r3 + 3] + np.float32(2.0 ** -20) * rng.standard_normal(DIM).astype(np.float32)
    emb[r3 + 5] = emb[r3 + 3]
    N = len(n_rows)
    grp = np.arange(N, dtype=np.int32) // 2
    grp[rng.random(N) < 0.05] = -1
    grp[:8] = np.arange(8)
    q = rng.standard_normal((8, DIM)).astype(np.float32)
    q[1] = emb[0]                                       # cos ~ 1 with the corpus' first row
    q[2] = -emb[C - 1]                                  # cos ~ -1 with its last row
    q[3] = emb[r3 + 3]                                  # equal to one of the near-duplicates
    q[4] *= np.float32(1e-3)
    q[5] *= np.float32(1e4)
    return dict(emb=emb, doc_off=off, url_group=grp, queries=q, N=N, C=C)


def candidates(rng, N, Q, n_range=(1, M), p_dup=0.05, lo=-3, extra=5):
    """Q candidate lists of M slots: documents in [lo, N + extra) (absent and out-of-range ones included), repeats, garbage
    past cand_n."""
    cand = rng.integers(lo, N + extra, (Q, M)).astype(np.int32)
    for q in range(Q):
        cand[q] = rng.permutation(np.arange(N))[:M] if N >= M and rng.random() < 0.5 else cand[q]
        dup = rng.random(M) < p_dup
        cand[q, dup] = cand[q, rng.integers(0, M, int(dup.sum()))]
    n = rng.integers(n_range[0], n_range[1] + 1, Q).astype(np.int32)
    return cand, n


def cos64(q, E):
    """float64 cosines of q [Q, 768] with rows E [R, 768], zero norms replaced by 1 (sklearn normalize) -> (cos [Q, R],
    A [Q, R] = sum_i |e_i q_i| / (|e| |q|))."""
    q = np.asarray(q, np.float64); E = np.asarray(E, np.float64)
    qn = np.linalg.norm(q, axis=1); qn[qn == 0] = 1.0
    en = np.linalg.norm(E, axis=1); en[en == 0] = 1.0
    return (q @ E.T) / qn[:, None] / en[None, :], (np.abs(q) @ np.abs(E).T) / qn[:, None] / en[None, :]


GATHER_A, GATHER_B = 20.0, 12.0     # the bar's coefficients (derivation: tests/test_gpu_rerank.py)


def gather_bar(A, c, inv_rel=13.0 * U32):
    """|gathered - exact| <= U32 (GATHER_A A + GATHER_B |c|) + inv_rel |c| (+ second order): A = sum |e_i q_i| / (|e| |q|),
    c the exact cosine, inv_rel the relative error of the row's inv_norm."""
    return (U32 * (GATHER_A * A + GATHER_B * np.abs(c)) + inv_rel * np.abs(c)) * (1.0 + 64 * U32)


def gather_restated(q, E, rows="f32", inv="exact", shift=0):
    """A gather restated in float64 from altered inputs -- rows rounded to f16 / bf16, the row `shift` places further
    (the neighbouring document's), or no inv_norm (a dot with the unit query only)."""
    import torch
    E = np.asarray(E, np.float32)
    if rows == "f16":
        E = E.astype(np.float16).astype(np.float32)
    elif rows == "bf16":
        E = torch.as_tensor(E).to(torch.bfloat16).float().numpy()
    if shift:
        E = np.roll(E, -shift, axis=0)
    q = np.asarray(q, np.float64)
    qn = np.linalg.norm(q, axis=1); qn[qn == 0] = 1.0
    en = np.linalg.norm(E.astype(np.float64), axis=1); en[en == 0] = 1.0
    dot = (q / qn[:, None]) @ E.astype(np.float64).T
    return dot if inv == "none" else dot / en[None, :]
