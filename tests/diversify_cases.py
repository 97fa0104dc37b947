"""Lists for the response's last step, msr_diversify: the oracle, a second formulation and the
case generators the CPU and GPU tests share.  TEST INFRASTRUCTURE ONLY: pure Python and numpy, nothing here touches the
package's native code.

A case is a dict: name, doc int32 [len], score float64 [len] (descending), optionally n (the fused_n to send; default len) and
top_k.  A document's domain is a function of its index alone, so that every case fits ONE bound table (DOMAIN_TABLE): document
d < REJECTED_FROM belongs to domain d // SLOTS, every document from REJECTED_FROM on is one the response models reject.
`domains(doc, table)` states what the kernel makes of another table: none bound -- every document its own domain, a negative
index rejected; a shorter one -- an index at or past its end rejected.

`expected` is the oracle: oracle.rerank_ref.hybrid_diversification (pinned to the reference-executed fixtures
tests/golden/diversification.json and diversification_edges.json) on the accepted entries.  `reduced` is DESIGN K6b's
reduction as plain loops, written from DESIGN's text: the kernel implements that reduction, test_diversify_cases.py shows
that it IS the oracle on every case below, the GPU tests compare the kernel with the oracle."""
import itertools
import json
import os

import numpy as np

from oracle import rerank_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLOTS = 1024                                   # documents per domain in DOMAIN_TABLE (a list's slot picks one of them)
N_DOMAINS = 1024
REJECTED_FROM = N_DOMAINS * SLOTS
DOMAIN_TABLE = np.concatenate([np.arange(REJECTED_FROM, dtype=np.int32) // SLOTS, np.full(SLOTS, -1, np.int32)])
THRESHOLDS = (0.8, 0.0, 1.0, 1.5, -1.0)        # the reference's; every score at or above; only 1.0 high; no high tier; all high
T = 0.8
BELOW = float(np.nextafter(T, 0))


def domains(doc, table=DOMAIN_TABLE):
    """int64 [len]: the domain of each entry, -1 = rejected, as msr_diversify reads the bound table (None: none bound)."""
    doc = np.asarray(doc, np.int64)
    if table is None:
        return np.where(doc >= 0, doc, -1)
    table = np.asarray(table)
    inside = (doc >= 0) & (doc < len(table))
    return np.where(inside, table[np.where(inside, doc, 0)], -1).astype(np.int64)


def length(case, max_cand=None):
    """The entries of the case the call looks at: fused_n clamped to [0, max_cand]."""
    n = int(case.get("n", len(case["doc"])))
    return min(max(n, 0), len(case["doc"]) if max_cand is None else max_cand)


def _accepted(case, table, max_cand):
    n = length(case, max_cand)
    dom = domains(case["doc"][:n], table)
    return [(i, int(dom[i]), float(case["score"][i])) for i in range(n) if dom[i] >= 0]


def expected(case, top_k, threshold=T, diversification=True, table=DOMAIN_TABLE, max_cand=None):
    """-> [(slot, score)]: the final list, by the oracle.  Rejected entries are removed beforehand, as the response models
    do (reranker_api.py:376-397); diversification=False: the first top_k accepted entries."""
    items = [{"slot": i, "url": f"https://h{g}.de/x", "similarity_score": s} for i, g, s in _accepted(case, table, max_cand)]
    out = rerank_ref.hybrid_diversification(items, relevance_threshold=threshold, top_k=top_k) if diversification else items[:top_k]
    return [(it["slot"], it["similarity_score"]) for it in out]


def reduced(case, top_k, threshold=T, diversification=True, table=DOMAIN_TABLE, max_cand=None):
    """-> [(slot, score)]: DESIGN K6b's reduction on a list in descending order, as plain loops."""
    acc = _accepted(case, table, max_cand)
    if not diversification:
        return [(i, s) for i, _, s in acc[:top_k]]
    tier = {}                                  # domain -> True iff its FIRST entry scores >= threshold
    kept_high, kept_medium, dropped = [], [], []
    for pos, (i, g, s) in enumerate(acc):
        if g not in tier:
            tier[g] = s >= threshold
            (kept_high if tier[g] else kept_medium).append((i, s))
        else:
            dropped.append((pos, tier[g], i, s))
    remaining = top_k - len(kept_high)
    final = kept_high + kept_medium[:remaining]                 # (Python slice semantics: a negative bound drops from the END)
    if len(final) < top_k and dropped:
        order = []                             # stable by score, the high tier's drops first on equal scores, then list order
        for e in dropped:
            at = len(order)
            while at > 0 and (order[at - 1][3] < e[3] or (order[at - 1][3] == e[3] and e[1] and not order[at - 1][1])):
                at -= 1
            order.insert(at, e)
        add = order[:top_k - len(final)]
        delta = add[0][3] - final[-1][1] + 1e-4
        final = final + [(i, max(0.0, s - delta)) for _, _, i, s in add]
    return final


def anatomy(case, top_k, threshold=T, table=DOMAIN_TABLE):
    """The counts an edge list is built for, from the oracle's own pieces (apply_domain_cap on the two tiers): n_accepted,
    n_high (kept entries of high domains), n_kept, n_dropped, remaining = top_k - n_high, n_medium, n_final (before the fill),
    n_added, delta (None without a fill), last_kept."""
    items = [{"slot": i, "url": f"https://h{g}.de/x", "similarity_score": s} for i, g, s in _accepted(case, table, None)]
    dom = lambda d: rerank_ref.extract_domain(d["url"])
    hi = {dom(d) for d in items if d["similarity_score"] >= threshold}
    kept_h, drop_h = rerank_ref.apply_domain_cap([d for d in items if dom(d) in hi], 1)
    kept_m, drop_m = rerank_ref.apply_domain_cap([d for d in items if dom(d) not in hi], 1)
    remaining = top_k - len(kept_h)
    final = kept_h + kept_m[:remaining]
    rest = sorted(drop_h + drop_m, key=lambda d: d["similarity_score"], reverse=True)
    add = rest[:max(top_k - len(final), 0)]
    return dict(n_accepted=len(items), n_high=len(kept_h), n_medium=len(kept_m), n_kept=len(kept_h) + len(kept_m),
                n_dropped=len(rest), remaining=remaining, n_final=len(final), n_added=len(add),
                delta=add[0]["similarity_score"] - final[-1]["similarity_score"] + 1e-4 if add else None,
                last_kept=final[-1]["similarity_score"] if final else None,
                tie_across_tiers=any(a["similarity_score"] == b["similarity_score"] for a in drop_h for b in drop_m))


# ---- generators -------------------------------------------------------------------------------------------------------------
def make(name, entries, top_k=None, n=None, **claims):
    """entries: (domain or None = rejected, score) per slot, or (domain, score, document) to name the document."""
    doc = np.zeros(len(entries), np.int32)
    for i, e in enumerate(entries):
        doc[i] = e[2] if len(e) > 2 else (REJECTED_FROM + i % SLOTS if e[0] is None else e[0] * SLOTS + i % SLOTS)
    score = np.array([e[1] for e in entries], np.float64)
    assert (np.diff(score) <= 0).all(), name
    c = dict(name=name, doc=doc, score=score, claims=claims)
    if top_k is not None:
        c["top_k"] = top_k
    if n is not None:
        c["n"] = n
    return c


def score_patterns(n):
    """Descending score rows of length n: all distinct (across the threshold, all above, all below), all equal (above, at the
    threshold, zero), ties on the threshold's two sides, exactly the threshold and one ulp below it, zeros at the end, and
    5e-5 (a kept score below the 1e-4 shift: the shifted tail clamps at 0)."""
    half = (n + 1) // 2
    rows = [
        [0.95, 0.9, 0.85, 0.5, 0.3][:n],
        [0.99, 0.95, 0.9, 0.85, 0.81][:n],
        [0.7, 0.6, 0.5, 0.4, 0.3][:n],
        [0.9] * n,
        [T] * n,
        [0.0] * n,
        [0.9] * half + [0.5] * (n - half),
        [T] * half + [BELOW] * (n - half),
        [0.9, T, BELOW, 0.5, 0.5][:n],
        [0.9, 0.5][:max(n - 2, 1)] + [0.0] * (n - len([0.9, 0.5][:max(n - 2, 1)])),
        [0.9] + [5e-5] * (n - 1),
    ]
    seen, out = set(), []
    for r in rows:
        if tuple(r) not in seen:
            seen.add(tuple(r))
            out.append(r)
    return out


def small_lists(max_len=5):
    """The exhaustive set -> cases with a top_k each: every length 1 .. max_len, every assignment of {rejected, domain 0, 1, 2}
    to the slots, every row of score_patterns, every top_k from 1 to n + 1."""
    out = []
    for n in range(1, max_len + 1):
        pats = score_patterns(n)
        for assign in itertools.product((None, 0, 1, 2), repeat=n):
            for p, row in enumerate(pats):
                doc = np.array([REJECTED_FROM + i if g is None else g * SLOTS + i for i, g in enumerate(assign)], np.int32)
                score = np.array(row, np.float64)
                for top_k in range(1, n + 2):
                    out.append(dict(name=f"small{n}", doc=doc, score=score, top_k=top_k))
    return out


def _desc(rng, n, lo=0.0, hi=1.0):
    return -np.sort(-rng.uniform(lo, hi, n))


def edge_lists():
    """Named lists, each built for one edge (its `claims` are asserted from the oracle's pieces by test_diversify_cases.py).
    The lists of at most 40 entries are also the inputs of the reference-executed fixture diversification_edges.json."""
    K = 5
    out = []
    hi_scores = lambda h: [0.99 - 0.01 * i for i in range(h)]                 # h distinct scores >= 0.89
    # the number of high domains against top_k, with n_medium chosen for the sign of n_medium + remaining
    for h, m, sign in ((K - 1, 3, 1), (K, 3, 1), (K + 1, 3, 1), (2 * K, 2, -1), (2 * K, K, 0), (K + 1, 1, 0)):
        e = [(g, s) for g, s in enumerate(hi_scores(h))] + [(100 + j, 0.7 - 0.05 * j) for j in range(m)]
        e += [(0, 0.35), (100, 0.3), (1, 0.25)][:3]                            # drops of both tiers behind them
        out.append(make(f"high{h}_medium{m}", e, K, n_high=h, n_medium=m, slice_sign=sign))
    for kept in (K - 1, K, K + 1):             # kept entries against top_k: two high domains, the rest medium, drops between
        e = [(0, 0.95), (0, 0.93), (1, 0.9)] + [(10 + j, 0.7 - 0.05 * j) for j in range(kept - 2)] + [(10, 0.2), (1, 0.1)]
        out.append(make(f"kept{kept}", e, K, n_kept=kept, n_high=2))
    for acc in (K - 1, K, K + 1):              # accepted entries against top_k, rejected ones between them
        e = [(None, 0.97)] + [(j % 3, 0.9 - 0.1 * j) for j in range(acc)]
        e.insert(3, (None, 0.75))
        e.append((None, 0.0))
        out.append(make(f"accepted{acc}", e, K, n_accepted=acc))
    out.append(make("nothing_dropped", [(j, 0.9 - 0.1 * j) for j in range(4)], K, n_dropped=0, n_added=0))
    out.append(make("all_high_nothing_added", [(j, 0.95 - 0.01 * j) for j in range(3)], K, n_dropped=0, n_added=0, n_high=3, n_final=3))
    out.append(make("high_only_list_longer_than_top_k", [(j, 0.95 - 0.01 * j) for j in range(9)], K, n_high=9, n_final=9, n_added=0))
    out.append(make("one_domain", [(7, 0.9 - 0.05 * j) for j in range(12)], K, n_kept=1, n_added=K - 1))
    out.append(make("one_domain_medium", [(7, 0.6 - 0.05 * j) for j in range(12)], K, n_kept=1, n_high=0, n_added=K - 1))
    # a dropped-high and a dropped-medium entry with equal scores, in both list orders: the high tier's drop is added first
    out.append(make("tie_high_drop_first", [(0, 0.9), (1, 0.6), (0, 0.5), (1, 0.5)], 3, tie_across_tiers=True, n_added=1))
    out.append(make("tie_medium_drop_first", [(0, 0.9), (1, 0.6), (1, 0.5), (0, 0.5)], 3, tie_across_tiers=True, n_added=1))
    out.append(make("tie_three_each", [(0, 0.9), (1, 0.6), (1, 0.5), (0, 0.5), (1, 0.5), (0, 0.5), (0, 0.5), (1, 0.5)], 6,
                    tie_across_tiers=True, n_added=4))
    out.append(make("tie_at_threshold_drops", [(0, T), (1, BELOW), (1, BELOW), (0, BELOW), (1, BELOW), (0, BELOW)], 4,
                    tie_across_tiers=True, n_added=2, n_high=1))
    out.append(make("threshold_and_one_ulp_below", [(0, 0.9), (1, T), (2, BELOW), (3, BELOW), (2, 0.1)], K, n_high=2, n_medium=2))
    out.append(make("last_kept_zero", [(0, 0.9), (1, 0.0), (1, 0.0), (0, 0.0)], 4, last_kept=0.0, n_added=2, delta_sign=1))
    out.append(make("last_kept_below_the_shift", [(0, 0.9), (1, 5e-5), (1, 5e-5), (0, 4e-5)], 4, last_kept=5e-5, n_added=2, delta_sign=1))
    out.append(make("first_drop_far_below", [(0, 0.9), (1, 0.85), (2, 0.6), (0, 0.1), (1, 0.05)], K, delta_sign=-1, n_added=2))
    out.append(make("first_drop_above_last_kept", [(0, 0.9), (0, 0.85), (0, 0.8), (1, 0.3), (1, 0.2)], K, delta_sign=1, n_added=3))
    rng = np.random.default_rng(17)
    s = _desc(rng, 40)
    out.append(make("random_doubles", [(int(g), float(x)) for g, x in zip(rng.integers(0, 6, 40), s)], 20, n_kept=6, n_added=14))
    s = np.repeat(_desc(rng, 20), 2)           # every score twice: equality is a comparison of all 64 bits
    out.append(make("random_doubles_in_pairs", [(int(g), float(x)) for g, x in zip(rng.integers(0, 5, 40), s)], 30, n_kept=5, n_added=25))
    near = [float(np.nextafter(0.5, 1)), 0.5, 0.5, float(np.nextafter(0.5, 0)), float(np.nextafter(0.5, 0))]
    out.append(make("one_ulp_apart_drops", [(0, 0.9), (1, 0.7)] + [(g, x) for g, x in zip((1, 0, 1, 0, 1), near)], 6, n_added=4))
    # documents repeated in a list (what a caller's merged lists may hold): entries, not documents, are kept and dropped
    out.append(make("documents_repeated", [(0, 0.9, 5), (1, 0.7, SLOTS + 5), (0, 0.6, 5), (1, 0.5, SLOTS + 5), (0, 0.4, 6), (0, 0.3, 5)], K,
                    n_kept=2, n_added=3))
    # ---- full width -----------------------------------------------------------------------------------------------------------
    out.append(make("thousand_one_score_two_domains", [(j % 2, 0.5) for j in range(1000)], 1000, n_kept=2, n_added=998))
    out.append(make("thousand_one_high_score_two_domains", [(j // 500, 0.9) for j in range(1000)], 700, n_kept=2, n_added=698))
    # accepted entries only at the slots around every multiple of 64 and at 1023: each wave edge of the first scan is crossed
    # with a count that differs from the slot
    at = sorted({x for k in range(1, 16) for x in (64 * k - 1, 64 * k, 64 * k + 1)} | {0, 1023})
    s = _desc(rng, 1024)
    e = [((at.index(i) % 9) if i in at else None, float(s[i])) for i in range(1024)]
    out.append(make("accepted_around_the_wave_edges", e, 30, n_accepted=len(at), n_kept=9))
    # ... and rejected entries at a few slots only: accepted, kept and kept-high RANKS cross the wave edges of all three scans
    gone = {0, 10, 64, 130, 500, 1022}
    e = [(None if i in gone else int(rng.integers(0, 300)), float(s[i])) for i in range(1024)]
    out.append(make("ranks_across_the_wave_edges", e, 1000, n_accepted=1024 - len(gone)))
    out.append(make("ranks_across_the_wave_edges_top100", e, 100, n_accepted=1024 - len(gone)))
    e = [(None if i in gone else i, float(s[i])) for i in range(1024)]      # every entry kept: the kept ranks reach 1017
    out.append(make("every_entry_kept", e, 1000, n_dropped=0, n_kept=1024 - len(gone)))
    e = [(i // 2, float(x)) for i, x in enumerate(_desc(rng, 1024, 0.8, 1.0))]
    out.append(make("high_domains_in_pairs", e, 600, n_high=512, n_added=88))
    return out


def widths():
    """-> [(max_cand, top_k, cases)]: a list of max_cand entries sent with every fused_n of interest (one query each)."""
    out = []
    for M in (1, 2, 63, 64, 65, 1000, 1024):
        rng = np.random.default_rng(1000 + M)
        s = np.round(_desc(rng, M), 2)                                         # ties, on both sides of the threshold
        g = rng.integers(0, M // 3 + 1, M)
        rej = rng.random(M) < 0.1
        e = [(None if r else int(d), float(x)) for r, d, x in zip(rej, g, s)]
        for top_k in (1, M, M + 1, 5000):
            cases = [make(f"width{M}_n{n}", e, top_k, n=n) for n in (-3, 0, 1, M - 1, M, M + 7)]
            out.append((M, top_k, cases))
    return out


def fixture_inputs():
    """What the reference's own function is executed on for diversification_edges.json: the edge lists of at most 40 entries,
    at every threshold."""
    return [(c, c["top_k"], t) for t in THRESHOLDS for c in edge_lists() if len(c["doc"]) <= 40]


def load_fixture(name="diversification_edges.json"):
    with open(os.path.join(GOLDEN, name), encoding="utf-8") as f:
        return json.load(f)
