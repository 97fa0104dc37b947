"""The oracle of the near-duplicate collapse (DESIGN K18; include/msretr.h states the definitions): min-hash signatures and the
greedy collapse, each as plain Python loops over Python integers and as vectorised numpy, and the case generators the CPU and
GPU tests share.  Nothing here touches the package's native code."""
import numpy as np

K = 64                       # MSR_SIG_WORDS
MAX_SHINGLE = 8              # MSR_SIG_MAX_SHINGLE
M32 = 0xFFFFFFFF
EMPTY = np.full(K, M32, np.uint32)
FNV = 0x01000193


def fmix(x):
    x &= M32
    x ^= x >> 16
    x = x * 0x85EBCA6B & M32
    x ^= x >> 13
    x = x * 0xC2B2AE35 & M32
    x ^= x >> 16
    return x


A = [fmix(2 * k + 1) | 1 for k in range(K)]
B = [fmix(2 * k + 2) for k in range(K)]


# ---- plain loops ----------------------------------------------------------------------------------------------------------------
def shingle_hashes(stream, w):
    s = [int(t) for t in stream]
    n = len(s)
    if n == 0:
        return []
    L = min(int(w), n)
    out = []
    for a in range(n - L + 1):
        x = 0
        for j in range(L):
            x = ((x ^ ((s[a + j] + 1) & M32)) * FNV) & M32
        out.append(fmix(x ^ L))
    return out


def signature(stream, w):
    """uint32 [64]: the signature of one token stream with shingle width w."""
    hs = shingle_hashes(stream, w)
    if not hs:
        return EMPTY.copy()
    return np.array([min((A[k] * h + B[k]) & M32 for h in hs) for k in range(K)], np.uint32)


def matches(x, y):
    return sum(int(a) == int(b) for a, b in zip(x, y))


def is_empty(sig):
    return all(int(v) == M32 for v in sig)


def collapse(docs, sigs, min_matches, passive=None):
    """docs: the document index of each slot, in fused order; sigs: uint32 [N, 64], the signature table; passive: per slot
    True for a slot that a domain table rejects (None: none) -- a slot is ALSO passive when its document lies outside the
    table or its signature is EMPTY.  -> (kept slots, [(dropped slot, leader slot, matches)] in drop order)."""
    n_sig = len(sigs)
    kept, leaders, drops = [], [], []
    for i, d in enumerate(docs):
        d = int(d)
        pas = (passive is not None and bool(passive[i])) or d < 0 or d >= n_sig or is_empty(sigs[d])
        lead = None
        if not pas:
            for j in leaders:                                # ascending slots: the first hit is the smallest
                m = matches(sigs[d], sigs[int(docs[j])])
                if m >= min_matches:
                    lead = (j, m)
                    break
        if lead is None:
            kept.append(i)
            if not pas:
                leaders.append(i)
        else:
            drops.append((i, lead[0], lead[1]))
    return kept, drops


# ---- vectorised -----------------------------------------------------------------------------------------------------------------
_A = np.array(A, np.uint32)
_B = np.array(B, np.uint32)


def _fmix_np(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def signature_fast(stream, w):
    s = np.asarray(stream, np.int64).astype(np.uint32)
    n = len(s)
    if n == 0:
        return EMPTY.copy()
    L = min(int(w), n)
    starts = n - L + 1
    with np.errstate(over="ignore"):
        x = np.zeros(starts, np.uint32)
        for j in range(L):
            x = (x ^ (s[j:j + starts] + np.uint32(1))) * np.uint32(FNV)
        h = _fmix_np(x ^ np.uint32(L))
        sig = np.full(K, M32, np.uint32)
        for a in range(0, starts, 4096):
            sig = np.minimum(sig, (_A[:, None] * h[None, a:a + 4096] + _B[:, None]).min(axis=1))
    return sig


def signatures_fast(tok_off, tok_ids, w, d0=0, d1=None):
    """uint32 [d1 - d0, 64]: the signatures of documents [d0, d1) of a forward index."""
    tok_off = np.asarray(tok_off, np.int64)
    d1 = len(tok_off) - 1 if d1 is None else d1
    return np.stack([signature_fast(tok_ids[tok_off[d]:tok_off[d + 1]], w) for d in range(d0, d1)]) if d1 > d0 \
        else np.zeros((0, K), np.uint32)


def collapse_fast(docs, sigs, min_matches, passive=None):
    """collapse() with the pairwise match counts from one numpy comparison."""
    docs = np.asarray(docs, np.int64)
    n, n_sig = len(docs), len(sigs)
    if n == 0:
        return [], []
    inside = (docs >= 0) & (docs < n_sig)
    rows = np.where(inside[:, None], np.asarray(sigs, np.uint32)[np.where(inside, docs, 0)], EMPTY[None, :]) if n_sig else \
        np.tile(EMPTY, (n, 1))
    active = inside & ~(rows == M32).all(axis=1)
    if passive is not None:
        active &= ~np.asarray(passive, bool)
    m = (rows[:, None, :] == rows[None, :, :]).sum(axis=2)
    dup = (m >= min_matches) & active[:, None] & active[None, :]
    kept_mask = np.zeros(n, bool)
    kept, drops = [], []
    for i in range(n):
        hit = np.nonzero(dup[i, :i] & kept_mask[:i])[0]
        if len(hit):
            drops.append((i, int(hit[0]), int(m[i, hit[0]])))
        else:
            kept.append(i)
            kept_mask[i] = active[i]                         # a passive slot is kept and leads nothing
    return kept, drops


def collapse_lists(fused_doc, fused_score, fused_orig, fused_chunk, fused_n, sigs, min_matches, domain=None):
    """The call's outputs for [Q, M] lists, as msr_collapse_duplicates pads them -> (doc, score, orig, chunk, n, drop_doc,
    drop_leader, drop_matches, drop_n).  domain: None or the bound doc-domain table (int32, by document index)."""
    fused_doc = np.asarray(fused_doc)
    Q, M = fused_doc.shape
    o_doc, o_chunk = np.full((Q, M), -1, np.int32), np.full((Q, M), -1, np.int32)
    o_score, o_orig = np.full((Q, M), -np.inf), np.zeros((Q, M))
    d_doc, d_lead, d_m = np.full((Q, M), -1, np.int32), np.full((Q, M), -1, np.int32), np.zeros((Q, M), np.int32)
    o_n, d_n = np.zeros(Q, np.int32), np.zeros(Q, np.int32)
    for q in range(Q):
        n = min(max(int(fused_n[q]), 0), M)
        docs = fused_doc[q, :n]
        passive = None
        if domain is not None:
            passive = [not (0 <= int(d) < len(domain)) or int(domain[int(d)]) < 0 for d in docs]
        kept, drops = collapse_fast(docs, sigs, min_matches, passive)
        o_n[q], d_n[q] = len(kept), len(drops)
        o_doc[q, :len(kept)] = docs[kept]
        o_score[q, :len(kept)] = np.asarray(fused_score)[q, kept]
        o_orig[q, :len(kept)] = np.asarray(fused_orig)[q, kept]
        o_chunk[q, :len(kept)] = np.asarray(fused_chunk)[q, kept]
        for p, (i, j, m) in enumerate(drops):
            d_doc[q, p], d_lead[q, p], d_m[q, p] = docs[i], docs[j], m
    return o_doc, o_score, o_orig, o_chunk, o_n, d_doc, d_lead, d_m, d_n


# ---- case generators ------------------------------------------------------------------------------------------------------------
LONG = 5000                  # a document of more than one segment of 4096 shingle starts: the kernel's shared path
LONGER = 40000               # ... and of more segments than the workgroup has waves: a wave takes a second segment


def stream_lengths(w):
    """The stream lengths at which the signature kernel takes another path for shingle width w."""
    return [0, 1, max(w - 1, 0), w, w + 1, 63, 64, 65, 64 + w - 1, 127, 128, 129, LONG]


def forward_index(n_terms=1000, seed=7):
    """Token streams for the signature kernel, every shingle width at once -> list of int32 arrays: a document of every length
    of stream_lengths(w), w = 1 .. 8, shuffled so that short ones stand behind long ones; one stream cut in two NEIGHBOURS, so
    that the second's first tokens would complete the first's last shingle (then the uncut stream, which must differ from
    both); term id n_terms - 1, alone and repeated; a 40 000-token document among the short ones; an empty document FIRST
    and the 5000-token document LAST in the buffer."""
    rng = np.random.default_rng(seed)
    lengths = sorted({n for w in range(1, MAX_SHINGLE + 1) for n in stream_lengths(w)} - {0, LONG})
    docs = [rng.integers(0, n_terms, n).astype(np.int32) for n in lengths]
    docs += [np.full(70, n_terms - 1, np.int32), np.array([n_terms - 1], np.int32), np.zeros(0, np.int32)]
    docs = [docs[i] for i in rng.permutation(len(docs))]
    whole = rng.integers(0, n_terms, 2 * MAX_SHINGLE + 3).astype(np.int32)
    docs[5:5] = [whole[:MAX_SHINGLE + 1], whole[MAX_SHINGLE + 1:], whole.copy()]
    docs.insert(12, rng.integers(0, n_terms, LONGER).astype(np.int32))
    return [np.zeros(0, np.int32)] + docs + [rng.integers(0, n_terms, LONG).astype(np.int32)]


def index_of(streams, n_terms):
    """A postings-only CorpusIndex whose tables agree with the streams (a document without tokens has doc_len 0 and no
    posting), with the streams as its forward index -> (ix, tok_off, tok_ids)."""
    from msretr.index import CorpusIndex
    N = len(streams)
    lens = np.array([len(s) for s in streams], np.int64)
    off = np.zeros(N + 1, np.int64)
    off[1:] = np.cumsum(lens)
    tok = np.concatenate([np.asarray(s, np.int32) for s in streams] + [np.zeros(0, np.int32)]).astype(np.int32)
    key = tok.astype(np.int64) * N + np.repeat(np.arange(N), lens)
    uniq, tf = np.unique(key, return_counts=True)
    term_off = np.zeros(n_terms + 1, np.int64)
    term_off[1:] = np.cumsum(np.bincount(uniq // N, minlength=n_terms))
    rows = lens[lens > 0]
    ix = CorpusIndex(doc_ids=np.arange(N, dtype=np.int64) * 3 + 7, doc_len=lens.astype(np.int32), term_off=term_off,
                     post_doc=(uniq % N).astype(np.int32), post_tf=tf.astype(np.int32),
                     idf=np.linspace(0.5, 2.0, n_terms).astype(np.float32), avgdl=float(np.float32(rows.mean())),
                     total_docs=len(rows), tok_off=off, tok_ids=tok)
    ix.n_docs_global = N
    return ix, off, tok


def near_copies(n_groups, copies, length=120, edits=2, n_terms=5000, seed=3):
    """Token streams for collapse cases: n_groups random pages, each followed by `copies` near-copies with up to `edits`
    tokens replaced (copy c of a page: 1 + c * edits // copies of them) -> (list of streams, group of each stream)."""
    rng = np.random.default_rng(seed)
    streams, group = [], []
    for g in range(n_groups):
        base = rng.integers(0, n_terms, length).astype(np.int32)
        streams.append(base)
        group.append(g)
        for k in range(copies):
            c = base.copy()
            e = 1 + k * edits // max(copies, 1)
            c[rng.integers(0, length, e)] = rng.integers(0, n_terms, e)
            streams.append(c)
            group.append(g)
    return streams, group


# ---- planted tables: exact match counts (bound directly with msr_bind_signatures) ----------------------------------------------
def planted_table(n_fill=1100):
    """A signature table with the match count of every pair of rows known: every word is unique in the table unless planted.
    -> (sig uint32 [N, 64], rows) with rows:
      pairs[(m, "first")] / pairs[(m, "last")] = (a, b), m = 0 .. 64: rows that agree in exactly the FIRST / the LAST m words;
      ones = (x, y, z): x holds one word of 0xFFFFFFFF (not EMPTY), y is x again (64 matches), z holds it in another word;
      empty = two EMPTY rows;  chain = (a, b, c): a ~ b 61, b ~ c 61, a ~ c 58;  two = (a, e, d): d ~ a 60, d ~ e 60, a ~ e 56;
      fill = n_fill rows that match nothing."""
    rows, table = {"pairs": {}}, []

    def fresh():
        r = len(table)
        table.append(np.arange(r * K + 1, r * K + K + 1, dtype=np.uint32))   # words r K + 1 .. r K + 64: unique, never 0xFFFFFFFF
        return r

    def copy_of(src, words):
        r = fresh()
        table[r][words] = table[src][words]
        return r

    for m in range(K + 1):
        a = fresh()
        rows["pairs"][(m, "first")] = (a, copy_of(a, slice(0, m)))
        a = fresh()
        rows["pairs"][(m, "last")] = (a, copy_of(a, slice(K - m, K)))
    x = fresh()
    table[x][0] = M32
    y = copy_of(x, slice(0, K))
    z = fresh()
    table[z][K - 1] = M32
    rows["ones"] = (x, y, z)
    rows["empty"] = (fresh(), fresh())
    for r in rows["empty"]:
        table[r][:] = M32
    a = fresh()
    b = copy_of(a, slice(3, K))
    c = copy_of(b, slice(0, K))
    table[c][3:6] += np.uint32(1 << 30)
    rows["chain"] = (a, b, c)
    a = fresh()
    d = copy_of(a, slice(0, 60))
    e = copy_of(d, slice(0, K))
    table[e][56:60] += np.uint32(1 << 30)
    rows["two"] = (a, e, d)
    rows["fill"] = [fresh() for _ in range(n_fill)]
    return np.stack(table), rows


def planted_pair_lists(rows, max_cand):
    """Three lists over every planted pair -> doc int32 [3, max_cand], n: the pairs side by side (a0 b0 a1 b1 ..); every a, then
    every b (a pair's rows in different tiles); and the first list behind one EMPTY row, so that pairs straddle the tile edges."""
    pairs = [rows["pairs"][k] for k in sorted(rows["pairs"])]
    flat = [r for p in pairs for r in p]
    assert max_cand >= len(flat) + 1
    doc = np.full((3, max_cand), -1, np.int32)
    doc[0, :len(flat)] = flat
    doc[1, :len(flat)] = [a for a, _ in pairs] + [b for _, b in pairs]
    doc[2, :len(flat) + 1] = [rows["empty"][0]] + flat
    return doc, np.array([len(flat), len(flat), len(flat) + 1], np.int32)


def full_width_list(rows, n_sig):
    """One list of 1024 slots of rows that match nothing, but: a leader at slot 600 whose copy stands at 1000 (the last tile);
    the chain A ~ B ~ C at slots 10, 100, 700 (three tiles); a row at 990 that duplicates the leaders at 20 and 530 (the
    smaller slot takes it); passive slots at 63, 64 (the two EMPTY rows) and 1023 (a document outside the table)."""
    doc = np.array(rows["fill"][:1024], np.int32)
    x, y, _ = rows["ones"]
    doc[600], doc[1000] = x, y
    doc[10], doc[100], doc[700] = rows["chain"]
    doc[20], doc[530], doc[990] = rows["two"]
    doc[63], doc[64] = rows["empty"]
    doc[1023] = n_sig + 3
    return doc


def many_pair_queries(rows, n_queries):
    """[n_queries, 2] lists of one planted pair each: query q holds pair (7 q + 3) mod 130."""
    pairs = np.array([rows["pairs"][k] for k in sorted(rows["pairs"])], np.int32)
    return pairs[(np.arange(n_queries, dtype=np.int64) * 7 + 3) % len(pairs)]


def pair_matches(rows):
    """The planted count of each pair, in the order of sorted(rows["pairs"])."""
    return np.array([m for m, _ in sorted(rows["pairs"])], np.int32)
