"""The plain numpy reference of the document sets that count (msr_match_sets, include/msretr_match.h; DESIGN K19): the only
source of expected values of test_match_cases.py and test_gpu_match.py.

    group_mask(z, terms) -> bool [N]                     the documents that fill a group: in the list of any of its terms
    match_mask(z, groups, need, base_mask) -> bool [N]    base AND (number of filled groups >= need), the header's conventions
    match_words(z, groups, need, base_mask) -> uint32     the same, packed (document d = bit d & 31 of word d >> 5)

z: {"term_off": int64 [V + 1], "post_doc": int [P], "n_docs": N}, as term_set_ref.py has it."""
import numpy as np

MAX_GROUPS = 64


def group_mask(z, terms):
    off, post = np.asarray(z["term_off"], np.int64), np.asarray(z["post_doc"], np.int64)
    V, N = len(off) - 1, int(z["n_docs"])
    docs = np.arange(N)
    has = np.zeros(N, bool)
    for t in terms:
        t = int(t)
        if 0 <= t < V:                                       # (a term outside the vocabulary contributes nothing)
            has |= np.isin(docs, post[off[t]:off[t + 1]])
    return has


def match_mask(z, groups, need, base_mask=None):
    """bool [N].  need <= 0: the base; more than MAX_GROUPS groups, or need above the number of groups: empty; base_mask None =
    every document."""
    N = int(z["n_docs"])
    base = np.ones(N, bool) if base_mask is None else np.array(base_mask, bool, copy=True)
    if need <= 0:
        return base
    if len(groups) > MAX_GROUPS or need > len(groups):
        return np.zeros(N, bool)
    count = np.zeros(N, np.int64)
    for g in groups:
        count += group_mask(z, g)
    return base & (count >= need)


def pack(mask):
    """bool [N] -> uint32 [ceil(N / 32)], bits at or above N zero."""
    N = len(mask)
    W = (N + 31) // 32
    padded = np.zeros(W * 32, bool)
    padded[:N] = mask
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    return (padded.reshape(W, 32).astype(np.uint64) * weights).sum(axis=1).astype(np.uint32)


def match_words(z, groups, need, base_mask=None):
    return pack(match_mask(z, groups, need, base_mask))
