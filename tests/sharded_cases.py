"""Cases for the compact rerank exchange's plan (msr_rerank_plan, include/msretr.h) and what the plan has to be, restated in
numpy from the definitions there -- no GPU:

  owner(q, m)      the shard s with bounds[s] <= cand[q, m] < bounds[s + 1], for slots m < min(cand_n[q], M) only (an empty
                   shard, bounds[s] == bounds[s + 1], owns nothing; -1, documents below bounds[0] and at or above bounds[-1]
                   belong to nobody)
  counts[s, q]     slots of query q that shard s owns
  send_base[q]     exclusive prefix over q of counts[my]: the first record of query q in my send buffer
  send_blk[q, b]   exclusive prefix, within query q, of my slots per block of 8 slots
  recv_off[s, j]   place of (source s, my j-th query) in my receive buffer: sources in rank order, each source's records in
                   query order; defined for j < hi - lo, my queries being [lo, hi) = [my qps, (my + 1) qps) cut at Q
  pair[s, o]       records source s sends to rank o: counts[s] summed over rank o's queries

tests/test_sharded_cases.py checks these against a slot-by-slot loop and that the cases hold the edges they are for;
tests/test_gpu_sharded_edges.py holds the kernels to them."""
import numpy as np

# (world, Q, M, empty shards): Q and queries_per_shard above 1024 (the offsets kernel's several elements per thread), M = 1024
# (the plan kernel's block table at its limit), M < 8 (one partial block), 64 shards of which most own no query
CASES = [
    (1, 1, 1, ()),
    (2, 3, 7, ("last",)),
    (3, 11, 8, ("mid",)),
    (5, 1025, 9, ("mid", "last")),
    (2, 2500, 16, ()),
    (8, 2048, 1000, ("mid",)),
    (64, 70, 1024, ("mid", "last")),
]
SMALL = [c for c in CASES if c[1] * c[2] <= 50000]          # what the slot-by-slot loop walks


def case_id(c):
    return f"world{c[0]}_q{c[1]}_m{c[2]}"


def make_case(world, Q, M, empty=(), seed=0):
    """-> dict(world, Q, M, qps, bounds int32 [world + 1], cand int32 [Q, M], cand_n int32 [Q])."""
    rng = np.random.default_rng([seed, world, Q, M])
    sizes = rng.integers(1, 200, world)
    if "mid" in empty and world >= 3:
        sizes[world // 2] = 0
        if world >= 16:
            sizes[3:9] = 0                                      # a run of empty shards: equal bounds several times over
    if "last" in empty and world >= 2:
        sizes[-1] = 0
    first = 7                                                   # bounds[0] > 0: documents below it belong to nobody
    bounds = np.concatenate([[first], first + np.cumsum(sizes)]).astype(np.int32)
    lo, hi = int(bounds[0]), int(bounds[-1])
    cand = rng.integers(lo - 5, hi + 5, (Q, M)).astype(np.int32)
    cand[rng.random((Q, M)) < 0.05] = -1
    cand[rng.random((Q, M)) < 0.03] = lo                        # the first and the last document of the range, and both
    cand[rng.random((Q, M)) < 0.03] = hi - 1                    # neighbours outside it
    cand[rng.random((Q, M)) < 0.02] = hi
    cand[rng.random((Q, M)) < 0.02] = lo - 1
    # cand_n: 0, 1, M, M + 5 in turn, then anything up to M (slots past cand_n hold documents that must not be counted)
    cn = rng.integers(0, M + 1, Q).astype(np.int32)
    cn[0::3] = np.resize(np.array([M, 0, 1, M + 5], np.int32), len(cn[0::3]))
    # one query (the last with all M slots) whose candidates all belong to ONE shard: whole blocks of 8 owned slots
    full = np.nonzero(cn >= M)[0]
    nonempty = np.nonzero(sizes > 0)[0]
    if len(full):
        s = int(nonempty[len(nonempty) // 2])
        cand[full[-1]] = rng.integers(bounds[s], bounds[s + 1], M)
    return dict(world=world, Q=Q, M=M, qps=(Q + world - 1) // world, bounds=bounds, cand=cand, cand_n=cn)


def owners(case):
    """int [Q, M]: the shard that owns each slot, -1 for nobody."""
    cand, cn, b = case["cand"].astype(np.int64), case["cand_n"].astype(np.int64), case["bounds"].astype(np.int64)
    M = cand.shape[1]
    live = (np.arange(M)[None, :] < np.minimum(cn, M)[:, None]) & (cand >= b[0]) & (cand < b[-1])
    own = (cand[:, :, None] >= b[None, None, :-1]) & (cand[:, :, None] < b[None, None, 1:])     # [Q, M, world]: at most one
    assert int(own.sum(axis=2).max(initial=0)) <= 1
    return np.where(live & own.any(axis=2), own.argmax(axis=2), -1)


def expected(case, my):
    """-> dict(counts [world, Q], send_base [Q], send_blk [Q, ceil(M / 8)], recv_off [world, qps], pair [world, world],
    lo, hi) for rank `my`; recv_off is defined for j < hi - lo only (zero elsewhere here)."""
    world, Q, M, qps = case["world"], case["Q"], case["M"], case["qps"]
    own = owners(case)
    counts = np.stack([(own == s).sum(axis=1) for s in range(world)]).astype(np.int64)
    send_base = np.concatenate([[0], np.cumsum(counts[my])[:-1]])
    n_blk = (M + 7) // 8
    mine = np.zeros((Q, n_blk * 8), np.int64)
    mine[:, :M] = own == my
    per_blk = mine.reshape(Q, n_blk, 8).sum(axis=2)
    send_blk = np.cumsum(per_blk, axis=1) - per_blk
    cut = lambda r: (min(Q, r * qps), min(Q, (r + 1) * qps))
    lo, hi = cut(my)
    flat = counts[:, lo:hi].reshape(-1)                         # (source, my query) in the order of the receive buffer
    recv_off = np.zeros((world, qps), np.int64)
    recv_off[:, :hi - lo] = (np.cumsum(flat) - flat).reshape(world, hi - lo)
    pair = np.array([[counts[s, cut(o)[0]:cut(o)[1]].sum() for o in range(world)] for s in range(world)], np.int64)
    i32 = lambda x: x.astype(np.int32)
    return dict(counts=i32(counts), send_base=i32(send_base), send_blk=i32(send_blk), recv_off=i32(recv_off), pair=i32(pair),
                per_blk=i32(per_blk), lo=lo, hi=hi)


def expected_by_loop(case, my):
    """The same, slot by slot in plain Python (small cases): records laid out one after the other, as a sender and a
    receiver would walk them."""
    world, Q, M, qps = case["world"], case["Q"], case["M"], case["qps"]
    cand, cn, b = case["cand"].tolist(), case["cand_n"].tolist(), case["bounds"].tolist()
    n_blk = (M + 7) // 8
    counts = [[0] * Q for _ in range(world)]
    send_base, send_blk = [0] * Q, [[0] * n_blk for _ in range(Q)]
    pair = [[0] * world for _ in range(world)]
    sent = 0
    for q in range(Q):
        send_base[q] = sent
        in_q = 0
        for m in range(M):
            if m % 8 == 0:
                send_blk[q][m // 8] = in_q
            if m >= cn[q]:
                continue
            d = cand[q][m]
            for s in range(world):
                if b[s] <= d < b[s + 1]:
                    counts[s][q] += 1
                    pair[s][q // qps] += 1
                    if s == my:
                        sent += 1
                        in_q += 1
    lo, hi = min(Q, my * qps), min(Q, (my + 1) * qps)
    recv_off, at = [[0] * qps for _ in range(world)], 0
    for s in range(world):
        for j in range(hi - lo):
            recv_off[s][j] = at
            at += counts[s][lo + j]
    a = lambda x: np.asarray(x, np.int32)
    return dict(counts=a(counts), send_base=a(send_base), send_blk=a(send_blk), recv_off=a(recv_off),
                pair=a(pair), lo=lo, hi=hi)
