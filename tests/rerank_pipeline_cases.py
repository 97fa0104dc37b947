"""Inputs for tests/test_gpu_rerank_pipeline.py and tools/record_rerank_gather.py.

TEST INFRASTRUCTURE ONLY, CPU, deterministic (numpy).

`recorded_runs` lists the gather calls whose output bits tests/golden/rerank_gather_parent.npz holds, recorded from the
gather BEFORE its row pipeline: the corpus of rerank_cases.gather_corpus(), layouts 0 and 1, max_chunks 10 and 3, 1, 3 and
17 queries per call (1 and 3: one wave per slot; 17: a wave per 8 slots), a shard with a document and a row base, and the
record form on a two-shard split.  `run_recorded` makes those calls on engines the caller supplies, so the recorder and
the test cannot drift apart.  Most lists are short: the file holds every word the gather writes and has to stay small.

`edge_corpus` is hand-built for the edges a flat row pipeline over a block of 8 slots creates.
"""
import numpy as np

import rerank_cases as RC

SHARD = (400, 1100)                 # the shard tests/test_gpu_rerank.py uses
RECORD_CUT = 700                    # records: shards [0, 700) and [700, N)
RECORD_Q = 6


def recorded_inputs(z):
    """-> (queries [17, 768], cand [17, M], cand_n [17])"""
    rng = np.random.default_rng(77)
    Q = 17
    qsel = np.concatenate([np.arange(8), rng.integers(0, 8, Q - 8)])
    cand, _ = RC.candidates(rng, z["N"], Q)
    n = rng.integers(1, 120, Q).astype(np.int32)
    n[0], n[5], n[11], n[13] = 150, RC.M, 5000, 0
    cand[0, :7] = np.arange(7)                                   # the special documents, the corpus' first row
    cand[1, :3] = (z["N"] - 1, 0, 6)                             # its last row
    cand[2, 9] = -1                                              # a padding slot in the middle of a list
    return z["queries"][qsel].copy(), cand, n


def recorded_runs():
    return [(layout, mc, Q) for layout in (0, 1) for mc in (10, 3) for Q in (1, 3, 17)]


def run_recorded(z, engine, plan_cls, torch):
    """engine(layout, d0, d1) -> a DeviceEngine over documents [d0, d1) of z (d1 None: to the end) -> {name: array}"""
    q, cand, n = recorded_inputs(z)
    np_ = lambda t: t.detach().cpu().numpy()
    out = {}
    for layout, mc, Q in recorded_runs():
        cos, meta = engine(layout, 0, None).rerank_gather(q[:Q], cand[:Q], n[:Q], max_chunks=mc)
        out[f"cos_l{layout}_c{mc}_q{Q}"], out[f"meta_l{layout}_c{mc}_q{Q}"] = np_(cos).view(np.int32), np_(meta)
    d0, d1 = SHARD
    cos, meta = engine(0, d0, d1).rerank_gather(q, cand, n, doc_base=d0, row_base=int(z["doc_off"][d0]), max_chunks=10)
    out["cos_shard"], out["meta_shard"] = np_(cos).view(np.int32), np_(meta)
    # the record form: two shards, every query of the call in one launch
    bounds = np.array([0, RECORD_CUT, z["N"]], np.int32)
    Q, Qs = RECORD_Q, RECORD_Q // 2
    dev = engine(0, 0, RECORD_CUT).device
    cand_t, n_t = torch.as_tensor(cand[:Q]).to(dev), torch.as_tensor(n[:Q]).to(dev)
    for r in range(2):
        e = engine(0, int(bounds[r]), int(bounds[r + 1]))
        plan = plan_cls(2, Q, Qs, RC.M, dev)
        e.rerank_plan(cand_t, n_t, torch.as_tensor(bounds).to(dev), r, Qs, plan)
        rec = torch.full((Q * RC.M * 16,), -7, dtype=torch.int32, device=dev)
        e.rerank_gather_records(q[:Q], cand_t, n_t, plan, rec, doc_base=int(bounds[r]),
                                row_base=int(z["doc_off"][bounds[r]]), max_chunks=10)
        total = int(np_(plan.pair)[r].sum())
        rec = np_(rec).reshape(-1, 16)
        assert (rec[total:] == -7).all()
        out[f"records_{r}"] = rec[:total].copy()
    return out


# ------------------------------------------------------------------ the pipeline's edges
EDGE_ROWS = [0, 1, 2, 3, 9, 10, 11, 25,          # documents 0 .. 7
             0, 0, 0, 0, 0, 0, 0, 0,             # 8 .. 15: a block of 8 slots without a row
             10, 10, 10, 10, 10, 10, 10, 10,     # 16 .. 23: a block of 80 rows
             4, 7, 1, 5, 2, 6, 3, 8,             # 24 .. 31
             12, 1, 0, 30, 2, 10, 9, 11, 5]      # 32 .. 40; document 40 ends at the matrix's last row


def edge_corpus(seed=9):
    """-> dict(emb [C, 768] f32 with UNIT rows in the sense the test needs: every row's inv_norm is bound as given,
    doc_off, url_group, N, C, queries [4, 768] unit f32)."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(EDGE_ROWS)]).astype(np.int32)
    C, N = int(off[-1]), len(EDGE_ROWS)
    emb = (rng.standard_normal((C, RC.DIM)) * rng.uniform(0.5, 2.0, (C, 1))).astype(np.float32)
    # unit queries whose normalisation on the device is exact whatever its summation order: 624 components of +-1/32 and
    # 100 of +-1/16 (624 / 1024 + 100 / 256 = 1, every partial sum of squares a multiple of 2^-10), 44 zeros
    mag = np.array([1 / 32] * 624 + [1 / 16] * 100 + [0.0] * 44, np.float32)
    q = np.stack([rng.permutation(mag) * rng.choice(np.float32([-1, 1]), RC.DIM) for _ in range(4)]).astype(np.float32)
    grp = (np.arange(N, dtype=np.int32) * 3) % 11
    grp[5] = -1
    return dict(emb=emb, doc_off=off, url_group=grp, N=N, C=C, queries=q)


def edge_lists(N):
    """-> (cand [Q, M], cand_n [Q], note per query).  Slots come in blocks of 8: the blocks below are laid out by hand."""
    M = RC.M
    lists = []

    def add(docs, n=None, note=""):
        row = np.full(M, -1, np.int32)
        row[:len(docs)] = docs
        lists.append((row, len(docs) if n is None else n, note))

    add([], note="no candidate")
    add([7], note="one candidate, 10 of its 25 rows")
    add([2, 1, 0, 3, 9, 4, 5], note="7 slots")
    add([0, 1, 2, 3, 4, 5, 6, 7], note="8 slots: one block, rows 0 1 2 3 9 10 10 10")
    add([40, 6, 5, 4, 3, 2, 1, 0, 39], note="9 slots: the matrix's last row first; a one-slot second block")
    add(list(range(8, 16)) + [1] + [8] * 7 + [9, 10, 1, 11, 12, 13, 14, 15],
        note="a block without rows, blocks of exactly one row (first slot; third slot)")
    add(list(range(16, 24)) + [35, 19, 37, 20, 21, 22, 23, 16], note="blocks of 80 rows")
    add([3, -1, 4, -1, -1, 5, N, N + 7, 40, -3, 7], note="padding -1 and foreign documents inside a list")
    add([20, 33, 21, 34, 0, 22, 8, 23] * 2, note="rowless documents between full ones")
    rng = np.random.default_rng(4)
    add(rng.integers(0, N, 1000).tolist(), note="1000 candidates")
    add(rng.integers(-1, N + 2, M).tolist(), n=4000, note="cand_n above M")
    # slots of another shard interleaved with owned ones: owned by [0, 24) or by [24, N) alternately
    add([x for a, b in zip(range(0, 24), list(range(24, N)) + [24] * 7) for x in (a, b)], note="alternating owners")
    cand = np.stack([r for r, _, _ in lists])
    n = np.array([k for _, k, _ in lists], np.int32)
    # junk behind cand_n: the gather must not read it as a candidate
    for i, k in enumerate(n):
        if k < M:
            cand[i, max(k, 0):] = rng.integers(0, N, M - max(k, 0))
    return cand, n, [t for _, _, t in lists]


def lane_order_cos(q_unit, E, inv):
    """The gather's f32 arithmetic restated: lane l holds float4 number l, l + 64, l + 128 of the row; 12 products summed in
    the kernel's grouping ((p0 + p1) + p2) + p3 per float4, the three float4 sums added in order, then the butterfly
    s += shfl_xor(s, o) for o = 32 .. 1 (every lane ends with the same sum), one multiply by inv_norm.  q_unit [768],
    E [R, 768], inv [R], all float32 -> [R] float32."""
    E = np.asarray(E, np.float32)
    p = (E * np.asarray(q_unit, np.float32)[None, :]).reshape(len(E), 3, 64, 4)          # [row, k, lane, component]
    g = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]                                 # [row, k, lane]
    s = (g[:, 0] + g[:, 1]) + g[:, 2]                                                      # [row, lane]
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ o]
    assert (s == s[:, :1]).all()
    return (s[:, 0] * np.asarray(inv, np.float32)).astype(np.float32)
