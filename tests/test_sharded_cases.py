"""The exchange-plan cases of tests/sharded_cases.py, checked without a GPU: the numpy restatement against a slot-by-slot loop,
the gloo tests' stand-in against both, and that every edge the cases are for is really in them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sharded_cases as sc  # noqa: E402

FIELDS = ("counts", "send_base", "send_blk", "recv_off", "pair")


@pytest.mark.parametrize("c", sc.SMALL, ids=sc.case_id)
def test_restatement_equals_the_slot_loop(c):
    case = sc.make_case(*c)
    for my in range(case["world"]):
        got, ref = sc.expected(case, my), sc.expected_by_loop(case, my)
        assert (got["lo"], got["hi"]) == (ref["lo"], ref["hi"])
        for f in FIELDS:
            assert got[f].shape == ref[f].shape and got[f].dtype == np.int32 and np.array_equal(got[f], ref[f]), (my, f)


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_plan_is_consistent(c):
    """What any plan must satisfy, at every size: each live slot inside the bounds has exactly one owner; the send buffer is
    the queries one after the other; the receive buffer is the (source, query) blocks one after the other; the matrix agrees
    with both ends."""
    case = sc.make_case(*c)
    world, Q, M, qps = case["world"], case["Q"], case["M"], case["qps"]
    assert sc.make_case(*c)["cand"].tobytes() == case["cand"].tobytes()                      # the generator is deterministic
    own = sc.owners(case)
    b = case["bounds"].astype(np.int64)
    live = (np.arange(M)[None, :] < case["cand_n"][:, None]) & (case["cand"] >= b[0]) & (case["cand"] < b[-1])
    assert np.array_equal(own >= 0, live)
    assert not np.isin(own[own >= 0], np.nonzero(np.diff(b) == 0)[0]).any()                  # an empty shard owns nothing
    for my in sorted({0, world // 2, world - 1}):
        e = sc.expected(case, my)
        assert int(e["counts"].sum()) == int(live.sum())
        total = int(e["counts"][my].sum())
        assert np.array_equal(e["send_base"][1:], np.cumsum(e["counts"][my])[:-1]) and (Q == 0 or e["send_base"][0] == 0)
        assert np.array_equal(e["send_blk"][:, 0], np.zeros(Q)) and np.array_equal(e["per_blk"].sum(axis=1), e["counts"][my])
        assert int(e["pair"][my].sum()) == total and np.array_equal(e["pair"].sum(axis=1), e["counts"].sum(axis=1))
        n = e["hi"] - e["lo"]
        if n:
            ends = e["recv_off"][:, :n] + e["counts"][:, e["lo"]:e["hi"]]
            flat_first, flat_end = e["recv_off"][:, :n].reshape(-1), ends.reshape(-1)
            assert flat_first[0] == 0 and np.array_equal(flat_first[1:], flat_end[:-1])
            assert int(flat_end[-1]) == int(e["pair"][:, my].sum())
            # source s' block of the receive buffer starts where the all-to-all puts it
            assert np.array_equal(e["recv_off"][:, 0], np.cumsum(e["pair"][:, my]) - e["pair"][:, my])
        else:
            assert int(e["pair"][:, my].sum()) == 0


def test_the_cases_hold_their_edges():
    seen = set()
    for c in sc.CASES:
        case = sc.make_case(*c)
        world, Q, M, qps = case["world"], case["Q"], case["M"], case["qps"]
        b, cand, cn = case["bounds"].astype(np.int64), case["cand"].astype(np.int64), case["cand_n"]
        sizes = np.diff(b)
        assert b[0] > 0 and (sizes >= 0).all()
        seen.add("bounds[0] > 0")
        if world >= 3 and (sizes[1:-1] == 0).any():
            seen.add("empty shard in the middle")
        if world >= 2 and sizes[-1] == 0:
            seen.add("empty last shard")
        if (world - 1) * qps >= Q:
            seen.add("rank without queries")
        if Q > 1024:
            seen.add("Q > 1024")
        if qps > 1024:
            seen.add("queries_per_shard > 1024")
        if M < 8:
            seen.add("M < 8")
        if M == 1024:
            seen.add("M == 1024")
        for v, name in ((0, "cand_n == 0"), (1, "cand_n == 1"), (M, "cand_n == M"), (M + 5, "cand_n > M")):
            if (cn == v).any():
                seen.add(name)
        inside = np.arange(M)[None, :] < np.minimum(cn, M)[:, None]
        for mask, name in ((cand == -1, "candidate -1"), ((cand >= 0) & (cand < b[0]), "candidate below bounds[0]"),
                           (cand >= b[-1], "candidate at or above bounds[-1]"), (cand == b[0], "first document"),
                           (cand == b[-1] - 1, "last document")):
            if (mask & inside).any():
                seen.add(name)
        own = sc.owners(case)
        one = [(own[q] == own[q, 0]).all() and own[q, 0] >= 0 for q in range(Q) if cn[q] >= M]
        if any(one) and M > 1:
            seen.add("a query owned by one shard")
        pad = np.full((Q, (M + 7) // 8 * 8), -1)
        pad[:, :M] = own
        for my in range(world):
            per_blk = (pad == my).reshape(Q, -1, 8).sum(axis=2)
            if (per_blk == 0).any():
                seen.add("block of 0 owned slots")
            if (per_blk == 8).any():
                seen.add("block of 8 owned slots")
    missing = {"bounds[0] > 0", "empty shard in the middle", "empty last shard", "rank without queries", "Q > 1024",
               "queries_per_shard > 1024", "M < 8", "M == 1024", "cand_n == 0", "cand_n == 1", "cand_n == M", "cand_n > M",
               "candidate -1", "candidate below bounds[0]", "candidate at or above bounds[-1]", "first document", "last document",
               "a query owned by one shard", "block of 0 owned slots", "block of 8 owned slots"} - seen
    assert not missing, missing


@pytest.mark.parametrize("c", sc.SMALL[:4], ids=sc.case_id)
def test_the_gloo_stand_in_plans_the_same(c):
    """OracleEngine.rerank_plan (what tests/test_sharded_gloo.py runs the exchange with) against the restatement."""
    import torch
    from msretr.distributed import _RerankPlan
    from oracle_engine import OracleEngine
    case = sc.make_case(*c)
    world, Q, M, qps = case["world"], case["Q"], case["M"], case["qps"]
    for my in range(world):
        plan = _RerankPlan(world, Q, qps, M, "cpu")
        OracleEngine.rerank_plan(None, torch.as_tensor(case["cand"]), torch.as_tensor(case["cand_n"]),
                                 torch.as_tensor(case["bounds"]), my, qps, plan)
        e = sc.expected(case, my)
        n = e["hi"] - e["lo"]
        for f in FIELDS:
            got = getattr(plan, f).numpy()
            if f == "recv_off":
                assert np.array_equal(got[:, :n], e[f][:, :n]), (my, f)
            else:
                assert np.array_equal(got, e[f]), (my, f)
