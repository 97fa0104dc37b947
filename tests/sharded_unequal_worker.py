"""One rank of tests/test_gpu_multirank.py::test_three_ranks_with_unequal_engines_and_shards (started by torch.distributed.run;
gloo, every rank on cuda:0): real engines on shards cut by hand, built with different max_queries, and -- in the second
search -- one shard that cannot split the dense call at all.  Rank 0 compares with an unsharded engine and with the float64
reference and prints one JSON line."""
import json
import os
import sys
import time
from datetime import timedelta

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_DOCS, N_CHUNKS, N_TERMS, SEED, QSEED = 12000, 60000, 20000, 31, 32
CUTS = (0, 3480, 8280, 12000)                  # 29 % / 40 % / 31 % of the documents: >= 17 000 rows, >= 64 row tiles each
MAX_QUERIES = (512, 128, 256)                  # dense_split_max 512 / 128 / 256: the ranks agree on 128
Q, K1, K2 = 200, 50, 10
CHECKED = (0, 1, 63, 64, 127, 128, 150, 199)   # queries of the second search held to the float64 reference
LONG_DOC = 10000                               # the document of the last shard that gets 257 chunks in the second search
MIN_GAP = 2e-5


def corpus():
    from msretr.synthetic import synthetic_corpus, synthetic_queries
    ix = synthetic_corpus(N_DOCS, n_chunks=N_CHUNKS, n_terms=N_TERMS, seed=SEED)
    terms, qvec = synthetic_queries(ix, Q, seed=QSEED)
    return ix, terms, qvec


def with_long_document(ix):
    """The same rows and postings; document LONG_DOC takes 257 chunks, the documents behind it (same shard) give one each."""
    cnt = np.diff(ix.doc_off.numpy().astype(np.int64))
    need = 257 - int(cnt[LONG_DOC])
    give = [d for d in range(LONG_DOC + 1, N_DOCS) if cnt[d] > 1][:need]
    assert len(give) == need
    cnt[give] -= 1
    cnt[LONG_DOC] = 257
    off = np.zeros(N_DOCS + 1, np.int64)
    off[1:] = np.cumsum(cnt)
    assert off[-1] == N_CHUNKS and off[CUTS[2]] == int(ix.doc_off[CUTS[2]])
    import copy
    out = copy.copy(ix)
    out.doc_off = torch.as_tensor(off.astype(np.int32))
    out._url_group = None
    return out


def long_document_queries(ix2, qvec):
    """Two of the checked queries point at rows of the long document (its first and its last chunk)."""
    q = qvec.clone()
    r0 = int(ix2.doc_off[LONG_DOC])
    q[63] = ix2.emb[r0] * 7.0
    q[150] = (ix2.emb[r0 + 256] + 0.3 * ix2.emb[r0 + 100]) * 2.0
    return q


def reference_top(ix, qvec, k):
    """float64-pinned reference lists of the checked queries, one entry more than k (the gap behind the list counts)."""
    from oracle import dense_ref
    emb, off = ix.emb.numpy(), ix.doc_off.numpy().astype(np.int64)
    return {i: dense_ref.quick_search(emb, off, qvec[i].numpy(), k + 1) for i in CHECKED}


def cut(ix, rank):
    ix.shard_bounds = lambda world: np.asarray(CUTS, np.int64)      # (this instance only: the hand-made cut)
    return ix.shard(rank, len(CUTS) - 1)


def main():
    from msretr.distributed import ShardedEngine
    from msretr.engine import DeviceEngine
    dist.init_process_group("gloo", timeout=timedelta(seconds=60))
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 3
    t0 = time.time()
    ix, terms, qvec = corpus()
    ix2 = with_long_document(ix)
    q2 = long_document_queries(ix2, qvec)
    report = {}
    try:
        for phase, (full, qv) in enumerate(((ix, qvec), (ix2, q2))):
            sh = cut(full, rank)
            eng = DeviceEngine(sh, device=0, max_queries=MAX_QUERIES[rank], max_k=K1, rerank_max_docs=K1)
            own = eng.dense_split_max(K2)
            assert own == ((512, 128, 256)[rank] if phase == 0 or rank < 2 else 0), (phase, rank, own)
            se = ShardedEngine(eng, sh.doc_base, sh.row_base)
            out = se.search([sh.term_ids(t) for t in terms], qv, k1=K1, k2=K2)
            torch.cuda.synchronize()
            assert se._split[K2] == (128 if phase == 0 else 0) and se._bounds[0] is not None
            path = eng.dense_path()
            # phase 0: every rank in 128 + 72 through the streaming pass; phase 1: nobody splits, the rank with the long
            # document sweeps (64 queries per pass), the others take their own streaming pass
            assert path in ((128, 256) if phase == 0 or rank < 2 else (64, 32)), (phase, rank, path)
            if rank == 0:
                ref_eng = DeviceEngine(full, device=0, max_queries=512, max_k=K1, rerank_max_docs=K1)
                ref = ShardedEngine(ref_eng, 0, 0)
                ref.world = 1                                       # no collectives: the single-engine reference
                exp = ref.search([full.term_ids(t) for t in terms], qv, k1=K1, k2=K2)
                ref_path = ref_eng.dense_path()
                assert ref_path in ((128, 256) if phase == 0 else (64, 32)), (phase, ref_path)
                for key in ("bm25", "rerank") + (("dense",) if phase == 0 else ()):
                    for j, (a, b) in enumerate(zip(out[key], exp[key])):
                        assert a.shape == b.shape and a.dtype == b.dtype, (phase, key, j)
                        bits = torch.int32 if a.element_size() == 4 else torch.int64
                        assert torch.equal(a.view(bits), b.view(bits)), f"search {phase}: sharded != unsharded for {key}[{j}]"
                if phase == 1:
                    top = reference_top(full, qv, K2)
                    d_doc, d_score, d_chunk, d_n = [x.cpu().numpy() for x in out["dense"]]
                    worst = 0.0
                    for i, (oi, osc, oa) in top.items():
                        assert np.all(-np.diff(osc.astype(np.float64)) >= MIN_GAP), ("reference scores too close", i)
                        assert d_n[i] == K2
                        err = float(np.abs(d_score[i].astype(np.float64) - osc[:K2]).max())
                        worst = max(worst, err)
                        assert err <= 1e-5, (i, err)
                        assert d_doc[i].tolist() == oi[:K2].tolist(), i       # (gaps >= 2e-5, errors <= 1e-5: the order is the reference's)
                    assert d_doc[63, 0] == LONG_DOC and d_doc[150, 0] == LONG_DOC
                    report["dense_max_err"] = worst
                ref_eng.close()
                report[f"paths{phase}"] = [path, ref_path]
            eng.close()
            dist.barrier()
        if rank == 0:
            report.update(ok=True, seconds=round(time.time() - t0, 2))
            print(json.dumps(report), flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
