"""Record the rerank gather's output bits (tests/golden/rerank_gather_parent.npz) for tests/test_gpu_rerank_pipeline.py.

Run it on the commit whose gather is the yardstick -- the parent of the row pipeline -- on the GPU box:
    python tools/record_rerank_gather.py [OUT.npz]
The calls are the ones of tests/rerank_pipeline_cases.run_recorded; the file is the project's own output."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import rerank_cases as RC
import rerank_pipeline_cases as PC
from msretr.distributed import _RerankPlan
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(RC.GOLDEN, "rerank_gather_parent.npz")
z = RC.gather_corpus()
engines = {}


def engine(layout, d0, d1):
    key = (layout, d0, d1)
    if key not in engines:
        e1 = z["N"] if d1 is None else d1
        r0, r1 = int(z["doc_off"][d0]), int(z["doc_off"][e1])
        ix = CorpusIndex(doc_ids=np.arange(d0, e1, dtype=np.int64), doc_off=(z["doc_off"][d0:e1 + 1] - z["doc_off"][d0]).astype(np.int32),
                         chunk_ids=np.arange(r0, r1, dtype=np.int64), emb=z["emb"][r0:r1], total_docs=z["N"], doc_base=d0,
                         row_base=r0, _url_group=z["url_group"][d0:e1].copy())
        engines[key] = DeviceEngine(ix, device=0, max_queries=32, max_k=100, rerank_max_docs=RC.M, scan_layout=layout)
    return engines[key]


arrays = PC.run_recorded(z, engine, _RerankPlan, torch)
torch.cuda.synchronize()
for e in engines.values():
    e.close()
np.savez_compressed(out_path, **arrays)
size = os.path.getsize(out_path)
print(f"{out_path}: {len(arrays)} arrays, {size} bytes")
assert size < 1 << 20, "the fixture must stay under 1 MiB"
