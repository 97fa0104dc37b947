"""bench.py prints ONE JSON line with the fields the driver reads (metric / value / unit / n_gpus / steps / warmup /
ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload) plus the `roofline` object; with
--full also the single-query latency, the variants, the drop-in API and the `cpu_baseline` object with the parity of the
GPU path against it; checked here on a small corpus so that a contract break shows up as a test failure."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what a plain run leaves to --full: each of these takes runs of its own
FULL_ONLY = ("p50_latency_ms_single_query", "variant_bf16_candidates", "roofline_exact_f32", "variant_with_encoder", "facade",
             "cpu_baseline", "vs_cpu_baseline", "bm25_parity_vs_cpu", "dense_parity_vs_cpu", "rerank_parity_vs_cpu")


def _run(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--docs", "60000",
           "--chunks", "250000", "--terms", "50000", "--latency-queries", "2", "--cpu-queries", "2", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _check_contract_fields(d):
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "queries/sec" and d["value"] > 0 and d["ms_per_step"] > 0 and d["data"] == "synthetic"
    assert abs(d["value"] - d["config"]["queries_per_step"] * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["config"]["queries_per_step"] == 256
    assert "model" not in d["config"] and d["config"]["workload"].startswith("hybrid: 60000 docs")
    assert "f64" in d["dtype"] and d["outputs_sane"] is True
    r = d["roofline"]
    # 256 queries per step: ONE pass of the 256-query streaming kernel over the f32 rows (csrc/msr_gemm_f32.hip) per step
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["kernel"] == "gemm_stream256_kernel<emit>"
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and "traffic" in r and r["launches"] == 3   # 1 pass x 3 steps
    assert r["bm25_taat"]["launches"] == 3


def test_plain_line_has_the_contract_fields():
    """A plain run: the headline fields and the roofline of its timed steps, nothing that takes runs of its own."""
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    d = _run()
    _check_contract_fields(d)
    assert [k for k in FULL_ONLY if k in d] == []


def test_full_line_has_the_contract_fields():
    """A --full run: the same fields and roofline, plus the latency, the CPU baseline, the parity against it and the variants."""
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    d = _run("--full")
    _check_contract_fields(d)
    assert d["p50_latency_ms_single_query"] > 0 and d["bm25_parity_vs_cpu"] is True
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "queries/sec" and c["sample"]
    for leg in ("port", "vectorised", "literal"):          # three legs, p50 per query, cores stated
        assert c[leg]["p50_ms"] > 0 and c[leg]["value"] > 0 and c[leg]["cores"] >= 1 and c[leg]["queries"] == 2, leg
    assert c["literal"]["cores"] == 1 and c["p50_ms"] == c["port"]["p50_ms"]
    # dense parity against the CPU restatement is reported with every --full benchmark line
    p = d["dense_parity_vs_cpu"]
    assert p["queries"] == 2 and p["k"] == 100 and p["within_1e-5"] is True and p["max_abs_score_diff"] <= 1e-5
    assert p["top_k_doc_sets_equal_up_to_boundary_near_ties"] is True and p["same_doc_at_same_rank"] > 0.95
    assert abs(d["vs_cpu_baseline"] - d["value"] / c["value"]) <= 1e-9 * d["vs_cpu_baseline"]
    e = d["variant_with_encoder"]                             # query path from token ids (search_api.py:69-152 in one number)
    assert e["value"] > 0 and e["encoder_ms_per_batch"] > 0 and e["outputs_sane"] is True and e["queries_per_step"] == 256
    v = d["variant_bf16_candidates"]
    assert v["value"] > 0 and v["top100_equals_default_path_within_2e-6"] is True


def test_exact_f32_line_reports_the_matrix_core_roofline():
    d = _run("--scan-variant", "2", "--no-cpu-baseline", "--no-variants")
    assert d["dtype"].startswith("f32 (dense cosine)") and "cpu_baseline" not in d and "variant_bf16_candidates" not in d
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 157.3 and 0 < r["frac"] < 1


def test_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    """--dump-outputs DIR: the arrays the last timed step returned, float32 / float64, every value finite (BM25 lists shorter than
    k1 are padded: those slots' scores are written as 0), at most 64 MB, identical in two runs with
    the same arguments (the inputs are seeded); --steps is the number of timed steps (one pass of each kernel per step)."""
    import numpy as np
    runs = []
    for name in ("a", "b"):
        d = _run("--steps", "2", "--no-cpu-baseline", "--no-variants", "--dump-outputs", str(tmp_path / name))
        assert d["steps"] == 2 and d["roofline"]["launches"] == 2 and d["roofline"]["bm25_taat"]["launches"] == 2
        assert d["outputs_sane"] is True
        runs.append({p.stem: np.load(p) for p in sorted((tmp_path / name).glob("*.npy"))})
    a, b = runs
    assert sorted(a) == sorted(["query_index", "bm25_doc", "bm25_score", "bm25_n", "dense_doc", "dense_score", "dense_chunk",
                                "dense_n", "rerank_doc", "rerank_score", "rerank_orig", "rerank_chunk", "rerank_n", "rerank_rows"])
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64 << 20
    assert np.array_equal(a["query_index"], np.arange(256))
    assert a["bm25_doc"].shape == (256, 1000) and a["dense_doc"].shape == (256, 100) and a["rerank_doc"].shape == (256, 1000)
    assert a["dense_score"].dtype == np.float32 and a["bm25_score"].dtype == np.float64 and np.all(a["dense_n"] == 100)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.isfinite(a[k]).all(), k
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
