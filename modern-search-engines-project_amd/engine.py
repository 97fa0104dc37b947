"""DeviceEngine: the index resident in HBM + the libmsretr handle.

PyTorch is plumbing here: it owns the device allocations and the stream; every computation on the path is
a HIP kernel in csrc/ reached through the C ABI (include/msretr.h).  There is no fallback: without a GPU
or without the built library, construction raises.
"""
import ctypes as C
import threading

import numpy as np
import torch

from . import _abi
from .index import DIM, CorpusIndex

RERANK_DEFAULTS = dict(smoothing=0.15, max_boost=0.1, max_decay=0.05, max_chunks=10)   # reranker/config.yaml:28,
#                                                                                        reranker_api.py:58,317-318


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def count_nonzero_words(t, n_words=None):
    """Test-only (msr_debug_count_nonzero, no engine): the number of non-zero 32-bit words among the first n_words (default:
    all) of the contiguous device tensor t, counted by their bits (-0.0 counts).  Synchronises."""
    assert t.is_cuda and t.is_contiguous() and (t.numel() * t.element_size()) % 4 == 0
    n = t.numel() * t.element_size() // 4 if n_words is None else int(n_words)
    out = torch.empty((1,), dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        rc = _abi.load().msr_debug_count_nonzero(_ptr(t) if t.numel() else C.c_void_p(0), n, _ptr(out),
                                                 C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream))
    _abi.check(None, rc)
    return int(out.item())


STREAM_MIN_BYTES = 64 << 20
_NP_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64,
          torch.int16: np.int16}


def stream_to_device(arr, device, block_bytes=128 << 20):
    """numpy array (typically a read-only memory map of a snapshot file, index.CorpusIndex.load_dir) -> device tensor,
    block by block through two pinned staging buffers: while block i travels to HBM (async copy on the current
    stream) block i + 1 is read from the file into the other buffer.  The host never holds more than two blocks."""
    dev = torch.device(device)
    out = torch.empty(arr.shape, dtype=torch.from_numpy(np.empty(0, arr.dtype)).dtype, device=dev)
    if arr.size == 0:
        return out
    flat_out = out.view(-1)
    row = int(np.prod(arr.shape[1:], dtype=np.int64)) if arr.ndim > 1 else 1
    rows_per_block = max(1, block_bytes // max(1, row * arr.itemsize))
    pinned = dev.type == "cuda"
    stage = [torch.empty(rows_per_block * row, dtype=out.dtype, pin_memory=pinned) for _ in range(2)]
    done = [None, None]
    for b, r0 in enumerate(range(0, arr.shape[0], rows_per_block)):
        r1 = min(arr.shape[0], r0 + rows_per_block)
        buf = stage[b & 1]
        if done[b & 1] is not None:
            done[b & 1].synchronize()                    # the copy that last used this buffer has finished
        n = (r1 - r0) * row
        np.copyto(buf.numpy()[:n].reshape((r1 - r0,) + tuple(arr.shape[1:])), arr[r0:r1])
        flat_out[r0 * row:r0 * row + n].copy_(buf[:n], non_blocking=pinned)
        if pinned:
            done[b & 1] = torch.cuda.Event()
            done[b & 1].record(torch.cuda.current_stream(dev))
    if pinned:
        torch.cuda.current_stream(dev).synchronize()
    return out


class DeviceEngine:
    """Single-threaded: its methods take no lock.  `lock` (an RLock that lives as long as the engine, rebind included) is what
    the facades hold for a whole request (serial.py)."""

    def __init__(self, index: CorpusIndex, device=0, max_queries=32, max_k=1000, rerank_max_docs=1000,
                 scan_layout=0, scan_variant=0, row_copy=True, single_emit=False):
        """row_copy=False: MSR_CFG_NO_ROW_COPY -- the 256-query pass reads the row-major matrix instead of an engine-owned
        fragment-order copy of it (half the embedding footprint, a slower pass, the same results).
        single_emit=True: MSR_CFG_SINGLE_EMIT -- the streaming pass emits in one launch per query group with the sample's
        thresholds (the reference form of the segmented pass: the same results, more entries; dense_pass_info())."""
        if not torch.cuda.is_available():
            raise _abi.MsrError(-102, "no GPU visible: the retrieval path runs on MI355X only (no CPU fallback)")
        self.lib = _abi.load()
        self.lock = threading.RLock()
        self.index = index
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.max_k = int(max_k)
        self.max_queries = int(max_queries)
        self.scan_layout = int(scan_layout)
        self.rerank_max_docs = int(rerank_max_docs)
        cfg = _abi.MsrConfig(C.sizeof(_abi.MsrConfig), self.device.index or 0, DIM, int(max_queries), int(max_k),
                             int(rerank_max_docs), int(scan_layout), int(scan_variant),
                             (0 if row_copy else _abi.MSR_CFG_NO_ROW_COPY) | (_abi.MSR_CFG_SINGLE_EMIT if single_emit else 0))
        self.handle = C.c_void_p()
        rc = self.lib.msr_create(C.byref(cfg), C.byref(self.handle))
        if rc != 0:
            raise _abi.MsrError(rc, (self.lib.msr_last_error(None) or b"?").decode())
        self._t = {}          # device tensors that the engine borrows: keep them alive
        self._bf16 = False    # enable_bf16 was called: a rebind rebuilds the image
        self._bind(index)

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, x, dtype):
        if x is None:
            return None
        if torch.is_tensor(x):
            return x.to(device=self.device, dtype=dtype).contiguous()
        if isinstance(x, np.ndarray) and x.nbytes >= STREAM_MIN_BYTES and x.dtype == _NP_OF[dtype]:
            return stream_to_device(x, self.device)      # large (memory-mapped) arrays: pinned double buffer
        x = np.ascontiguousarray(x)
        if not x.flags.writeable:                            # small read-only memory maps: torch wants a writable source
            x = x.copy()
        return torch.as_tensor(x).to(device=self.device, dtype=dtype)

    def _check(self, rc):
        _abi.check(self.handle, rc)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            torch.cuda.synchronize(self.device)
            self.lib.msr_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _bind(self, ix):
        t = self._t
        with torch.cuda.device(self.device):
            if ix.term_off is not None and ix.n_terms > 0:
                t["term_off"] = self._dev(ix.term_off, torch.int64)
                t["post_doc"] = self._dev(ix.post_doc, torch.int32)
                t["post_tf"] = self._dev(ix.post_tf, torch.int32)
                t["doc_len"] = self._dev(ix.doc_len, torch.int32)
                t["idf"] = self._dev(ix.idf, torch.float32)
                self._check(self.lib.msr_bind_postings(
                    self.handle, _ptr(t["term_off"]), ix.n_terms, _ptr(t["post_doc"]), _ptr(t["post_tf"]),
                    int(t["post_doc"].numel()), _ptr(t["doc_len"]), ix.n_docs, _ptr(t["idf"]),
                    C.c_float(ix.avgdl), C.c_double(ix.k1), C.c_double(ix.b), self._stream()))
                if ix.tok_off is not None:                   # the forward index (phrase search, msr_bind_tokens)
                    tok_off, tok_ids = self._dev(ix.tok_off, torch.int64), self._dev(ix.tok_ids, torch.int32)
                    self._check(self.lib.msr_bind_tokens(self.handle, _ptr(tok_off), _ptr(tok_ids) if tok_ids.numel() else
                                                         C.c_void_p(0), ix.n_docs, int(tok_ids.numel()), self._stream()))
                    t["tok_off"], t["tok_ids"] = tok_off, tok_ids
                if ix.vocab:                                 # the term strings (typo-tolerant lookup, msr_bind_vocab)
                    char_off, chars, weight = ix.vocab_image()
                    v_off, v_w = self._dev(char_off, torch.int64), self._dev(weight.view(np.int32), torch.int32)
                    v_chars = self._dev(chars.view(np.int16), torch.int16)
                    self._check(self.lib.msr_bind_vocab(self.handle, _ptr(v_off), _ptr(v_chars) if v_chars.numel() else
                                                        C.c_void_p(0), _ptr(v_w), ix.n_terms, int(v_chars.numel()),
                                                        self._stream()))
                    t["voc_off"], t["voc_chars"], t["voc_weight"] = v_off, v_chars, v_w
            if ix.doc_off is not None and ix.emb is not None:
                t["doc_off"] = self._dev(ix.doc_off, torch.int32)
                emb = self._dev(ix.emb, torch.float32)
                n_chunks = int(emb.shape[0])
                inv = None
                if self.scan_layout == 1:
                    nrm = torch.linalg.vector_norm(emb, dim=1)
                    inv = (1.0 / torch.where(nrm == 0, torch.ones_like(nrm), nrm)).contiguous()
                    pad = (n_chunks + 15) // 16 * 16
                    tiled = torch.empty((pad, DIM), dtype=torch.float32, device=self.device)
                    self._check(self.lib.msr_interleave_rows(self.handle, _ptr(emb), n_chunks, _ptr(tiled), self._stream()))
                    torch.cuda.synchronize(self.device)
                    del emb
                    emb = tiled
                t["emb"], t["inv_norm"] = emb, inv
                self._check(self.lib.msr_bind_chunks(self.handle, _ptr(emb), n_chunks, _ptr(t["doc_off"]),
                                                     ix.n_docs, _ptr(inv), self._stream()))
                t["url_group"] = self._dev(ix.url_group(), torch.int32)
                self._check(self.lib.msr_bind_doc_meta(self.handle, _ptr(t["url_group"]), ix.n_docs, self._stream()))
            torch.cuda.synchronize(self.device)

    def rebind(self, ix: CorpusIndex):
        """Serve another index (e.g. index_build.bm25_add_token_ids(self.index, ...)) with this engine: synchronise, drop the
        old binding (msr_unbind: tables, copies, a pending dense_begin), bind `ix` -- any number of documents -- and rebuild
        the bf16 image if it was enabled.  The old index's device copies are released before the new ones are made.  If a
        bind fails the engine is left unbound (every call raises MSR_ERR_NOT_BOUND) and the error is raised."""
        torch.cuda.synchronize(self.device)
        self._check(self.lib.msr_unbind(self.handle))
        self._t = {}
        self.index = ix
        try:
            self._bind(ix)
            if self._bf16:
                self.enable_bf16()
        except Exception:
            torch.cuda.synchronize(self.device)
            self.lib.msr_unbind(self.handle)
            self._t = {}
            raise

    @property
    def has_tokens(self):
        """True if the bound index came with a forward index (CorpusIndex.tok_off / tok_ids): phrase_sets works."""
        return "tok_off" in self._t

    @property
    def has_vocab(self):
        """True if the bound index came with its term strings (CorpusIndex.vocab): fuzzy_terms and wildcard_terms work."""
        return "voc_off" in self._t

    def fuzzy_terms(self, words, max_edits=None, limit=1):
        """The vocabulary terms nearest to each word (msr_fuzzy_terms, DESIGN K15) -> per word ([(term id, distance), ...],
        total): the first `limit` (1 .. 16) candidates -- terms with a document frequency above 0 within the word's tolerance
        by optimal string alignment distance (insertion, deletion, substitution, swap of two adjacent code points), ordered by
        distance, then document frequency descending, then term id -- and the number of all candidates.  max_edits: None (the
        AUTO rule per word, fuzzy.auto_edits), an int for every word or one per word, each 0 .. 2.  A word that cannot be
        looked up (empty, more than 32 code points, a code point above 0xFFFE) gets ([], 0).  ONE upload, two launches, one
        copy back for up to MSR_FUZZY_MAX_WORDS words; longer lists go in slices.  Raises MsrError without a vocabulary."""
        from .fuzzy import auto_edits, encode_words, lookable
        if not self.has_vocab:
            raise _abi.MsrError(-2, "fuzzy_terms: the index has no vocabulary (CorpusIndex.vocab: term strings); a term-id-only "
                                    "index cannot suggest words")
        limit = int(limit)
        if not 1 <= limit <= _abi.MSR_FUZZY_MAX_LIMIT:
            raise ValueError(f"fuzzy_terms: limit must be 1 .. MSR_FUZZY_MAX_LIMIT = {_abi.MSR_FUZZY_MAX_LIMIT} (got {limit})")
        words = list(words)
        W = len(words)
        if max_edits is None:
            maxes = [auto_edits(len(w)) if isinstance(w, str) else 0 for w in words]
        else:
            maxes = [int(max_edits)] * W if np.ndim(max_edits) == 0 else [int(v) for v in max_edits]
            if len(maxes) != W or any(not 0 <= m <= 2 for m in maxes):
                raise ValueError("fuzzy_terms: max_edits is None, or 0 .. 2 for every word")
        out = [([], 0)] * W
        ask = [i for i in range(W) if lookable(words[i])]
        step = _abi.MSR_FUZZY_MAX_WORDS
        for a in range(0, len(ask), step):
            part = ask[a:a + step]
            n = len(part)
            off, chars = encode_words([words[i] for i in part])
            # ONE upload: offsets, tolerances, then the code points two to a word
            chars32 = np.zeros((len(chars) + 1) // 2 + 1, np.int32)
            chars32.view(np.uint16)[:len(chars)] = chars
            up = self._dev(np.concatenate([off, np.asarray([maxes[i] for i in part], np.int32), chars32]), torch.int32)
            d_off, d_max, d_chars = up[:n + 1], up[n + 1:2 * n + 1], up[2 * n + 1:]
            res = torch.empty((2 * n * limit + 2 * n,), dtype=torch.int32, device=self.device)
            need = int(self.lib.msr_fuzzy_scratch_bytes(self.index.n_terms, n, limit))
            scratch = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=self.device)
            r_term, r_dist = res[:n * limit], res[n * limit:2 * n * limit]
            r_n, r_total = res[2 * n * limit:2 * n * limit + n], res[2 * n * limit + n:]
            self._check(self.lib.msr_fuzzy_terms(self.handle, n, _ptr(d_off), _ptr(d_chars), _ptr(d_max), limit, _ptr(r_term),
                                                 _ptr(r_dist), _ptr(r_n), _ptr(r_total), _ptr(scratch), need, self._stream()))
            host = res.cpu().numpy()
            term, dist = host[:n * limit].reshape(n, limit), host[n * limit:2 * n * limit].reshape(n, limit)
            cnt, total = host[2 * n * limit:2 * n * limit + n], host[2 * n * limit + n:]
            for j, i in enumerate(part):
                out[i] = ([(int(term[j, c]), int(dist[j, c])) for c in range(int(cnt[j]))], int(total[j]))
        return out

    def wildcard_terms(self, patterns, limit=8):
        """The vocabulary terms each pattern matches (msr_wildcard_terms, DESIGN K16) -> per pattern ([term id, ...], total):
        the first `limit` (1 .. 16) matches -- terms with a document frequency above 0 that the pattern matches as a whole,
        `*` standing for any run of code points and `?` for exactly one -- ordered by document frequency descending, then
        term id, and the number of all matches.  A pattern the device cannot take (empty, more than 32 symbols, a code point
        above 0xFFFE) gets ([], 0) without a lookup.  ONE upload, two launches, one copy back for up to
        MSR_WILD_MAX_PATTERNS patterns; longer lists go in slices.  Raises MsrError without a vocabulary."""
        from .fuzzy import encode_words
        from .wildcard import encodable
        if not self.has_vocab:
            raise _abi.MsrError(-2, "wildcard_terms: the index has no vocabulary (CorpusIndex.vocab: term strings); a "
                                    "term-id-only index cannot expand a pattern")
        limit = int(limit)
        if not 1 <= limit <= _abi.MSR_WILD_MAX_LIMIT:
            raise ValueError(f"wildcard_terms: limit must be 1 .. MSR_WILD_MAX_LIMIT = {_abi.MSR_WILD_MAX_LIMIT} (got {limit})")
        patterns = list(patterns)
        out = [([], 0)] * len(patterns)
        ask = [i for i in range(len(patterns)) if encodable(patterns[i])]
        step = _abi.MSR_WILD_MAX_PATTERNS
        for a in range(0, len(ask), step):
            part = ask[a:a + step]
            n = len(part)
            off, chars = encode_words([patterns[i] for i in part])
            chars32 = np.zeros((len(chars) + 1) // 2 + 1, np.int32)         # ONE upload: offsets, then the symbols two to a word
            chars32.view(np.uint16)[:len(chars)] = chars
            up = self._dev(np.concatenate([off, chars32]), torch.int32)
            d_off, d_chars = up[:n + 1], up[n + 1:]
            res = torch.empty((n * limit + 2 * n,), dtype=torch.int32, device=self.device)
            need = int(self.lib.msr_wildcard_scratch_bytes(self.index.n_terms, n, limit))
            scratch = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=self.device)
            r_term, r_n, r_total = res[:n * limit], res[n * limit:n * limit + n], res[n * limit + n:]
            self._check(self.lib.msr_wildcard_terms(self.handle, n, _ptr(d_off), _ptr(d_chars), limit, _ptr(r_term), _ptr(r_n),
                                                    _ptr(r_total), _ptr(scratch), need, self._stream()))
            host = res.cpu().numpy()
            term, cnt, total = host[:n * limit].reshape(n, limit), host[n * limit:n * limit + n], host[n * limit + n:]
            for j, i in enumerate(part):
                out[i] = ([int(term[j, c]) for c in range(int(cnt[j]))], int(total[j]))
        return out

    def scan_arith(self):
        """'f32' (exact f32 MFMA) or 'f16x2' (f32 rows split into two f16 pieces, f32 accumulation)."""
        return {0: "f32", 1: "f16x2"}.get(self.lib.msr_scan_arith(self.handle), "none")

    # ------------------------------------------------------------------ stage 1
    def batch_width(self):
        """Queries served by one bf16 sweep in dense_topk_batched (128 or 64; -1 before enable_bf16)."""
        return int(self.lib.msr_batch_width(self.handle))

    def batch_gemm_ok(self):
        """True if dense_topk_batched runs batches of more than 128 queries as the tiled matrix-core GEMM."""
        return bool(self.lib.msr_batch_gemm_ok(self.handle))

    def scan_width(self):
        """Most queries one pass over the embedding matrix serves in dense_topk (256 / 128: streaming pass, 64: K-split sweep,
        else 32)."""
        return int(self.lib.msr_scan_width(self.handle))

    def row_copy_state(self):
        """'none' (not applicable), 'built', 'declined' (row_copy=False) or 'alloc_failed' (fell back to the row-major matrix)."""
        return {0: "none", 1: "built", 2: "declined", 3: "alloc_failed"}.get(self.lib.msr_row_copy_state(self.handle), "?")

    def row_image_state(self):
        """The f16 image of the rows that launches of several 256-query groups read (max_queries >= 512): 'none', 'built',
        'declined' or 'alloc_failed' (those launches then convert the f32 rows in registers, like a single-group launch)."""
        return {0: "none", 1: "built", 2: "declined", 3: "alloc_failed"}.get(self.lib.msr_row_image_state(self.handle), "?")

    def owned_bytes(self):
        """Device bytes the handle owns (scratch, tables and copies built at bind); the bound index tensors are not included."""
        return int(self.lib.msr_owned_bytes(self.handle))

    def dense_path(self):
        """Queries per pass of the kernel the most recent dense_topk call ran (256 / 128 / 64 / 32; 0 before the first)."""
        return int(self.lib.msr_dense_path(self.handle))

    def dense_pass_info(self):
        """(segments, entries) of the streaming pass of the most recent dense_topk / dense_begin call: emit launches per query
        group (1: one launch over all tiles; 2: cut once, thresholds raised in between; 0: the call ran on the sweeps) and the
        entries it appended to its wave buffers.  Diagnostic: waits for the device."""
        seg, ent = C.c_int32(0), C.c_int64(0)
        self._check(self.lib.msr_dense_pass_info(self.handle, C.byref(seg), C.byref(ent)))
        return int(seg.value), int(ent.value)

    def pack_queries(self, term_lists):
        """list of term-id lists (repeats allowed, any unknown id < 0) -> device CSR of UNIQUE terms in
        first-occurrence order with their query frequencies (bm25_indexer.py:405-409)."""
        off, terms, qtf = [0], [], []
        for tl in term_lists:
            cnt = {}
            for t in tl:
                cnt[int(t)] = cnt.get(int(t), 0) + 1
            if len(cnt) > 64:
                raise ValueError("a query may hold at most 64 unique terms (MSR_MAX_QUERY_TERMS)")
            for t, c in cnt.items():
                terms.append(t)
                qtf.append(c)
            off.append(len(terms))
        mk = lambda a: torch.tensor(a if a else [0], dtype=torch.int32, device=self.device)
        return mk(off), mk(terms), mk(qtf), len(term_lists)

    def pack_within(self, within, n_queries):
        """within (None | DocSet | list / tuple of DocSet / None per query) -> (set words int32 [n_sets, stride] device, q_set
        int32 [n_queries] device, n_sets, stride) for msr_*_topk_within; identical sets are stacked once (docset.pack_within).
        One DocSet for every query: its cached device copy and q_set = 0, nothing packed on the host."""
        from .docset import DeviceSets, DocSet, pack_within
        if isinstance(within, DeviceSets):                   # built on the device (term_sets): its fields as they are
            within.check(self.index)
            if len(within) != n_queries:
                raise ValueError(f"within: {len(within)} entries for {n_queries} queries")
            return within.bits, within.q_set, within.n_sets, within.stride
        if isinstance(within, DocSet):
            within.check(self.index)
            stride = max(1, (self.index.n_docs + 31) // 32)
            bits = within.to(self.device).reshape(1, -1)
            if bits.shape[1] < stride:                       # (an index without documents: one zero word)
                bits = torch.nn.functional.pad(bits, (0, stride - bits.shape[1]))
            return bits, torch.zeros((n_queries,), dtype=torch.int32, device=self.device), 1, stride
        words, q_set, n_sets, stride = pack_within(within, n_queries, self.index)
        bits = torch.from_numpy(words.view(np.int32)).to(self.device)
        return bits, torch.from_numpy(q_set).to(self.device), n_sets, stride

    def term_sets(self, must, must_not=None, within=None):
        """Per-query document sets from posting lists, built on the device (msr_term_sets): query q's set is the documents of
        within[q] that hold EVERY term of must[q] and NONE of must_not[q].  must / must_not: per query a list of term ids
        (None: no lists of that kind), unknown ids < 0 as CorpusIndex.term_ids gives them: an unknown must term empties the
        set, an unknown must_not term is ignored.  within: None, a DocSet (every query) or a list of DocSet / None per query.
        -> DeviceSets (bits, q_set, n_sets, stride), to be passed as within= to bm25_topk / dense_topk / dense_topk_grouped.
        Queries with the same (set of must ids, set of must_not ids, base) share one row -- compared as sets of ids on the
        host (repeats and order do not matter), never on bits; must_not ids the index lacks or whose list is empty are dropped
        here.  A query without operators gets its base's row, or -1, and costs no kernel row.  Reads nothing back; the upload of
        the lists is a blocking copy on the caller's stream (it waits for what the stream holds).  The
        FIRST call after a bind also reads the document frequencies (term_off, for the order of the must terms) once: a
        synchronous copy of 8 bytes per term if the index lives on the device; they are kept until the next bind."""
        from .docset import DeviceSets
        bits, q_set, n_sets, stride, _ = self._term_rows(must, must_not, within)
        return DeviceSets(self.index, bits, torch.tensor(q_set, dtype=torch.int32, device=self.device), n_sets, stride)

    def _doc_freq(self):
        """int64 [n_terms]: the document frequencies of the bound index (term_sets and match.match_sets order their lists by
        them), read once per bind and kept until the next."""
        from .index import _np
        ix = self.index
        df = getattr(self, "_df", None)
        if df is None or df[0] is not ix:
            df = self._df = (ix, np.diff(_np(ix.term_off).astype(np.int64)))
        return df[1]

    def _term_rows(self, must, must_not, within, extra_rows=0, tail=None):
        """The work of term_sets -> (bits int32 [n_sets + extra_rows, stride] device, q_set as a HOST list, n_sets, stride,
        tail on the device or None); the extra rows (behind the n_sets rows, not written here) are for a caller that derives
        further rows (phrase_sets).  tail(q_set, n_sets) -> a list of int32 values that travel in the SAME upload as the term
        lists (the caller's own lists, built from the row numbers): the call then costs one upload, not two."""
        from .docset import DeviceSets, DocSet, pack_within
        from .index import _np
        ix = self.index
        if ix.term_off is None or ix.n_terms <= 0:
            raise _abi.MsrError(-2, "term_sets: the index has no postings")
        if must is None and must_not is None:
            raise ValueError("term_sets: must or must_not is needed (a list of term ids per query)")
        Q = len(must if must is not None else must_not)
        must = [()] * Q if must is None else list(must)
        must_not = [()] * Q if must_not is None else list(must_not)
        if len(must) != Q or len(must_not) != Q:
            raise ValueError(f"term_sets: {len(must)} must lists and {len(must_not)} must_not lists")
        stride = max(1, (ix.n_docs + 31) // 32)
        base_bits, n_base, base_of = None, 0, [-1] * Q
        if isinstance(within, DocSet):
            base_bits, _, n_base, _ = self.pack_within(within, Q)
            base_of = [0] * Q
        elif within is not None:
            if isinstance(within, DeviceSets):
                raise TypeError("term_sets: within takes DocSets (a DeviceSets is a result, not a base)")
            words, base_q, n_base, _ = pack_within(within, Q, ix)
            base_of = base_q.tolist()
            if n_base:
                base_bits = torch.from_numpy(words.view(np.int32)).to(self.device)
        df, n_terms = self._doc_freq(), int(ix.n_terms)
        EMPTY = ((-1,), ())
        rows, row_of, q_row, keep_base = [], {}, [], False
        for q in range(Q):
            m = {int(t) if 0 <= int(t) < n_terms else -1 for t in must[q]}
            x = {int(t) for t in must_not[q] if 0 <= int(t) < n_terms and df[int(t)] > 0}
            if not m and not x:
                q_row.append(None)
                keep_base = keep_base or base_of[q] >= 0
                continue
            if -1 in m or m & x or any(df[t] == 0 for t in m):
                key = EMPTY + (-1,)
            else:                                            # the shortest list first: it empties most spans for the others
                key = (tuple(sorted(m, key=lambda t: (df[t], t))), tuple(sorted(x)), base_of[q])
            r = row_of.get(key)
            if r is None:
                r = row_of[key] = len(rows)
                rows.append(key)
            q_row.append(r)
        first = n_base if keep_base else 0                   # base rows that operator-less queries still name come first
        q_set = [(base_of[q] if base_of[q] >= 0 and keep_base else -1) if r is None else first + r for q, r in enumerate(q_row)]
        bits = torch.empty((first + len(rows) + int(extra_rows), stride), dtype=torch.int32, device=self.device)
        if first:
            bits[:first] = base_bits
        n_sets = first + len(rows)
        tail_host = [int(v) for v in tail(q_set, n_sets)] if tail is not None else []
        d_tail = None
        if not rows and tail_host:
            d_tail = torch.from_numpy(np.asarray(tail_host, np.int32)).to(self.device)
        if rows:
            m_off, m_terms, x_off, x_terms = [0], [], [0], []
            for m, x, _ in rows:
                m_terms.extend(m); m_off.append(len(m_terms))
                x_terms.extend(x); x_off.append(len(x_terms))
            R = len(rows)
            host = np.asarray(m_off + x_off + [b for _, _, b in rows] + m_terms + x_terms + tail_host, np.int32)
            dev = torch.from_numpy(host).to(self.device)
            p_moff, p_xoff, p_base = dev[:R + 1], dev[R + 1:2 * R + 2], dev[2 * R + 2:3 * R + 2]
            p_m = dev[3 * R + 2:3 * R + 2 + len(m_terms)]
            end = 3 * R + 2 + len(m_terms) + len(x_terms)
            p_x = dev[3 * R + 2 + len(m_terms):end]
            if tail_host:
                d_tail = dev[end:]
            self._check(self.lib.msr_term_sets(self.handle, R, _ptr(p_moff), _ptr(p_m), _ptr(p_xoff), _ptr(p_x),
                                               _ptr(base_bits) if n_base else C.c_void_p(0), n_base, stride,
                                               _ptr(p_base) if n_base else C.c_void_p(0), _ptr(bits[first:]), stride,
                                               self._stream()))
        return bits, q_set, n_sets, stride, d_tail

    # ------------------------------------------------------------------ facet counts (msr_facet_counts, DESIGN K17)
    @property
    def has_facet(self):
        """True while a facet table is bound (bind_facet); a rebind drops it with the postings."""
        return "facet_local" in self._t

    def bind_facet(self, value, n_values):
        """Bind one facet to the bound postings' documents: value int32 [N] in [-1, n_values) (-1: none; facets.facet_values).
        The table is built on the host (facets.build_table, msr_facet_table), uploaded and checked once on the device
        (msr_bind_facet: the call synchronises).  The arrays live with the postings' tensors: rebind / unbind drop them.
        value=None unbinds."""
        from .facets import build_table
        names = ("facet_local", "facet_span_off", "facet_span_values", "facet_value_off", "facet_value_pos")
        if value is None:
            null = C.c_void_p(0)
            self._check(self.lib.msr_bind_facet(self.handle, null, null, null, null, null, 0, 0, self._stream()))
            for k in names:
                self._t.pop(k, None)
            self._facet_n_values = 0
            return
        value = np.ascontiguousarray(value, np.int32)
        if value.shape != (self.index.n_docs,):
            raise ValueError(f"bind_facet: {value.shape} values for {self.index.n_docs} documents")
        local, span_off, span_values, value_off, value_pos = build_table(value, n_values)
        with torch.cuda.device(self.device):
            dev = [self._dev(local.view(np.int16), torch.int16)] + \
                  [self._dev(a, torch.int32) for a in (span_off, span_values, value_off, value_pos)]
            self._check(self.lib.msr_bind_facet(self.handle, *[_ptr(t) if t.numel() else C.c_void_p(0) for t in dev],
                                                self.index.n_docs, int(n_values), self._stream()))
        self._t.update(zip(names, dev))                      # (a refused table leaves the previous binding and its tensors)
        self._facet_n_values = int(n_values)

    def facet_counts(self, term_lists, within=None, limit=10, counts=False):
        """Per row: how many documents hold AT LEAST ONE of the row's terms inside its set, and how many of those carry each
        value of the bound facet (msr_facet_counts) -> host arrays (hits int32 [R], n_values_hit int32 [R], top_value int32
        [R, limit], top_count int32 [R, limit][, counts int32 [R, n_values] with counts=True]): the values with a count above 0
        in (count desc, value asc) order, the first `limit` (0 .. MSR_FACET_MAX_LIMIT) of them, the rest of a row -1 / 0.
        term_lists: per row a list of term ids (repeats allowed; ids the index lacks contribute nothing); an EMPTY list is no
        term condition -- the row counts its whole set.  within: None, a DocSet, a list of DocSet / None per row, or a
        DeviceSets (term_sets / phrase_sets), through pack_within.  Documents without a value count in hits only.  The rows go
        through the device in slices of at most max_queries, one scratch tensor for all of them, one copy back per slice."""
        if not self.has_facet:
            raise _abi.MsrError(-2, "facet_counts: no facet bound (bind_facet)")
        limit = int(limit)
        if not 0 <= limit <= _abi.MSR_FACET_MAX_LIMIT:
            raise ValueError(f"facet_counts: limit must be 0 .. MSR_FACET_MAX_LIMIT = {_abi.MSR_FACET_MAX_LIMIT} (got {limit})")
        term_lists = [[int(t) for t in tl] for tl in term_lists]
        R, V = len(term_lists), self._facet_n_values
        bits, q_set, n_base, stride = self.pack_within(within, R)
        hits, n_hit = np.zeros(R, np.int32), np.zeros(R, np.int32)
        top_value, top_count = np.full((R, limit), -1, np.int32), np.zeros((R, limit), np.int32)
        all_counts = np.zeros((R, V), np.int32) if counts else None
        step = max(1, self.max_queries)
        need = int(self.lib.msr_facet_scratch_bytes(self.handle, min(step, R)))
        if need < 0:
            self._check(need)
        scratch = torch.empty((max(1, (need + 15) // 16 * 2),), dtype=torch.int64, device=self.device)
        for a in range(0, R, step):
            b = min(R, a + step)
            n = b - a
            off, terms = [0], []
            for tl in term_lists[a:b]:
                terms += tl
                off.append(len(terms))
            up = torch.from_numpy(np.asarray(off + terms, np.int32)).to(self.device)     # ONE upload: offsets, then the ids
            d_off, d_terms = up[:n + 1], up[n + 1:]
            res = torch.empty((2 * n + 2 * n * limit + (n * V if counts else 0),), dtype=torch.int32, device=self.device)
            r_hits, r_nh = res[:n], res[n:2 * n]
            r_tv, r_tc = res[2 * n:2 * n + n * limit], res[2 * n + n * limit:2 * n + 2 * n * limit]
            r_cnt = res[2 * n + 2 * n * limit:] if counts else None
            self._check(self.lib.msr_facet_counts(
                self.handle, n, _ptr(d_off), _ptr(d_terms) if terms else C.c_void_p(0), _ptr(bits) if n_base else C.c_void_p(0),
                n_base, stride, _ptr(q_set[a:b]) if n_base else C.c_void_p(0), limit, _ptr(r_hits), _ptr(r_nh),
                _ptr(r_tv) if limit else C.c_void_p(0), _ptr(r_tc) if limit else C.c_void_p(0),
                _ptr(r_cnt) if counts and V else C.c_void_p(0), V, _ptr(scratch), need, self._stream()))
            host = res.cpu().numpy()
            hits[a:b], n_hit[a:b] = host[:n], host[n:2 * n]
            top_value[a:b] = host[2 * n:2 * n + n * limit].reshape(n, limit)
            top_count[a:b] = host[2 * n + n * limit:2 * n + 2 * n * limit].reshape(n, limit)
            if counts:
                all_counts[a:b] = host[2 * n + 2 * n * limit:].reshape(n, V)
        return (hits, n_hit, top_value, top_count) + ((all_counts,) if counts else ())

    # ------------------------------------------------------------------ near-duplicate collapse (msr_collapse_duplicates, DESIGN K18)
    def doc_signatures(self, shingle=4, d0=0, d1=None, out=None):
        """The min-hash signatures of documents [d0, d1) of the bound forward index (msr_doc_signatures) -> device tensor int32
        [d1 - d0, MSR_SIG_WORDS] (the bits of the uint32 words).  shingle: 1 .. MSR_SIG_MAX_SHINGLE tokens.  out: write into
        the rows of this tensor instead.  Only enqueues."""
        d1 = self.index.n_docs if d1 is None else int(d1)
        d0 = int(d0)
        if out is None:
            out = torch.empty((max(d1 - d0, 0), _abi.MSR_SIG_WORDS), dtype=torch.int32, device=self.device)
        self._check(self.lib.msr_doc_signatures(self.handle, d0, d1, int(shingle), _ptr(out) if out.numel() else C.c_void_p(0),
                                                self._stream()))
        return out

    @property
    def has_signatures(self):
        """True while a signature table is bound (bind_signatures); a rebind drops it with the postings."""
        return "doc_sig" in self._t

    def bind_signatures(self, sig):
        """Bind the signatures of ALL bound documents (doc_signatures(); int32 device tensor [N, MSR_SIG_WORDS]) for
        collapse_duplicates.  The tensor lives with the postings' tensors: rebind drops it.  None unbinds."""
        if sig is None:
            self._check(self.lib.msr_bind_signatures(self.handle, C.c_void_p(0), 0, self._stream()))
            self._t.pop("doc_sig", None)
            return
        if sig.dtype != torch.int32 or sig.dim() != 2 or sig.shape[1] != _abi.MSR_SIG_WORDS or sig.device != self.device:
            raise ValueError(f"bind_signatures: an int32 [N, {_abi.MSR_SIG_WORDS}] tensor on {self.device} is needed")
        sig = sig.contiguous()
        n = int(sig.shape[0])
        self._check(self.lib.msr_bind_signatures(self.handle, _ptr(sig) if n else C.c_void_p(0), n, self._stream()))
        if n:
            self._t["doc_sig"] = sig
        else:
            self._t.pop("doc_sig", None)

    def collapse_duplicates(self, fused, min_matches):
        """fused = (doc, score, orig, chunk, n, ...) of rerank / rerank_fuse -> ((doc, score f64, orig f64, chunk, n), (drop_doc,
        drop_leader, drop_matches, drop_n)): every query's list without the rows whose signature agrees with an earlier kept
        row's in at least min_matches (1 .. 64) of 64 words -- the first tuple feeds diversify unchanged -- and, in drop
        order, the dropped documents, the document that swallowed each and their match counts (int32 [Q, M] / [Q]).  The
        bound doc-domain table is read: a document it rejects neither drops nor leads.  Only enqueues."""
        if not self.has_signatures:
            raise _abi.MsrError(-2, "collapse_duplicates: no signatures bound (bind_signatures)")
        doc, score, orig, chunk, n = [x.contiguous() for x in fused[:5]]
        Q, M = int(doc.shape[0]), int(doc.shape[1])
        mk = lambda dt: torch.empty((Q, M), dtype=dt, device=self.device)
        o_doc, o_score, o_orig, o_chunk = mk(torch.int32), mk(torch.float64), mk(torch.float64), mk(torch.int32)
        d_doc, d_lead, d_m = mk(torch.int32), mk(torch.int32), mk(torch.int32)
        o_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        d_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        need = int(self.lib.msr_collapse_scratch_bytes(Q, M))
        scratch = torch.empty((max(need, 16) // 8,), dtype=torch.int64, device=self.device)
        self._check(self.lib.msr_collapse_duplicates(
            self.handle, Q, _ptr(doc), _ptr(score), _ptr(orig), _ptr(chunk), _ptr(n), M, int(min_matches), _ptr(o_doc),
            _ptr(o_score), _ptr(o_orig), _ptr(o_chunk), _ptr(o_n), _ptr(d_doc), _ptr(d_lead), _ptr(d_m), _ptr(d_n), _ptr(scratch),
            max(need, 0), self._stream()))
        return (o_doc, o_score, o_orig, o_chunk, o_n), (d_doc, d_lead, d_m, d_n)

    def phrase_sets(self, must_phrases, must_not_phrases=None, must=None, must_not=None, within=None):
        """Per-query document sets of phrase search, built on the device: query q's set is the documents of within[q] that hold
        every term of must[q], none of must_not[q] (term_sets' rules), EVERY phrase of must_phrases[q] and NO phrase of
        must_not_phrases[q].  A phrase is a list of 1 .. MSR_PHRASE_MAX_TERMS term ids (unknown ids < 0 as CorpusIndex.term_ids
        gives them); a document holds it when the ids stand next to each other, in this order, in its indexed token stream
        (msretr.h msr_phrase_sets).  A must phrase with an unknown id, or an empty one, empties the set; such a not phrase is
        ignored; a longer phrase raises ValueError.  -> DeviceSets, for every consumer of term_sets' result.

        Three launches, nothing is read back (the uploads of the host lists are blocking copies on the caller's stream: they
        wait for what the stream holds): ONE term_sets call builds every phrase's candidate row (a must phrase: its
        terms AND the query's base and must / must_not terms; a not phrase: its terms AND the base), ONE msr_phrase_sets call
        verifies the distinct (phrase, candidate row) pairs -- compared as tuples on the host, identical pairs share a row --
        and ONE msr_combine_sets call gives each query the AND of its must rows without its not rows (a query with only not
        phrases: its term / base row without them); every list of the three calls and q_set travel in ONE upload.  The
        result's `layout` is (term rows, phrase rows, per-query rows).  A query without phrases keeps its term_sets row, or -1, and costs no
        phrase row.  Raises MsrError when the index has no forward index (index_build.attach_tokens, or a build with
        keep_tokens=True, gives it one).

        Proximity (DESIGN K13): wherever a phrase may stand, a text.Near of ids may -- the terms within a window, in order or
        in any order (msretr.h msr_proximity_sets).  Its candidate row comes from the same term_sets call, built from its
        ids exactly as a phrase's; the distinct (ids, span, ordered, candidate row) tuples get rows BEHIND the exact phrases'
        rows, ONE msr_proximity_sets call verifies them, the one msr_combine_sets call reads both kinds, and their lists
        travel in the same upload.  `layout` stays (T, P, C) with P = exact + proximity rows; `n_near` says how many of the P
        are proximity rows.  An unknown id follows the phrases' rule.  A call without a Near launches and uploads what it did."""
        from .docset import DeviceSets, DocSet
        from .text import Near
        ix = self.index
        if not self.has_tokens:
            raise _abi.MsrError(-2, "phrase_sets: the index has no forward index (tok_off / tok_ids): build it with "
                                    "keep_tokens=True or attach the token streams with index_build.attach_tokens, then rebind")
        if must_phrases is None and must_not_phrases is None:
            raise ValueError("phrase_sets: must_phrases or must_not_phrases is needed (a list of phrases per query)")
        Q = len(must_phrases if must_phrases is not None else must_not_phrases)
        lists = [[()] * Q if x is None else list(x) for x in (must_phrases, must_not_phrases, must, must_not)]
        if any(len(x) != Q for x in lists):
            raise ValueError(f"phrase_sets: {[len(x) for x in lists]} must_phrases / must_not_phrases / must / must_not lists")
        mp, xp, m, x = lists
        if isinstance(within, DocSet) or within is None:
            base = [within] * Q
        else:
            if isinstance(within, DeviceSets):
                raise TypeError("phrase_sets: within takes DocSets (a DeviceSets is a result, not a base)")
            base = list(within)
            if len(base) != Q:
                raise ValueError(f"within: {len(base)} entries for {Q} queries")
        n_terms = int(ix.n_terms)
        ids_of = lambda p: tuple(int(t) if 0 <= int(t) < n_terms else -1 for t in p)
        norm = lambda p: p.with_terms(ids_of(p.terms)) if isinstance(p, Near) else ids_of(p)
        terms_of = lambda p: list(p.terms) if isinstance(p, Near) else list(p)
        # virtual queries of the one term_sets call: per query its own (terms, base) row, then one per phrase
        v_must, v_not, v_base, plan = [], [], [], []
        for q in range(Q):
            ph_m, ph_x = [norm(p) for p in mp[q]], [norm(p) for p in xp[q]]
            for p in ph_m + ph_x:
                if len(p) > _abi.MSR_PHRASE_MAX_TERMS:
                    raise ValueError(f"a phrase may hold at most {_abi.MSR_PHRASE_MAX_TERMS} terms (MSR_PHRASE_MAX_TERMS), got {len(p)}")
            own = len(v_must)
            v_must.append(list(m[q])); v_not.append(list(x[q])); v_base.append(base[q])
            plan.append((own, ph_m, len(v_must), ph_x, len(v_must) + len(ph_m)))
            for p in ph_m:
                v_must.append(terms_of(p) + list(m[q])); v_not.append(list(x[q])); v_base.append(base[q])
            for p in ph_x:
                v_must.append(terms_of(p)); v_not.append([]); v_base.append(base[q])
        n_phrase_q = sum(1 for pl in plan if pl[1] or pl[3])
        if not any(b is not None for b in v_base):
            v_base = None
        # the buffer holds the term rows, then the distinct (phrase, candidate row) pairs' rows (at most one per phrase), then
        # one row per query with phrases.  The phrase and combine lists need the term rows' numbers, which _term_rows knows
        # before it uploads: it calls lists_of() and sends the result along with its own lists (one upload for the whole call)
        V = len(v_must)
        rows, near, cut = [], [], []                         # exact rows, proximity rows (behind them): (phrase, candidate row)

        def lists_of(v_row, T):
            row_of = {}
            and_off, and_ref, not_off, not_ref, q_set = [0], [], [0], [], []
            for q, (own, ph_m, i_m, ph_x, i_x) in enumerate(plan):
                if not ph_m and not ph_x:
                    q_set.append(v_row[own])
                    continue
                rm = []
                for key in [(p, v_row[i_m + j]) for j, p in enumerate(ph_m)] + [(p, v_row[i_x + j]) for j, p in enumerate(ph_x)]:
                    r = row_of.get(key)
                    if r is None:
                        kind = near if isinstance(key[0], Near) else rows
                        r = row_of[key] = (kind, len(kind))
                        kind.append(key)
                    rm.append(r)
                a = rm[:len(ph_m)]
                if not ph_m and v_row[own] != -1:            # only not phrases: the query's own term / base row
                    a = [v_row[own]]
                and_ref += a; and_off.append(len(and_ref))
                not_ref += rm[len(ph_m):]; not_off.append(len(not_ref))
                q_set.append(None)
            # a row's number: the exact rows stand at T, the proximity rows behind them
            at = lambda ref: ref if not isinstance(ref, tuple) else T + ref[1] + (len(rows) if ref[0] is near else 0)
            and_rows, not_rows = [at(ref) for ref in and_ref], [at(ref) for ref in not_ref]
            k = 0
            for q in range(Q):
                if q_set[q] is None:
                    q_set[q] = T + len(rows) + len(near) + k
                    k += 1
            p_off, p_terms = [0], []
            for p, _ in rows:
                p_terms += list(p); p_off.append(len(p_terms))
            parts = [p_off, [c for _, c in rows], and_off, not_off, p_terms, and_rows, not_rows, q_set]
            if near:
                n_off, n_terms_ = [0], []
                for p, _ in near:
                    n_terms_ += list(p.terms); n_off.append(len(n_terms_))
                parts += [n_off, [c for _, c in near], [p.span for p, _ in near], [int(p.ordered) for p, _ in near], n_terms_]
            cut.extend(np.cumsum([0] + [len(part) for part in parts]).tolist())
            return [v for part in parts for v in part]

        bits, _, T, stride, dev = self._term_rows(v_must, v_not, v_base, extra_rows=(V - Q) + n_phrase_q, tail=lists_of)
        d_poff, d_cand, d_aoff, d_xoff, d_pt, d_a, d_x, d_q = [dev[cut[i]:cut[i + 1]] for i in range(8)]
        P, Pn, C_ = len(rows), len(near), int(d_aoff.numel()) - 1
        if C_:
            ptr = lambda t: _ptr(t) if t.numel() else C.c_void_p(0)
            cand = (ptr(bits[:T]) if T else C.c_void_p(0), T, stride)
            if P:
                self._check(self.lib.msr_phrase_sets(self.handle, P, _ptr(d_poff), ptr(d_pt), *cand,
                                                     _ptr(d_cand) if T else C.c_void_p(0), _ptr(bits[T:]), stride, self._stream()))
            if Pn:
                d_noff, d_ncand, d_nspan, d_nord, d_nt = [dev[cut[i]:cut[i + 1]] for i in range(8, 13)]
                self._check(self.lib.msr_proximity_sets(self.handle, Pn, _ptr(d_noff), ptr(d_nt), _ptr(d_nspan), _ptr(d_nord), *cand,
                                                        _ptr(d_ncand) if T else C.c_void_p(0), _ptr(bits[T + P:]), stride,
                                                        self._stream()))
            self._check(self.lib.msr_combine_sets(self.handle, C_, _ptr(d_aoff), ptr(d_a), _ptr(d_xoff), ptr(d_x), _ptr(bits),
                                                  T + P + Pn, stride, _ptr(bits[T + P + Pn:]), stride, self._stream()))
        out = DeviceSets(ix, bits[:T + P + Pn + C_], d_q, T + P + Pn + C_, stride)
        out.layout = (T, P + Pn, C_)
        out.n_near = Pn
        return out

    def best_windows(self, pair_doc, pair_row, rows, weights, spans):
        """Query-biased snippets (msr_best_windows, DESIGN K14): per pair (pair_doc[i], pair_row[i]) the window of the
        document's token stream that covers the most weight of row pair_row[i] -> five device tensors of len(pair_doc)
        entries: start int32 (-1: no window), cover int32, hits int32, mask int64 (the uint64 position mask's bits), terms
        int32 (the uint32 term bits).  rows: lists of term ids, weights: lists of ints (one per id), spans: an int or one per
        row.  pair_doc / pair_row: host arrays or device tensors of document indices and row numbers.  Every list travels in
        ONE upload (host pairs with them; a blocking copy on the caller's stream, so it waits for what the stream holds), ONE
        launch follows and nothing is read back: the caller copies back.  What the
        ABI turns into "no window" (an id, weight, span, document or row out of range) is not checked here.  Raises MsrError
        when the index has no forward index."""
        if not self.has_tokens:
            raise _abi.MsrError(-2, "best_windows: the index has no forward index (tok_off / tok_ids): build it with "
                                    "keep_tokens=True or attach the token streams with index_build.attach_tokens, then rebind")
        R = len(rows)
        if len(weights) != R:
            raise ValueError(f"best_windows: {len(weights)} weight lists for {R} rows")
        spans = [int(spans)] * R if np.ndim(spans) == 0 else [int(v) for v in spans]
        if len(spans) != R:
            raise ValueError(f"best_windows: {len(spans)} spans for {R} rows")
        off, terms, wts = [0], [], []
        for p, w in zip(rows, weights):
            if len(p) != len(w):
                raise ValueError(f"best_windows: a row of {len(p)} terms with {len(w)} weights")
            terms += [int(t) for t in p]; wts += [int(v) for v in w]; off.append(len(terms))
        on_dev = torch.is_tensor(pair_doc) and pair_doc.is_cuda
        if on_dev != (torch.is_tensor(pair_row) and pair_row.is_cuda):
            raise ValueError("best_windows: pair_doc and pair_row are both host arrays or both device tensors")
        n = int(pair_doc.numel()) if on_dev else len(pair_doc)
        if (int(pair_row.numel()) if on_dev else len(pair_row)) != n:
            raise ValueError("best_windows: pair_doc and pair_row differ in length")
        parts = [off, terms or [0], wts or [0], spans or [0]]     # (an empty list keeps a word, so that no pointer is NULL)
        if not on_dev:
            parts += [np.asarray(pair_doc, np.int64).astype(np.int32).reshape(-1) if n else [0],
                      np.asarray(pair_row, np.int64).astype(np.int32).reshape(-1) if n else [0]]
        cut = np.cumsum([0] + [len(p) for p in parts])
        dev = self._dev(np.concatenate([np.asarray(p, np.int32) for p in parts]), torch.int32)
        d_off, d_terms, d_wts, d_span = [dev[cut[i]:cut[i + 1]] for i in range(4)]
        if on_dev:
            d_doc, d_row = self._dev(pair_doc, torch.int32).reshape(-1), self._dev(pair_row, torch.int32).reshape(-1)
        else:
            d_doc, d_row = dev[cut[4]:cut[5]], dev[cut[5]:cut[6]]
        i32 = lambda: torch.empty(n, dtype=torch.int32, device=self.device)
        out = (i32(), i32(), i32(), torch.empty(n, dtype=torch.int64, device=self.device), i32())
        if n:
            self._check(self.lib.msr_best_windows(self.handle, n, _ptr(d_doc), _ptr(d_row), R, _ptr(d_off), _ptr(d_terms),
                                                  _ptr(d_wts), _ptr(d_span), *[_ptr(t) for t in out], self._stream()))
        return out

    def bm25_topk(self, term_lists, k=1000, min_score=0.0, packed=None, within=None):
        """-> (doc index int32 [Q, k], score float64 [Q, k], n int32 [Q]) device tensors.  within: None, a DocSet (every
        query) or a list of DocSet / None per query -- the top k of each query's set (msr_bm25_topk_within)."""
        q_off, q_terms, q_qtf, Q = packed if packed is not None else self.pack_queries(term_lists)
        out_doc = torch.empty((Q, k), dtype=torch.int32, device=self.device)
        out_score = torch.empty((Q, k), dtype=torch.float64, device=self.device)
        out_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        n_sets = 0
        if within is not None:
            bits, q_set, n_sets, stride = self.pack_within(within, Q)
        if n_sets == 0:
            self._check(self.lib.msr_bm25_topk(self.handle, _ptr(q_off), _ptr(q_terms), _ptr(q_qtf), Q, k,
                                               C.c_double(min_score), _ptr(out_doc), _ptr(out_score), _ptr(out_n),
                                               self._stream()))
        else:
            self._check(self.lib.msr_bm25_topk_within(self.handle, _ptr(q_off), _ptr(q_terms), _ptr(q_qtf), Q, k,
                                                      C.c_double(min_score), _ptr(bits), n_sets, stride, _ptr(q_set),
                                                      _ptr(out_doc), _ptr(out_score), _ptr(out_n), self._stream()))
        return out_doc, out_score, out_n

    def bm25_split(self, n_queries):
        """(tiles per work item, segments per query) of the scoring kernel for ONE internal slice of n_queries queries
        (1 .. max_queries) on the bound postings (msr_debug_bm25_split: launches nothing).  For tests that must know which
        split a call ran; results never depend on it."""
        tpw, n_seg = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.msr_debug_bm25_split(self.handle, int(n_queries), C.byref(tpw), C.byref(n_seg)))
        return int(tpw.value), int(n_seg.value)

    SELECT_STATE = np.dtype([("pref_hi", "<u8"), ("mask_hi", "<u8"), ("pref_lo", "<u4"), ("mask_lo", "<u4"), ("k_rem", "<i4"),
                             ("n_above", "<i4"), ("done", "<i4"), ("n_sel", "<i4")])

    def debug_select(self, scores, k, n=None, idx=None, counts=None, seg_stride=0, win_base=None, set_bits=None, q_set=None,
                     gate=None, gate_per64=False, out=None):
        """Test-only (msr_debug_select): the engine's own select over raw score rows.  scores: device tensor [Q, stride],
        float32 or float64, row q = its first n elements (default: the whole row).  Lists (float64 only): idx int32
        [Q, stride], counts int32 [Q, n_seg], seg_stride, optional win_base int64 [Q] (the bits of the uint64 anchors).
        Within (float32 only): set_bits int32 [n_sets, words], q_set int32 [Q].  gate: int32 device word(s).  out: optional
        (doc, score, n) tensors to write into (a gated-off call leaves them alone).
        -> (doc int32 [Q, k], score [Q, k], n int32 [Q], state: numpy record array [Q] of SELECT_STATE, as the streaming
        passes left it).  Synchronises (the state is copied to the host)."""
        assert scores.is_cuda and scores.dim() == 2 and scores.is_contiguous()
        Q, stride = int(scores.shape[0]), int(scores.shape[1])
        f64 = scores.dtype == torch.float64
        if idx is not None:
            mode = _abi.MSR_SELECT_F64_LIST
        elif set_bits is not None:
            mode = _abi.MSR_SELECT_F32_WITHIN
        else:
            mode = _abi.MSR_SELECT_F64 if f64 else _abi.MSR_SELECT_F32
        assert f64 == (mode in (_abi.MSR_SELECT_F64, _abi.MSR_SELECT_F64_LIST)) and scores.dtype in (torch.float32, torch.float64)
        n_seg = int(counts.shape[1]) if counts is not None else 0
        n_sets, set_stride = (int(set_bits.shape[0]), int(set_bits.shape[1])) if set_bits is not None else (0, 0)
        if out is None:
            out = (torch.empty((Q, k), dtype=torch.int32, device=self.device),
                   torch.empty((Q, k), dtype=scores.dtype, device=self.device),
                   torch.empty((Q,), dtype=torch.int32, device=self.device))
        out_doc, out_score, out_n = out
        state = torch.zeros((max(Q, 1) * self.SELECT_STATE.itemsize,), dtype=torch.uint8, device=self.device)
        keep = [t.contiguous() if t is not None else None for t in (idx, counts, win_base, set_bits, q_set, gate)]
        self._check(self.lib.msr_debug_select(
            self.handle, mode, _ptr(scores), stride if n is None else int(n), stride, Q, int(k), _ptr(keep[0]), _ptr(keep[1]),
            n_seg, int(seg_stride), _ptr(keep[2]), _ptr(keep[3]), n_sets, set_stride, _ptr(keep[4]), _ptr(keep[5]),
            1 if gate_per64 else 0, _ptr(out_doc), _ptr(out_score), _ptr(out_n), _ptr(state), self._stream()))
        st = state.cpu().numpy().view(self.SELECT_STATE)[:Q].copy()
        return out_doc, out_score, out_n, st

    def scratch_dirty(self):
        """Test-only (msr_debug_scratch_dirty): {name: non-zero 32-bit words} of every engine buffer documented "zero between
        calls", counted over its whole allocation (-1: not allocated), plus "split_pending": the queries of a dense_begin that
        has not been ended.  Names: _abi.MSR_DIRTY_NAMES.  Every count is 0 after every call.  Synchronises."""
        out = (C.c_int64 * len(_abi.MSR_DIRTY_NAMES))()
        self._check(self.lib.msr_debug_scratch_dirty(self.handle, out, len(_abi.MSR_DIRTY_NAMES), self._stream()))
        return {name: int(out[i]) for i, name in enumerate(_abi.MSR_DIRTY_NAMES)}

    # ------------------------------------------------------------------ hybrid candidates (msr_bm25_point.hip)
    def bm25_score_docs(self, term_lists, doc, doc_n=None, packed=None):
        """BM25 scores of NAMED documents (msr_bm25_score_docs): doc int32 [Q, M] document indices, doc_n int32 [Q] valid
        slots per row (None: all M) -> (score float64 [Q, M], touched int32 [Q, M]) device tensors: bm25_topk's score of
        (query, document) bit for bit, touched = the document holds a query term.  A slot past doc_n or naming no document of
        the index gets 0.0 / 0.  Only enqueues."""
        q_off, q_terms, q_qtf, Q = packed if packed is not None else self.pack_queries(term_lists)
        d = self._dev(doc if torch.is_tensor(doc) else np.asarray(doc, np.int32), torch.int32)
        if d.dim() != 2 or int(d.shape[0]) != Q:
            raise ValueError(f"doc: shape {tuple(d.shape)} for {Q} queries (want [Q, M])")
        M = int(d.shape[1])
        dn = None if doc_n is None else self._dev(doc_n if torch.is_tensor(doc_n) else np.asarray(doc_n, np.int32), torch.int32)
        if dn is not None and tuple(dn.shape) != (Q,):
            raise ValueError(f"doc_n: shape {tuple(dn.shape)} for {Q} queries")
        out_score = torch.empty((Q, M), dtype=torch.float64, device=self.device)
        out_touched = torch.empty((Q, M), dtype=torch.int32, device=self.device)
        self._check(self.lib.msr_bm25_score_docs(self.handle, _ptr(q_off), _ptr(q_terms), _ptr(q_qtf), Q, _ptr(d), _ptr(dn), M,
                                                 _ptr(out_score), _ptr(out_touched), self._stream()))
        return out_score, out_touched

    def union_candidates(self, lex, dense_doc, dense_bm25, dense_n, max_cand=None):
        """lex = (doc int32 [Q, k_lex], score float64 [Q, k_lex], n int32 [Q]) of bm25_topk; dense_doc int32 [Q, k_dense] /
        dense_n int32 [Q] of dense_topk; dense_bm25 float64 [Q, k_dense] of bm25_score_docs -> (doc int32 [Q, max_cand],
        score float64, src int32 (1 lexical, 2 dense, 3 both), n int32 [Q]): the lexical list, then the dense list's new
        documents in dense rank order (msr_union_candidates) -- the cand_doc / cand_bm25 / cand_n of rerank_gather /
        rerank_fuse.  max_cand: columns of the output (default k_lex + k_dense).  Only enqueues."""
        ld, ls, ln = (self._dev(x, dt) for x, dt in zip(lex[:3], (torch.int32, torch.float64, torch.int32)))
        dd, db, dn = self._dev(dense_doc, torch.int32), self._dev(dense_bm25, torch.float64), self._dev(dense_n, torch.int32)
        Q, k_lex, k_dense = int(ld.shape[0]), int(ld.shape[1]), int(dd.shape[1])
        if int(dd.shape[0]) != Q or tuple(ls.shape) != (Q, k_lex) or tuple(db.shape) != (Q, k_dense) or \
                tuple(ln.shape) != (Q,) or tuple(dn.shape) != (Q,):
            raise ValueError("union_candidates: the lists do not have the shapes [Q, k_lex] / [Q, k_dense] / [Q]")
        M = k_lex + k_dense if max_cand is None else int(max_cand)
        out_doc = torch.empty((Q, max(M, 0)), dtype=torch.int32, device=self.device)
        out_score = torch.empty((Q, max(M, 0)), dtype=torch.float64, device=self.device)
        out_src = torch.empty((Q, max(M, 0)), dtype=torch.int32, device=self.device)
        out_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        self._check(self.lib.msr_union_candidates(self.handle, Q, _ptr(ld), _ptr(ls), _ptr(ln), k_lex, _ptr(dd), _ptr(db),
                                                  _ptr(dn), k_dense, _ptr(out_doc), _ptr(out_score), _ptr(out_src), _ptr(out_n),
                                                  M, self._stream()))
        return out_doc, out_score, out_src, out_n

    # ------------------------------------------------------------------ stage 2 (full scan)
    def dense_topk(self, qvec, k=100, max_chunks_per_doc=0, want_chunk=True, within=None):
        """qvec float32 [Q, 768] (not normalised) -> (doc [Q,k] i32, score [Q,k] f32, chunk row [Q,k] i32, n [Q]).
        within: None, a DocSet or a list of DocSet / None per query (msr_dense_topk_within: every query on the sweeps, whose
        scores are the sweep's -- not the exact-f32 rescoring of the 256-query pass)."""
        q = self._dev(qvec, torch.float32).reshape(-1, DIM)
        Q = int(q.shape[0])
        out_doc = torch.empty((Q, k), dtype=torch.int32, device=self.device)
        out_score = torch.empty((Q, k), dtype=torch.float32, device=self.device)
        out_chunk = torch.empty((Q, k), dtype=torch.int32, device=self.device) if want_chunk else None
        out_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        n_sets = 0
        if within is not None:
            bits, q_set, n_sets, stride = self.pack_within(within, Q)
        if n_sets == 0:
            self._check(self.lib.msr_dense_topk(self.handle, _ptr(q), Q, k, int(max_chunks_per_doc), _ptr(out_doc),
                                                _ptr(out_score), _ptr(out_chunk), _ptr(out_n), self._stream()))
        else:
            self._check(self.lib.msr_dense_topk_within(self.handle, _ptr(q), Q, k, int(max_chunks_per_doc), _ptr(bits), n_sets,
                                                       stride, _ptr(q_set), _ptr(out_doc), _ptr(out_score), _ptr(out_chunk),
                                                       _ptr(out_n), self._stream()))
        return out_doc, out_score, out_chunk, out_n

    def gather_rows(self, rows):
        """rows int [n] chunk row indices -> float32 [n, 768] device tensor: the bound rows as given to the index (not
        normalised), bit for bit, whatever scan_layout the engine holds (msr_gather_rows; a row outside [0, n_chunks) raises)."""
        r = self._dev(np.asarray(rows, np.int64).reshape(-1) if not torch.is_tensor(rows) else rows.reshape(-1), torch.int32)
        n = int(r.numel())
        out = torch.empty((n, DIM), dtype=torch.float32, device=self.device)
        self._check(self.lib.msr_gather_rows(self.handle, _ptr(r), n, _ptr(out), self._stream()))
        return out

    def dense_topk_grouped(self, qvec, group_off, exclude=None, k=10, min_score=None, within=None):
        """Per group of query rows the top k documents by the maximum over the group's rows of the dense score
        (msr_dense_topk_grouped).  qvec float32 [R, 768]; group_off int [G + 1] (group g = rows group_off[g] ..
        group_off[g + 1]); exclude: None or G iterables of document indices never returned for that group; min_score: None or
        a float threshold; within: None, a DocSet (every group) or a list of DocSet / None per group.
        -> (doc [G, k] i32, score [G, k] f32, chunk row [G, k] i32, source row [G, k] i32 (index into qvec), n [G]) device."""
        q = self._dev(qvec, torch.float32).reshape(-1, DIM)
        R = int(q.shape[0])
        goff = np.asarray(group_off, np.int64).reshape(-1)
        G = int(goff.shape[0]) - 1
        if G < 0:
            raise ValueError("group_off needs at least one entry")
        excl = [[] for _ in range(G)] if exclude is None else [list(x) for x in exclude]
        if len(excl) != G:
            raise ValueError(f"exclude: {len(excl)} entries for {G} groups")
        eoff = np.zeros(G + 1, np.int64)
        eoff[1:] = np.cumsum([len(x) for x in excl], dtype=np.int64)
        edoc = np.asarray([int(d) for x in excl for d in x] or [0], np.int64)
        t_goff, t_eoff, t_edoc = self._dev(goff, torch.int32), self._dev(eoff, torch.int32), self._dev(edoc, torch.int32)
        out_doc = torch.empty((G, k), dtype=torch.int32, device=self.device)
        out_score = torch.empty((G, k), dtype=torch.float32, device=self.device)
        out_chunk = torch.empty((G, k), dtype=torch.int32, device=self.device)
        out_src = torch.empty((G, k), dtype=torch.int32, device=self.device)
        out_n = torch.empty((G,), dtype=torch.int32, device=self.device)
        bits, g_set, n_sets, stride = None, None, 0, 0
        if within is not None:
            bits, g_set, n_sets, stride = self.pack_within(within, G)
        ms = -np.inf if min_score is None else float(min_score)
        self._check(self.lib.msr_dense_topk_grouped(self.handle, _ptr(q), R, _ptr(t_goff), G, _ptr(t_eoff), _ptr(t_edoc), int(k),
                                                    C.c_float(ms), _ptr(bits), n_sets, stride, _ptr(g_set), _ptr(out_doc),
                                                    _ptr(out_score), _ptr(out_chunk), _ptr(out_src), _ptr(out_n), self._stream()))
        return out_doc, out_score, out_chunk, out_src, out_n

    def dense_split_max(self, k=100):
        """Most queries one dense_begin / dense_end pair takes (0: this engine cannot split the dense call)."""
        return int(self.lib.msr_dense_split_max(self.handle, int(k)))

    def dense_begin(self, qvec, k=100, k_part=None):
        """First half of dense_topk for a doc-sharded index (msr_dense_topk_begin): -> part float32 [Q] (device): a cosine that
        k_part documents of this shard reach exactly.  The caller takes the minimum over the shards (k_part = ceil(k / shards))
        and hands it to dense_end."""
        q = self._dev(qvec, torch.float32).reshape(-1, DIM)
        Q = int(q.shape[0])
        part = torch.empty((Q,), dtype=torch.float32, device=self.device)
        self._check(self.lib.msr_dense_topk_begin(self.handle, _ptr(q), Q, int(k), int(k_part or k), _ptr(part), self._stream()))
        return part

    def dense_end(self, Q, k=100, bound=None, want_chunk=True, out=None):
        """Second half (msr_dense_topk_end): bound float32 [Q] (device) or None -> (doc, score, chunk row, n) as dense_topk; with
        a bound n may be < k -- every document this shard can contribute to the global top-k.  out: optional (doc, score,
        chunk, n) contiguous tensors of those shapes to write into (row slices of a larger result)."""
        if out is not None:
            out_doc, out_score, out_chunk, out_n = out
            assert tuple(out_doc.shape) == (Q, k) and out_doc.is_contiguous() and out_score.is_contiguous() and out_n.is_contiguous()
        else:
            out_doc = torch.empty((Q, k), dtype=torch.int32, device=self.device)
            out_score = torch.empty((Q, k), dtype=torch.float32, device=self.device)
            out_chunk = torch.empty((Q, k), dtype=torch.int32, device=self.device) if want_chunk else None
            out_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        self._check(self.lib.msr_dense_topk_end(self.handle, int(Q), int(k), _ptr(bound), _ptr(out_doc), _ptr(out_score),
                                                _ptr(out_chunk), _ptr(out_n), self._stream()))
        return out_doc, out_score, out_chunk, out_n

    def enable_bf16(self):
        """Build the bf16 copy of the embeddings used by dense_topk_batched (+7.7 GB at 5 M chunks)."""
        self._check(self.lib.msr_enable_bf16(self.handle, self._stream()))
        torch.cuda.synchronize(self.device)
        self._bf16 = True

    def dense_topk_batched(self, qvec, k=100, max_chunks_per_doc=0, want_chunk=True):
        """Throughput variant of dense_topk: bf16 candidate sweep (up to 128 queries per sweep) + exact f32 rescoring.
        Same outputs; queries whose candidate set overflowed are rerun on the exact f32 scan."""
        q = self._dev(qvec, torch.float32).reshape(-1, DIM)
        Q = int(q.shape[0])
        out_doc = torch.empty((Q, k), dtype=torch.int32, device=self.device)
        out_score = torch.empty((Q, k), dtype=torch.float32, device=self.device)
        out_chunk = torch.empty((Q, k), dtype=torch.int32, device=self.device) if want_chunk else None
        out_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        self._check(self.lib.msr_dense_topk_bf16(self.handle, _ptr(q), Q, k, int(max_chunks_per_doc), _ptr(out_doc),
                                                 _ptr(out_score), _ptr(out_chunk), _ptr(out_n), self._stream()))
        bad = torch.nonzero(out_n < 0).flatten()
        if bad.numel():                                   # (syncs; rare) exact rerun of the overflowed queries
            d, s, c, n = self.dense_topk(q[bad], k=k, max_chunks_per_doc=max_chunks_per_doc, want_chunk=want_chunk)
            out_doc[bad], out_score[bad], out_n[bad] = d, s, n
            if want_chunk:
                out_chunk[bad] = c
        return out_doc, out_score, out_chunk, out_n

    # ------------------------------------------------------------------ rerank / fuse
    def rerank(self, qvec, cand_doc, cand_bm25, cand_n, **params):
        """cand_doc int32 [Q, M] dense indices, cand_bm25 float64 [Q, M], cand_n int32 [Q]
        -> (doc, new_similarity f64, normalised bm25 f64, chunk row, n, rows) device tensors [Q, M] / [Q]."""
        p = dict(RERANK_DEFAULTS)
        p.update(params)
        q = self._dev(qvec, torch.float32).reshape(-1, DIM)
        cand_doc = self._dev(cand_doc, torch.int32)
        cand_bm25 = self._dev(cand_bm25, torch.float64)
        cand_n = self._dev(cand_n, torch.int32)
        Q, M = int(cand_doc.shape[0]), int(cand_doc.shape[1])
        prm = _abi.MsrRerankParams(p["smoothing"], p["max_boost"], p["max_decay"], int(p["max_chunks"]), 0)
        mk = lambda dt: torch.empty((Q, M), dtype=dt, device=self.device)
        out_doc, out_score, out_orig, out_chunk = mk(torch.int32), mk(torch.float64), mk(torch.float64), mk(torch.int32)
        out_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        out_rows = torch.empty((Q,), dtype=torch.int32, device=self.device)
        self._check(self.lib.msr_rerank(self.handle, _ptr(q), Q, _ptr(cand_doc), _ptr(cand_bm25), _ptr(cand_n), M,
                                        C.byref(prm), _ptr(out_doc), _ptr(out_score), _ptr(out_orig),
                                        _ptr(out_chunk), _ptr(out_n), _ptr(out_rows), self._stream()))
        return out_doc, out_score, out_orig, out_chunk, out_n, out_rows

    def rerank_gather(self, qvec, cand_doc_global, cand_n, doc_base=0, row_base=0, max_chunks=10, out=None):
        """Shard-local half of rerank: (cos float32 [Q, M, 10], meta int32 [Q, M, 3]); zeros for foreign docs.
        out: optional (cos, meta) contiguous tensors of those shapes to write into (views of an exchange buffer)."""
        q = self._dev(qvec, torch.float32).reshape(-1, DIM)
        cand = self._dev(cand_doc_global, torch.int32)
        cn = self._dev(cand_n, torch.int32)
        Q, M = int(cand.shape[0]), int(cand.shape[1])
        if out is not None:
            cos, meta = out
            assert cos.is_contiguous() and meta.is_contiguous() and cos.dtype == torch.float32 and meta.dtype == torch.int32
            assert tuple(cos.shape) == (Q, M, _abi.MSR_RERANK_MAX_CHUNKS) and tuple(meta.shape) == (Q, M, 3)
        else:
            cos = torch.empty((Q, M, _abi.MSR_RERANK_MAX_CHUNKS), dtype=torch.float32, device=self.device)
            meta = torch.empty((Q, M, 3), dtype=torch.int32, device=self.device)
        self._check(self.lib.msr_rerank_gather(self.handle, _ptr(q), Q, _ptr(cand), _ptr(cn), M, int(doc_base),
                                               int(row_base), int(max_chunks), _ptr(cos), _ptr(meta), self._stream()))
        return cos, meta

    def rerank_gather_blocks(self, qvec, cand_doc_global, cand_n, blocks, queries_per_block, doc_base=0, row_base=0, max_chunks=10):
        """rerank_gather for ALL queries in one launch, written into `blocks` (int32 [n_blocks, block_words], contiguous: the
        send buffer of the all-to-all): block b = [cos of queries b * qpb .. | their meta | padding] (msr_rerank_gather_blocks)."""
        q = self._dev(qvec, torch.float32).reshape(-1, DIM)
        cand = self._dev(cand_doc_global, torch.int32)
        cn = self._dev(cand_n, torch.int32)
        Q, M = int(cand.shape[0]), int(cand.shape[1])
        assert blocks.is_contiguous() and blocks.dtype == torch.int32 and blocks.dim() == 2
        assert int(blocks.shape[0]) * int(queries_per_block) >= Q
        self._check(self.lib.msr_rerank_gather_blocks(self.handle, _ptr(q), Q, _ptr(cand), _ptr(cn), M, int(doc_base), int(row_base),
                                                      int(max_chunks), _ptr(blocks), int(queries_per_block), int(blocks.shape[1]),
                                                      self._stream()))

    def rerank_combine(self, cos_parts, meta_parts, nq):
        """Join of the gathered halves: cos_parts float32 [G, Qs, M, 10] and meta_parts int32 [G, Qs, M, 3] are views of ONE
        receive buffer (the same stride between parts, each part contiguous); -> (cos [nq, M, 10], meta [nq, M, 3]) of the
        first nq queries, the bitwise OR over the G parts (msr_rerank_combine)."""
        G, M = int(cos_parts.shape[0]), int(cos_parts.shape[2])
        stride = cos_parts.stride(0) * 4 if G > 1 else 0
        assert G == 1 or meta_parts.stride(0) * 4 == stride
        assert cos_parts[0].is_contiguous() and meta_parts[0].is_contiguous()
        cos = torch.empty((nq, M, _abi.MSR_RERANK_MAX_CHUNKS), dtype=torch.float32, device=self.device)
        meta = torch.empty((nq, M, 3), dtype=torch.int32, device=self.device)
        self._check(self.lib.msr_rerank_combine(self.handle, _ptr(cos_parts), _ptr(meta_parts), G, int(stride), int(nq), M,
                                                _ptr(cos), _ptr(meta), self._stream()))
        return cos, meta

    # -- the compact form of the rerank exchange (msretr.h: msr_rerank_plan / _gather_records / _scatter)
    def rerank_plan(self, cand_doc_global, cand_n, shard_bounds, my_shard, queries_per_shard, plan):
        """Fills `plan` (distributed._RerankPlan: counts [N, Q], send_base [Q], send_blk [Q, ceil(M / 8)], recv_off [N, Qs],
        pair [N, N], all int32 on the device) for the merged candidate lists cand_doc_global [Q, M] / cand_n [Q]."""
        cand = self._dev(cand_doc_global, torch.int32)
        cn = self._dev(cand_n, torch.int32)
        Q, M = int(cand.shape[0]), int(cand.shape[1])
        N = int(shard_bounds.numel()) - 1
        assert tuple(plan.counts.shape) == (N, Q) and tuple(plan.send_blk.shape) == (Q, (M + 7) // 8)
        assert tuple(plan.recv_off.shape) == (N, int(queries_per_shard)) and tuple(plan.pair.shape) == (N, N)
        self._check(self.lib.msr_rerank_plan(self.handle, Q, _ptr(cand), _ptr(cn), M, _ptr(shard_bounds), N, int(my_shard),
                                             int(queries_per_shard), _ptr(plan.counts), _ptr(plan.send_base), _ptr(plan.send_blk),
                                             _ptr(plan.recv_off), _ptr(plan.pair), self._stream()))

    def rerank_gather_records(self, qvec, cand_doc_global, cand_n, plan, records, doc_base=0, row_base=0, max_chunks=10):
        """rerank_gather for ALL queries in one launch, as 16-word records of the slots this shard owns, at the places `plan`
        holds (records: int32, at least sum(plan.pair[my]) * 16 words)."""
        q = self._dev(qvec, torch.float32).reshape(-1, DIM)
        cand = self._dev(cand_doc_global, torch.int32)
        cn = self._dev(cand_n, torch.int32)
        Q, M = int(cand.shape[0]), int(cand.shape[1])
        assert records.is_contiguous() and records.dtype == torch.int32
        self._check(self.lib.msr_rerank_gather_records(self.handle, _ptr(q), Q, _ptr(cand), _ptr(cn), M, int(doc_base), int(row_base),
                                                       int(max_chunks), _ptr(plan.send_base), _ptr(plan.send_blk), _ptr(records),
                                                       int(records.numel()) // 16, self._stream()))

    def rerank_scatter(self, records, plan, first_query, nq, M):
        """The received records of my queries [first_query, first_query + nq) -> (cos [nq, M, 10], meta [nq, M, 3])."""
        N, Q = int(plan.counts.shape[0]), int(plan.counts.shape[1])
        cos = torch.empty((nq, M, _abi.MSR_RERANK_MAX_CHUNKS), dtype=torch.float32, device=self.device)
        meta = torch.empty((nq, M, 3), dtype=torch.int32, device=self.device)
        self._check(self.lib.msr_rerank_scatter(self.handle, _ptr(records), int(records.numel()) // 16, _ptr(plan.counts), _ptr(plan.recv_off), N, Q,
                                                int(plan.recv_off.shape[1]), int(first_query), int(nq), int(M), _ptr(cos), _ptr(meta),
                                                self._stream()))
        return cos, meta

    def rerank_fuse(self, cand_doc_global, cand_bm25, cand_n, cos, meta, **params):
        p = dict(RERANK_DEFAULTS)
        p.update(params)
        cand = self._dev(cand_doc_global, torch.int32)
        bm = self._dev(cand_bm25, torch.float64)
        cn = self._dev(cand_n, torch.int32)
        Q, M = int(cand.shape[0]), int(cand.shape[1])
        prm = _abi.MsrRerankParams(p["smoothing"], p["max_boost"], p["max_decay"], int(p["max_chunks"]), 0)
        mk = lambda dt: torch.empty((Q, M), dtype=dt, device=self.device)
        out_doc, out_score, out_orig, out_chunk = mk(torch.int32), mk(torch.float64), mk(torch.float64), mk(torch.int32)
        out_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        out_rows = torch.empty((Q,), dtype=torch.int32, device=self.device)
        cos, meta = cos.contiguous(), meta.contiguous()      # (named: a copy must outlive the call that reads it)
        self._check(self.lib.msr_rerank_fuse(self.handle, Q, _ptr(cand), _ptr(bm), _ptr(cn), M, _ptr(cos),
                                             _ptr(meta), C.byref(prm), _ptr(out_doc), _ptr(out_score),
                                             _ptr(out_orig), _ptr(out_chunk), _ptr(out_n), _ptr(out_rows),
                                             self._stream()))
        return out_doc, out_score, out_orig, out_chunk, out_n, out_rows

    # ------------------------------------------------------------------ response assembly on the device
    def bind_doc_domains(self, domain):
        """domain int32 [N_global]: domain id of every document (equal ids = same urlparse(url).netloc.lower()), -1 = a
        document the response models reject (NULL title / url / text, reranker_api.py:376-397).  None unbinds."""
        t = None if domain is None else self._dev(domain, torch.int32)
        self._t["doc_domain"] = t
        self._check(self.lib.msr_bind_doc_domains(self.handle, _ptr(t), 0 if t is None else int(t.numel()), self._stream()))

    def diversify(self, fused, top_k=100, relevance_threshold=0.8, diversification=True):
        """fused = (doc, score, orig, chunk, n, ...) of rerank / rerank_fuse -> (doc, score f64, orig f64, chunk, n): the final
        list of every query after reranker_api.py:178-236 (or, diversification=False, its first top_k accepted entries)."""
        # (named: the copy of a non-contiguous input must outlive the call -- as a temporary its block went back to the
        # allocator at once and the next input's copy was written over it before the kernel ran)
        doc, score, orig, chunk, n = (t.contiguous() for t in fused[:5])
        Q, M = int(doc.shape[0]), int(doc.shape[1])
        mk = lambda dt: torch.empty((Q, M), dtype=dt, device=self.device)
        o_doc, o_score, o_orig, o_chunk = mk(torch.int32), mk(torch.float64), mk(torch.float64), mk(torch.int32)
        o_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        self._check(self.lib.msr_diversify(self.handle, Q, _ptr(doc), _ptr(score), _ptr(orig),
                                           _ptr(chunk), _ptr(n), M, int(top_k),
                                           C.c_double(relevance_threshold), 1 if diversification else 0, _ptr(o_doc),
                                           _ptr(o_score), _ptr(o_orig), _ptr(o_chunk), _ptr(o_n), self._stream()))
        return o_doc, o_score, o_orig, o_chunk, o_n

    # ------------------------------------------------------------------ shard merge
    def merge_topk(self, docs, scores, ns, k):
        """docs int32 [G, Q, k] GLOBAL indices, scores f32/f64 [G, Q, k], ns int32 [G, Q] -> merged top-k."""
        G, Q = int(docs.shape[0]), int(docs.shape[1])
        bits = 64 if scores.dtype == torch.float64 else 32
        out_doc = torch.empty((Q, k), dtype=torch.int32, device=self.device)
        out_score = torch.empty((Q, k), dtype=scores.dtype, device=self.device)
        out_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        docs, scores, ns = docs.contiguous(), scores.contiguous(), ns.contiguous()      # (named: see diversify)
        self._check(self.lib.msr_merge_topk(self.handle, _ptr(docs), _ptr(scores),
                                            _ptr(ns), G, Q, k, bits, _ptr(out_doc), _ptr(out_score),
                                            _ptr(out_n), self._stream()))
        return out_doc, out_score, out_n

    def merge_gathered(self, ex, doc, score, n, payload, k):
        """Merge the `world` records of an all-gather IN PLACE (distributed._Exchange): the kernel reads segment `doc` /
        `score` / `n` (/ `payload`) of every rank's record through a byte stride.  -> (doc, score, n, payload | None)."""
        sc0 = ex.part(0, score)
        Q = ex.Q
        bits = 64 if sc0.dtype == torch.float64 else 32
        out_doc = torch.empty((Q, k), dtype=torch.int32, device=self.device)
        out_score = torch.empty((Q, k), dtype=sc0.dtype, device=self.device)
        out_n = torch.empty((Q,), dtype=torch.int32, device=self.device)
        out_pay = torch.empty((Q, k), dtype=torch.int32, device=self.device) if payload else None
        self._check(self.lib.msr_merge_topk_payload(
            self.handle, _ptr(ex.part(0, doc)), _ptr(sc0), _ptr(ex.part(0, n)), _ptr(ex.part(0, payload)) if payload else _ptr(None),
            ex.world, ex.record, Q, k, bits, _ptr(out_doc), _ptr(out_score), _ptr(out_n), _ptr(out_pay), self._stream()))
        return out_doc, out_score, out_n, out_pay

    # ------------------------------------------------------------------ timing hooks (bench.py)
    def set_timing(self, on):
        self._check(self.lib.msr_set_timing(self.handle, 1 if on else 0))

    def kernel_time_ms(self, which):
        ms, n = C.c_float(), C.c_int32()
        self._check(self.lib.msr_kernel_time_ms(self.handle, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value
