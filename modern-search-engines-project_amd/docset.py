"""Document sets: restrict a search to part of the corpus (a `site:` search, a caller's access list, a takedown).

    R = DocSet.from_sites(ix, ["uni-tuebingen.de"])          # every document whose URL's domain is, or ends in, .site
    R = DocSet.from_doc_ids(ix, allowed_ids) - DocSet.from_doc_ids(ix, taken_down)
    retriever.search(query, within=R)                        # also BM25.search(..., within=R), quick_search(..., within=R)

A DocSet is a set of dense document indices [0, N) of ONE CorpusIndex: using it with another index (after
Retriever.update_index, index_build.remove_documents or bm25_add_token_ids) raises ValueError.  The restriction acts where the
cut happens -- inside the BM25 scoring kernel's candidate emission and inside the dense select (msr_bm25_topk_within /
msr_dense_topk_within) -- so the allowed documents ranked behind the whole corpus's top k are found; filtering a result
after the cut would lose them.  The device form is a bitset of uint32 words: document d is bit d & 31 of word d >> 5.
"""
import weakref
from urllib.parse import urlsplit

import numpy as np


def _n_words(n_docs):
    return (int(n_docs) + 31) // 32


def url_host(url):
    """The host of a URL as site matching sees it: urlparse(url).netloc lower-cased, without user info (`user@`) and without
    a port; None for a missing URL, one that does not parse, or one without a host."""
    if not url:
        return None
    try:
        net = urlsplit(url).netloc
    except Exception:
        return None
    host = net.rsplit("@", 1)[-1].lower()
    if host.startswith("["):                         # [IPv6]:port
        host = host[:host.find("]") + 1] if "]" in host else host
    elif ":" in host:
        head, tail = host.rsplit(":", 1)
        if tail.isdigit() or tail == "":
            host = head
    return host or None


def normalise_sites(sites):
    """The canonical form of a list of sites: stripped, lower case, without leading / trailing dots, duplicates removed,
    sorted -- equal lists give equal tuples (a cache key)."""
    if isinstance(sites, str):
        sites = [sites]
    return tuple(sorted({str(x).strip().lower().strip(".") for x in sites if x and str(x).strip().strip(".")}))


def _host_table(ix):
    """(host id int32 [N] (-1: no host), list of the distinct hosts) of an index's URLs: built once per index (one parse per
    URL) and kept on the index while its `urls` list is the same object of the same length."""
    urls = ix.urls
    got = getattr(ix, "_docset_hosts", None)
    if got is not None and got[0] is urls and got[1] == len(urls):
        return got[2], got[3]
    ids, hosts = {}, []
    out = np.full(len(urls), -1, np.int32)
    for i, u in enumerate(urls):
        h = url_host(u)
        if h is not None:
            j = ids.get(h)
            if j is None:
                j = ids[h] = len(hosts)
                hosts.append(h)
            out[i] = j
    ix._docset_hosts = (urls, len(urls), out, hosts)
    return out, hosts


def pack_bits(mask):
    """bool [N] -> uint32 [ceil(N / 32)]: document d is bit d & 31 of word d >> 5 (bits at or above N are 0)."""
    mask = np.asarray(mask, bool).reshape(-1)
    W = _n_words(len(mask))
    by = np.packbits(mask, bitorder="little")
    out = np.zeros(W * 4, np.uint8)
    out[:len(by)] = by
    return out.view("<u4").astype(np.uint32)


class DocSet:
    """A set of documents of one CorpusIndex (see the module's doc)."""

    def __init__(self, ix, mask):
        mask = np.asarray(mask, bool).reshape(-1)
        if len(mask) != ix.n_docs:
            raise ValueError(f"DocSet: mask of {len(mask)} entries for an index of {ix.n_docs} documents")
        self._ix = weakref.ref(ix)
        self.n_docs = int(ix.n_docs)
        self.mask = mask
        self.mask.setflags(write=False)
        self._words = None
        self._dev = {}
        self.not_found = 0

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_mask(cls, ix, mask):
        """mask: bool [N] over the dense document indices of `ix`."""
        return cls(ix, np.array(mask, bool, copy=True))

    @classmethod
    def from_doc_ids(cls, ix, ids):
        """External doc_ids; ids the index lacks are counted in `.not_found`, not raised (as in remove_documents)."""
        from .index import _np
        ids = np.asarray(_np(ids) if not isinstance(ids, (list, tuple)) else ids, np.int64).reshape(-1)
        have = np.asarray(_np(ix.doc_ids), np.int64)
        N = len(have)
        mask = np.zeros(N, bool)
        if N and len(ids):
            pos = np.minimum(np.searchsorted(have, ids), N - 1)
            found = have[pos] == ids
            mask[pos[found]] = True
            nf = int((~found).sum())
        else:
            nf = len(ids)
        out = cls(ix, mask)
        out.not_found = nf
        return out

    @classmethod
    def from_sites(cls, ix, sites):
        """Documents whose URL's host (url_host: urlparse(url).netloc lower-cased, without user info and port) equals a site or
        ends with "." + site; sites are host names (no port), compared case-insensitively, without leading / trailing dots
        (normalise_sites).  A document without a URL, or whose URL does not parse or has no host, never matches.  The URLs are
        parsed once per index (kept on it); a call then costs one test per DISTINCT host plus a gather over the documents."""
        want = normalise_sites(sites)
        N = ix.n_docs
        if ix.urls is None or not want:
            return cls(ix, np.zeros(N, bool))
        host_id, hosts = _host_table(ix)
        suffixes = tuple("." + w for w in want)
        exact = set(want)
        hit = np.array([h in exact or h.endswith(suffixes) for h in hosts] + [False], bool)
        return cls(ix, hit[host_id])                  # (host id -1 picks the trailing False)

    @classmethod
    def from_words(cls, ix, words):
        """The inverse of words(): uint32 (or int32) [>= ceil(N / 32)] bitset words -> the set (document d = bit d & 31 of word
        d >> 5), e.g. a row of a DeviceSets copied back.  Words past ceil(N / 32) are ignored; a bit at or above N inside the
        last word raises ValueError (no document has that number)."""
        N, W = int(ix.n_docs), _n_words(ix.n_docs)
        w = np.ascontiguousarray(np.asarray(words).reshape(-1)).view(np.uint32)
        if len(w) < W:
            raise ValueError(f"DocSet.from_words: {len(w)} words for an index of {N} documents ({W} words)")
        bits = np.unpackbits(w[:W].astype("<u4").view(np.uint8), bitorder="little")
        if bits[N:].any():
            raise ValueError(f"DocSet.from_words: a bit at or above n_docs = {N} is set")
        return cls(ix, bits[:N].astype(bool))

    # ------------------------------------------------------------------ binding
    @property
    def index(self):
        return self._ix()

    def check(self, ix):
        """Raise ValueError unless this set belongs to `ix` (the same object, with the same number of documents)."""
        if self._ix() is not ix or ix.n_docs != self.n_docs:
            raise ValueError("DocSet: built for another index (the index was updated or replaced since): rebuild it from the "
                             "index being searched")

    # ------------------------------------------------------------------ set algebra
    def _same(self, other):
        if not isinstance(other, DocSet):
            return NotImplemented
        if other._ix() is not self._ix() or other.n_docs != self.n_docs:
            raise ValueError("DocSet: operands belong to different indexes")
        return other

    def _new(self, mask):
        return DocSet(self._ix(), mask)

    def __and__(self, other):
        o = self._same(other)
        return o if o is NotImplemented else self._new(self.mask & o.mask)

    def __or__(self, other):
        o = self._same(other)
        return o if o is NotImplemented else self._new(self.mask | o.mask)

    def __sub__(self, other):
        o = self._same(other)
        return o if o is NotImplemented else self._new(self.mask & ~o.mask)

    def __invert__(self):
        return self._new(~self.mask)                 # the complement within [0, N)

    def __len__(self):
        return int(self.mask.sum())

    def __contains__(self, d):
        return 0 <= int(d) < self.n_docs and bool(self.mask[int(d)])

    def __eq__(self, other):
        return isinstance(other, DocSet) and other._ix() is self._ix() and np.array_equal(self.mask, other.mask)

    __hash__ = object.__hash__

    def __repr__(self):
        return f"DocSet({len(self)} of {self.n_docs} documents)"

    def indices(self):
        """int64 [len(self)]: the dense document indices, ascending."""
        return np.nonzero(self.mask)[0]

    # ------------------------------------------------------------------ device form
    def words(self):
        """uint32 [ceil(N / 32)]: the bitset (document d = bit d & 31 of word d >> 5)."""
        if self._words is None:
            self._words = pack_bits(self.mask)
            self._words.setflags(write=False)
        return self._words

    def to(self, device):
        """The bitset as an int32 tensor [ceil(N / 32)] on `device` (the uint32 words' bits; cached per device)."""
        import torch
        key = str(torch.device(device))
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = torch.from_numpy(self.words().view(np.int32).copy()).to(device)
        return t


def pack_within(within, n_queries, ix):
    """The host form of a restricted call: within = None, one DocSet (every query), or a list of n_queries DocSet / None.
    -> (words uint32 [n_sets, stride], q_set int32 [n_queries], n_sets, stride): identical sets are stacked once, None is -1,
    stride = max(1, ceil(N / 32)).  n_sets == 0 means the unrestricted call.  Every DocSet is checked against `ix`."""
    stride = max(1, _n_words(ix.n_docs))
    if within is None:
        return np.zeros((0, stride), np.uint32), np.full(n_queries, -1, np.int32), 0, stride
    per_q = [within] * n_queries if isinstance(within, DocSet) else list(within)
    if len(per_q) != n_queries:
        raise ValueError(f"within: {len(per_q)} entries for {n_queries} queries")
    rows, row_of_set, row_of_bits, q_set = [], {}, {}, np.full(n_queries, -1, np.int32)
    for q, s in enumerate(per_q):
        if s is None:
            continue
        r = row_of_set.get(id(s))
        if r is None:                                # (each distinct object is checked and compared once)
            if not isinstance(s, DocSet):
                raise TypeError("within: a DocSet or None per query")
            s.check(ix)
            w = s.words()
            key = w.tobytes()
            r = row_of_bits.get(key)
            if r is None:
                r = row_of_bits[key] = len(rows)
                rows.append(w)
            row_of_set[id(s)] = r
        q_set[q] = r
    words = np.zeros((len(rows), stride), np.uint32)
    for r, w in enumerate(rows):
        words[r, :len(w)] = w
    return words, q_set, len(rows), stride


class DeviceSets:
    """Document sets that live on the device, as DeviceEngine.term_sets builds them from posting lists (msr_term_sets): the four
    fields DeviceEngine.pack_within returns -- bits int32 [n_sets, stride] (rows in the layout above), q_set int32 [Q] (query
    q's row; -1 = every document), n_sets, stride -- tied to the index they were built for.  Pass it as `within=` to
    bm25_topk / dense_topk / dense_topk_grouped / the Retriever's chain; after a rebind or update_index it is refused like a
    DocSet.  Unpacks as (bits, q_set, n_sets, stride).  `layout` says what the rows are when the producer has more than one
    kind: None (term_sets: base rows, then one row per distinct operator list), or DeviceEngine.phrase_sets' (T, P, C) -- T rows
    as term_sets makes them, then P verified (phrase, candidate row) pairs, then C rows, one per query with phrases; n_sets =
    T + P + C; `n_near` = how many of the P rows are proximity rows (text.Near; they stand behind the exact phrases' rows).  A
    part taken with queries() names the same rows and keeps the layout."""

    def __init__(self, ix, bits, q_set, n_sets, stride):
        self._ix = weakref.ref(ix)
        self.n_docs = int(ix.n_docs)
        self.bits, self.q_set, self.n_sets, self.stride = bits, q_set, int(n_sets), int(stride)
        self.layout = None
        self.n_near = 0

    def __iter__(self):
        return iter((self.bits, self.q_set, self.n_sets, self.stride))

    def __len__(self):
        return int(self.q_set.shape[0])

    @property
    def index(self):
        return self._ix()

    def check(self, ix):
        """Raise ValueError unless these sets belong to `ix` (the same object, with the same number of documents)."""
        if self._ix() is not ix or ix.n_docs != self.n_docs:
            raise ValueError("DocSet: built for another index (the index was updated or replaced since): rebuild it from the "
                             "index being searched")

    def queries(self, a, b):
        """The sets of queries a .. b: the same rows, their part of q_set (nothing is copied) -- for a caller that works through
        the queries in chunks."""
        part = DeviceSets.__new__(DeviceSets)
        part.__dict__.update(self.__dict__)
        part.q_set = self.q_set[a:b]
        return part

    def docset(self, q):
        """Query q's set as a DocSet of the index (one row copied back): for set algebra, counting, a look at the members."""
        ix = self._ix()
        if ix is None:
            raise ValueError("DocSet: built for another index (the index was updated or replaced since): rebuild it from the "
                             "index being searched")
        r = int(self.q_set[q])
        if r == -1:
            return DocSet(ix, np.ones(self.n_docs, bool))
        if r < 0 or r >= self.n_sets:
            return DocSet(ix, np.zeros(self.n_docs, bool))
        return DocSet.from_words(ix, self.bits[r].cpu().numpy())
