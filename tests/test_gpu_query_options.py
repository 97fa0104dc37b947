"""The query options all at once, through the public API only: a batch equals its queries one by one, and chunking the
final lists changes nothing.  No reference implementation here: each side of an equality is the engine's own answer (the
options against a CPU oracle: test_gpu_options_oracle.py)."""
import numpy as np
import pytest
import torch

from msretr.docset import DocSet
from msretr.index import _np
from msretr.index_build import attach_tokens
from msretr.retriever import Retriever
from msretr.synthetic import synthetic_corpus
from msretr.text import Near, preprocess_query, simple_tokenize
from options_cases import _streams, _word

pytestmark = pytest.mark.gpu

N_DOCS = 2000
HOSTS = ["uni-tuebingen.de", "www.tuebingen.de", "tuebingen.de", "example.org"] + [f"s{i}.example.net" for i in range(40)]


@pytest.fixture(scope="module")
def site():
    """test_gpu_facets' corpus: a vocabulary, a forward index, URLs and texts; eight queries fill the engine."""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix = synthetic_corpus(N_DOCS, n_chunks=6000, n_terms=3000, seed=31)
    rng = np.random.default_rng(32)
    w = 1.0 / (1.0 + np.arange(len(HOSTS))) ** 1.2
    host = rng.choice(len(HOSTS), N_DOCS, p=w / w.sum())
    ids = _np(ix.doc_ids)
    ix.urls = [None if d % 97 == 5 else f"https://{HOSTS[host[d]]}/doc{int(ids[d])}" for d in range(N_DOCS)]
    ix._url_group = None
    df = np.diff(_np(ix.term_off).astype(np.int64))
    mid = [int(t) for t in np.argsort(-df, kind="stable")[100:140]]
    assert 0 not in mid and df[mid[0]] < N_DOCS // 2
    names = {t: _word(t) for t in range(ix.n_terms)}
    names.update({0: "tübingen", mid[20]: "mensa", mid[21]: "bibliothek", mid[22]: "bibliothekar", mid[23]: "universität",
                  mid[24]: "unibibliothek"})
    ix.vocab = {name: t for t, name in names.items()}
    off, tok = _streams(ix)
    attach_tokens(ix, off, tok)
    ix.titles = [""] * N_DOCS                                # (snippets are cut from the page: its words are its indexed stream)
    ix.texts = [" ".join(names[int(t)] for t in tok[off[d]:off[d + 1]]) for d in range(N_DOCS)]
    qv = torch.randn((8, 768), generator=torch.Generator().manual_seed(33)).numpy()
    r = Retriever(indexer=ix, max_queries=8, max_k=1000)
    wa, wb, wc = _word(mid[1]), _word(mid[9]), _word(mid[3])
    w1, w2 = _word(30), _word(31)                # frequent words with adjacent ids stand next to each other where both are
    # every text syntax between them: +w -w "a b" -"a b" "a b"~2 "a b"~>1 uni* t?bingen, a misspelt word, an unknown word
    queries = [f"mensa +{wa} -{wb}", f'mensa "{w1} {w2}"', f'{wa} -"{w1} {w2}"', f'bibliothek "{w2} {w1}"~2',
               f'"{w1} {w2}"~>1 {wb}', "uni* mensa", "t?bingen mensaa bibliothekk", "zzzzqqqq bibliothek* mensa"]
    uni = DocSet.from_sites(ix, ["uni-tuebingen.de", "tuebingen.de", "example.org"])
    net = DocSet.from_sites(ix, ["example.net"])
    lists = {"within": [None, uni, None, None, net, uni, None, None],
             "must": [[], [wc], [wc], [wc], [], ["mensaa"], [], []],               # (queries 2 and 3: the same conditions)
             "must_not": [[], [], [], [], [wa], [], [], []],
             "must_phrases": [[f"{w1} {w2}"], [], [[w1, w2]], [[w1, w2]], [], [Near(f"{w2} {w1}", 3)], [], []],
             "must_not_phrases": [[], [], [], [], [], [], [Near([w1, w2], 0, ordered=True)], []],
             "patterns": [None, ["bib*"], None, None, ["Uni*", "?ensa"], None, [], ["w*"]]}
    yield ix, qv, r, queries, lists
    r.engine.close()


EXTRAS = ("corrections", "corrected_query", "expansions", "hits", "facets", "facet_values")


@pytest.mark.parametrize("mode", ["lexical", "hybrid"])
def test_batch_equals_one_by_one(site, mode):
    ix, qv, r, queries, lists = site
    on = dict(mode=mode, dense_k=40, operators=True, proximity=True, fuzzy=True, wildcards=True, max_expansions=5, snippets=True,
              snippet_tokens=12, facets=True, facet_by="host", facet_limit=7)
    batch = r.search_batch(queries, query_embeddings=qv, query_ids=[f"q{q}" for q in range(8)], **lists, **on)
    assert len(batch) == 8 and sum(len(rows) > 0 for rows in batch) >= 6
    assert any(b.corrections for b in batch) and any(b.expansions for b in batch) and any(b.hits for b in batch)
    assert batch[5].expansions["uni*"]["terms"] and batch[6].expansions["t?bingen"]["terms"] == ["tübingen"]
    assert batch[6].corrections == {"mensaa": "mensa", "bibliothekk": "bibliothek"} and batch[5].corrections == {"mensaa": "mensa"}
    for q in range(8):
        one = r.search(queries[q], query_embedding=qv[q], query_id=f"q{q}", **{k: v[q] for k, v in lists.items()}, **on)
        assert list(batch[q]) == list(one), q
        for name in EXTRAS:
            assert getattr(batch[q], name) == getattr(one, name), (q, name)


@pytest.mark.parametrize("mode", ["lexical", "hybrid"])
def test_chunking_changes_nothing(site, mode):
    ix, qv, r, queries, lists = site
    terms = [simple_tokenize(preprocess_query(q)) for q in queries]
    ids = [ix.term_ids(t) for t in terms]
    pats = [list(p or ()) for p in lists["patterns"]]
    pats[5], pats[6] = ["uni*"], ["t?bingen"]
    kw = {k: lists[k] for k in ("within", "must", "must_not")}
    for k in ("must_phrases", "must_not_phrases"):           # (here a phrase is a list of terms: there is no text to tokenise)
        kw[k] = [[p.split() if isinstance(p, str) else p for p in ps] for ps in lists[k]]
    if mode == "hybrid":
        kw.update(mode="hybrid", dense_k=40, with_source=True)

    def run(chunk):
        dicts = {"fuzzy": {"terms": terms}, "wildcards": {"patterns": pats, "limit": 4}, "facets": {"by": "domain", "limit": 5}}
        return r.final_lists(ids, qv, 1000, chunk=chunk, **kw, **dicts), dicts
    want, wd = run(None)
    assert int((want[3] > 0).sum()) >= 6 and any(wd["fuzzy"]["corrections"]) and any(wd["wildcards"]["expansions"])
    assert sum(int(h) for h in wd["facets"]["hits"]) > 0
    for chunk in (2, 3):                          # both leave a short last chunk; 3 splits queries 2 and 3
        got, gd = run(chunk)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a, b), chunk
        for d, keys in (("fuzzy", ("corrections", "ids")), ("wildcards", ("expansions", "ids")),
                        ("facets", ("hits", "top_value", "top_count"))):
            for key in keys:
                assert len(gd[d][key]) == 8
                assert [np.asarray(x).tolist() for x in gd[d][key]] == [np.asarray(x).tolist() for x in wd[d][key]], (chunk, d, key)
