"""What the three fields derived from the `text` column share (rag_fin_amd/text_fields.py), through the store's
public surface and over the doubles of the per-field CPU tests: one life cycle (declare, build lazily, follow
appends and deletes, drop, undeclare) and one table of refusals per field -- the exact message of every argument a
search of the field refuses, and which message wins when two hold at once -- run through search() and, where
hybrid_search checks the same thing, through an arm."""
import numpy as np
import pytest

from rag_fin_amd import late_interaction as late
from rag_fin_amd import store as store_mod
from rag_fin_amd.hybrid import AnnSearchRequest, RRFRanker
from rag_fin_amd.ranker import BoostRanker
from test_hybrid_surface_cpu import TEXTS, FakeIndex, FakeSparse, HostStore, fake_fuse
from test_late_interaction_cpu import FakeColBERT, FakeTokenField, fake_maxsim
from test_sparse_encoder_cpu import FakeSparseEncoder

SPARSE, LEARNED, TOKENS = "sparse", "sparse_embedding", "token_embeddings"
SPEC = {SPARSE: {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "BM25"},
        LEARNED: {"index_type": "SPARSE_INVERTED_INDEX", "metric_type": "IP"},
        TOKENS: {"index_type": "EMB_LIST_FLAT", "metric_type": "MAX_SIM_IP"}}
ENCODER = {SPARSE: None, LEARNED: FakeSparseEncoder, TOKENS: FakeColBERT}
VEC = np.ones((1, 8), dtype=np.float32)
COS = {"metric_type": "COSINE"}
QUERY = ["eps q1"]


def metric(name, **more):
    return dict({"metric_type": SPEC[name]["metric_type"]}, **more)


def declare(st, name):
    enc = ENCODER[name]
    st.create_index(name, SPEC[name], **({} if enc is None else {"encoder": enc()}))


def make_store(texts=TEXTS, fields=(SPARSE, LEARNED, TOKENS)):
    n = len(texts)
    st = HostStore("c", dim=8, capacity=64, index=FakeIndex(capacity=64))
    st.add([f"k{i}" for i in range(n)], list(texts), np.ones((n, 8), dtype=np.float32), [f"Q{i % 2}" for i in range(n)],
           ["a"] * n, ["s"] * n, [float(i) for i in range(n)])
    for name in fields:
        declare(st, name)
    return st


# ---- refusals: (what is wrong, the message of search(), the message of a hybrid_search arm or None) ---------------
# "what is wrong" overrides the good call search(QUERY, name, {"metric_type": ...}, limit=3); declared=False: a store
# without the field; iterator=True: search_iterator.  None for the arm: hybrid_search has no such argument, or an
# AnnSearchRequest cannot carry it.
ARM_LIST = "hybrid_search: an arm takes one expr string, not a list (per-query filters)"
ARM_LIMIT = "hybrid_search: an arm's limit is at most 64, got 65"
WINDOW = "offset + limit must be an integer window of at most 16384 (got offset = 2, limit = 0)"
RANKER_LIST = "boosted search (ranker) cannot be combined with per-query filters (a list expr)"
BOOST = BoostRanker('period == "Q0"', 2.0)
LIST_EXPR = ['period == "Q0"']

NO_SPARSE = "no sparse index: call create_index('sparse', {'index_type': 'SPARSE_INVERTED_INDEX', 'metric_type': 'BM25'}) first"
SPARSE_DATA = "the sparse field is searched with query strings (a list of str), not with vectors"
SPARSE_METRIC = "the sparse field is searched with metric_type BM25, search asked for COSINE"
SPARSE_RANGE = "BM25 search (anns_field='sparse') has no range form (radius / range_filter)"
SPARSE_OFFSET = "offset has no BM25 (anns_field='sparse'), grouping (group_by_field) or MMR (mmr_lambda) form"
SPARSE_FORMS = "BM25 search (anns_field='sparse') has no grouping and no MMR form"

NO_LEARNED = ("no sparse_embedding index: call create_index('sparse_embedding', {'index_type': "
              "'SPARSE_INVERTED_INDEX', 'metric_type': 'IP'}, encoder=...) first")
LEARNED_DATA = ("the sparse_embedding field is searched with query strings, a scipy sparse matrix or a "
                "list of {term_id: weight} dicts")
LEARNED_METRIC = "the sparse_embedding field is searched with metric_type IP, search asked for BM25"
LEARNED_RANGE = "learned sparse search (anns_field='sparse_embedding') has no range form (radius / range_filter)"
LEARNED_FORMS = "learned sparse search (anns_field='sparse_embedding') has no offset, grouping or MMR form"
LEARNED_ARM_OFFSET = "learned sparse search (anns_field='sparse_embedding') takes no offset"

NO_TOKENS = ("no token_embeddings index: call create_index('token_embeddings', {'index_type': "
             "'EMB_LIST_FLAT', 'metric_type': 'MAX_SIM_IP'}, encoder=...) first")
TOKENS_DATA = "the token_embeddings field is searched with query strings or a list of [n_tok, D] arrays"
TOKENS_METRIC = "the token_embeddings field is searched with metric_type MAX_SIM_IP, search asked for IP"
TOKENS_RANGE = "late-interaction search (anns_field='token_embeddings') has no range form (radius / range_filter)"
TOKENS_FORMS = "late-interaction search (anns_field='token_embeddings') has no offset, grouping or MMR form"
TOKENS_ARM_OFFSET = "late-interaction search (anns_field='token_embeddings') takes no offset"
TOKENS_LIMIT = "late-interaction search (anns_field='token_embeddings'): limit must be an integer >= 1"
TOKENS_BIG = "late-interaction search (anns_field='token_embeddings'): limit = 65 > 64"

PARAMS = "search: param['params'] must be a dict"
LIMIT = "limit must be an integer >= 1"

REFUSALS = {
    SPARSE: [
        (dict(declared=False), NO_SPARSE, NO_SPARSE),
        (dict(param=COS), SPARSE_METRIC, SPARSE_METRIC),
        (dict(param=metric(SPARSE, params=3)), PARAMS, PARAMS),
        (dict(param=metric(SPARSE, params={"radius": 1.0})), SPARSE_RANGE, SPARSE_RANGE),
        (dict(param=metric(SPARSE, params={"range_filter": 1.0})), SPARSE_RANGE, SPARSE_RANGE),
        (dict(offset=2), SPARSE_OFFSET, None),
        (dict(param=metric(SPARSE, offset=2)), SPARSE_OFFSET, None),
        (dict(limit=0), LIMIT, None),
        (dict(limit=True), LIMIT, None),
        (dict(limit=65), "BM25 search: limit = 65 > 64 (the sparse arm is not paged)", ARM_LIMIT),
        (dict(data=VEC), SPARSE_DATA, SPARSE_DATA),
        (dict(data=[[1.0, 2.0]]), SPARSE_DATA, SPARSE_DATA),
        (dict(expr=LIST_EXPR), "per-query filters (a list expr) have no BM25 form (anns_field='sparse')", ARM_LIST),
        (dict(ranker=BOOST), "boosted search (ranker) has no BM25 form (anns_field='sparse')", None),
        (dict(group_by_field="period"), SPARSE_FORMS, None),
        (dict(mmr_lambda=0.5), SPARSE_FORMS, None),
        (dict(mmr_fetch_k=20), SPARSE_FORMS, None),
        (dict(iterator=True), "search_iterator: unknown vector field 'sparse' (only 'embedding')", None),
        # two at once
        (dict(data=VEC, param=COS), SPARSE_DATA, SPARSE_DATA),                       # vectors before the metric
        (dict(data=VEC, declared=False), NO_SPARSE, NO_SPARSE),
        (dict(param=COS, limit=65), SPARSE_METRIC, ARM_LIMIT),
        (dict(param=metric(SPARSE, params={"radius": 1.0}), limit=0), SPARSE_RANGE, None),
        (dict(offset=2, group_by_field="period"), SPARSE_OFFSET, None),
        (dict(offset=2, limit=0), WINDOW, None),
        (dict(group_by_field="period", declared=False), SPARSE_FORMS, None),
        (dict(ranker=BOOST, expr=LIST_EXPR), RANKER_LIST, None),
    ],
    LEARNED: [
        (dict(declared=False), NO_LEARNED, NO_LEARNED),
        (dict(param={"metric_type": "BM25"}), LEARNED_METRIC, LEARNED_METRIC),
        (dict(param=metric(LEARNED, params=3)), PARAMS, PARAMS),
        (dict(param=metric(LEARNED, params={"radius": 1.0})), LEARNED_RANGE, LEARNED_RANGE),
        (dict(param=metric(LEARNED, params={"range_filter": 1.0})), LEARNED_RANGE, LEARNED_RANGE),
        (dict(offset=2), LEARNED_FORMS, None),
        (dict(param=metric(LEARNED, offset=2)), LEARNED_FORMS, LEARNED_ARM_OFFSET),
        (dict(limit=0), LIMIT, None),
        (dict(limit=True), LIMIT, None),
        (dict(limit=65), "learned sparse search: limit = 65 > 64 (the sparse arm is not paged)", ARM_LIMIT),
        (dict(data=VEC), LEARNED_DATA, LEARNED_DATA),
        (dict(data=[[1.0, 2.0]]), LEARNED_DATA, LEARNED_DATA),
        (dict(expr=LIST_EXPR), "per-query filters (a list expr) have no learned sparse form (anns_field='sparse_embedding')",
         ARM_LIST),
        (dict(ranker=BOOST), "boosted search (ranker) has no learned sparse form (anns_field='sparse_embedding')", None),
        (dict(group_by_field="period"), LEARNED_FORMS, None),
        (dict(mmr_lambda=0.5), LEARNED_FORMS, None),
        (dict(mmr_fetch_k=20), LEARNED_FORMS, None),
        (dict(iterator=True), "search_iterator: unknown vector field 'sparse_embedding' (only 'embedding')", None),
        # two at once
        (dict(data=VEC, param={"metric_type": "BM25"}), LEARNED_METRIC, LEARNED_METRIC),   # the data is looked at last
        (dict(data=VEC, limit=65), "learned sparse search: limit = 65 > 64 (the sparse arm is not paged)", ARM_LIMIT),
        (dict(data=VEC, declared=False), NO_LEARNED, NO_LEARNED),
        (dict(param=metric(LEARNED, params={"radius": 1.0}), limit=0), LEARNED_RANGE, None),
        (dict(param=metric(LEARNED, offset=2, params={"radius": 1.0})), LEARNED_FORMS, LEARNED_RANGE),
        (dict(offset=2, limit=0), WINDOW, None),
        (dict(group_by_field="period", declared=False), LEARNED_FORMS, None),
        (dict(ranker=BOOST, expr=LIST_EXPR), RANKER_LIST, None),
    ],
    TOKENS: [
        (dict(declared=False), NO_TOKENS, NO_TOKENS),
        (dict(param={"metric_type": "IP"}), TOKENS_METRIC, TOKENS_METRIC),
        (dict(param=metric(TOKENS, params=3)), PARAMS, PARAMS),
        (dict(param=metric(TOKENS, params={"radius": 1.0})), TOKENS_RANGE, TOKENS_RANGE),
        (dict(param=metric(TOKENS, params={"range_filter": 1.0})), TOKENS_RANGE, TOKENS_RANGE),
        (dict(offset=2), TOKENS_FORMS, None),
        (dict(param=metric(TOKENS, offset=2)), TOKENS_FORMS, TOKENS_ARM_OFFSET),
        (dict(limit=0), TOKENS_LIMIT, None),
        (dict(limit=True), TOKENS_LIMIT, None),
        (dict(limit=65), TOKENS_BIG, ARM_LIMIT),
        (dict(data=VEC), TOKENS_DATA, TOKENS_DATA),
        (dict(data=[{0: 1.0}]), TOKENS_DATA, TOKENS_DATA),
        (dict(data=[np.ones((33, 32), np.float16)]),
         "the token_embeddings field: query 0 has 33 token vectors, more than 32",
         "the token_embeddings field: query 0 has 33 token vectors, more than 32"),
        (dict(expr=LIST_EXPR), "per-query filters (a list expr) have no late-interaction form (anns_field='token_embeddings')",
         ARM_LIST),
        (dict(ranker=BOOST), "boosted search (ranker) has no late-interaction form (anns_field='token_embeddings')", None),
        (dict(group_by_field="period"), TOKENS_FORMS, None),
        (dict(mmr_lambda=0.5), TOKENS_FORMS, None),
        (dict(mmr_fetch_k=20), TOKENS_FORMS, None),
        (dict(iterator=True), "search_iterator has no late-interaction form (anns_field='token_embeddings')", None),
        # two at once
        (dict(data=VEC, param={"metric_type": "IP"}), TOKENS_METRIC, TOKENS_METRIC),      # the data is looked at last
        (dict(data=VEC, limit=65), TOKENS_BIG, ARM_LIMIT),
        (dict(data=VEC, declared=False), NO_TOKENS, NO_TOKENS),
        (dict(param=metric(TOKENS, params={"radius": 1.0}), limit=0), TOKENS_RANGE, None),
        (dict(param=metric(TOKENS, offset=2, params={"radius": 1.0})), TOKENS_FORMS, TOKENS_RANGE),
        (dict(offset=2, limit=0), WINDOW, None),
        (dict(group_by_field="period", declared=False), TOKENS_FORMS, None),
        (dict(ranker=BOOST, expr=LIST_EXPR), RANKER_LIST, None),
    ],
}
CASES = [(name, *row) for name, rows in REFUSALS.items() for row in rows]
IDS = [f"{name}-{'+'.join(wrong)}-{j}" for name, rows in REFUSALS.items() for j, (wrong, _, _) in enumerate(rows)]


def refused(call) -> str:
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


@pytest.mark.parametrize("name,wrong,message,arm_message", CASES, ids=IDS)
def test_a_search_of_a_derived_field_refuses_with_the_message_of_its_field(name, wrong, message, arm_message):
    wrong = dict(wrong)
    st = make_store(fields=(name,) if wrong.pop("declared", True) else ())
    good = dict(data=QUERY, anns_field=name, param=metric(name), limit=3)
    if wrong.pop("iterator", False):
        assert refused(lambda: st.search_iterator(VEC, name, metric(name))) == message
    else:
        assert refused(lambda: st.search(**dict(good, **wrong))) == message
    if arm_message is not None:
        arm = dict(good, **wrong)
        reqs = [AnnSearchRequest(VEC, "embedding", COS, 3),
                AnnSearchRequest(arm["data"], name, arm["param"], arm["limit"], arm.get("expr"))]
        assert refused(lambda: st.hybrid_search(reqs, RRFRanker(), 3)) == arm_message
    assert st.index.calls == []                                          # refused before anything ran


# ---- the life cycle every field shares -----------------------------------------------------------------------------
@pytest.fixture
def doubles(monkeypatch):
    from rag_fin_amd import text_fields   # (imported here: the refusal table above needs only the public surface)
    monkeypatch.setattr(text_fields, "SparseIndex", FakeSparse)
    monkeypatch.setattr(late, "TokenField", FakeTokenField)
    monkeypatch.setattr(late, "maxsim", fake_maxsim)
    monkeypatch.setattr(store_mod, "fuse_rrf", fake_fuse)
    FakeSparse.built.clear()


def built_state(st, name):
    """What the field has built over the store's rows (built now if a mutation is pending), as plain lists."""
    field = st._text_fields[name]
    if name == TOKENS:
        f = field.index()
        return f.off_host.tolist(), [r.tolist() for r in f.rows]
    p = (field.index() if name == SPARSE else field.postings())[0]
    state = [p.post_off.tolist(), p.post_row.tolist(), np.asarray(p.post_imp).view(np.uint32).tolist()]
    return state + [list(p.vocab), p.post_tf.tolist(), p.dl.tolist()] if name == SPARSE else state


def answers(st, name):
    return [[(h.row, h.id, h.score) for h in q] for q in st.search(["eps q1", "words"], name, metric(name), limit=5)]


NO_INDEX = {SPARSE: NO_SPARSE, LEARNED: NO_LEARNED, TOKENS: NO_TOKENS}


@pytest.mark.parametrize("spelling", ["field_name", "index_name"])
@pytest.mark.parametrize("name", [SPARSE, LEARNED, TOKENS])
def test_a_derived_field_is_declared_built_lazily_kept_up_to_date_and_dropped(doubles, name, spelling):
    st = make_store(fields=())
    field = st._text_fields[name]
    assert not st.has_index(**{spelling: name}) and not field.declared
    declare(st, name)
    assert st.has_index(**{spelling: name}) and field.declared and field.built is None      # declared, not built
    assert not st.has_index() and st.index_type == "FLAT"                                   # the vector index is untouched
    assert [st.has_index(field_name=other) for other in NO_INDEX if other != name] == [False, False]
    st.add(["n0", "n1"], ["new row words eps", "q1 words"], np.ones((2, 8), np.float32), ["Q0", "Q1"], ["a"] * 2, ["s"] * 2,
           [1.0, 2.0])
    assert field.built is None
    assert all(answers(st, name)) and field.built is not None                               # the first search builds
    st.delete('period == "Q0"')                                                             # rows 0, 2, .., and n0
    survivors = list(st.columns["text"])
    assert len(survivors) == 6 and survivors[-1] == "q1 words"
    fresh = make_store(survivors, fields=(name,))
    assert built_state(st, name) == built_state(fresh, name)
    assert [[(r, s) for r, _, s in q] for q in answers(st, name)] == [[(r, s) for r, _, s in q] for q in answers(fresh, name)]
    st.drop()
    assert st.has_index(**{spelling: name}) and field.built is None                         # the declaration survives
    assert answers(st, name) == [[], []]
    st.drop_index(**{spelling: name})
    assert not st.has_index(**{spelling: name}) and not field.declared and field.built is None
    assert refused(lambda: st.search(QUERY, name, metric(name), limit=3)) == NO_INDEX[name]
    assert refused(lambda: st.hybrid_search([AnnSearchRequest(QUERY, name, metric(name), 3)], RRFRanker(), 3)) == NO_INDEX[name]
