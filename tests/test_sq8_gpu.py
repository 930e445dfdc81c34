"""The SQ8 index type on the GPU: the int8 shadow against a numpy mirror of the
quantizer, the error bound |a - a~| <= delta_q on every row, the integer MFMA's fragment map,
rf_search_sq8 against rf_search and the C oracle (ids, ranks, fp32 and fp64 scores, flags after
the fallback), the candidate superset (experiments build, child process), the shadow's upkeep
through adds, compactions, growth, drop and save/load, concurrent searches, and the store level."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from oracle import c_oracle, search as osearch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- data ------------------------------------------------------------------------------------
def clustered(n, d, seed, centers=1024, spread=0.05):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32)
    x = c[rng.integers(0, centers, n)] + spread * rng.standard_normal((n, d)).astype(np.float32)
    return osearch.l2_normalize_f32(x).astype(np.float16)


def dominant(n, d, seed, factor=30.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:, 7] *= factor
    return osearch.l2_normalize_f32(x).astype(np.float16)


def raw_ip(n, d, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) * rng.uniform(0.1, 3.0, (n, 1))).astype(np.float16)


def make_index(c16, device, sq8=True, capacity=None):
    import torch
    from rag_fin_amd.store import GpuIndex
    ix = GpuIndex(c16.shape[1], capacity or max(1, c16.shape[0]), device)
    if c16.shape[0]:
        ix.add(torch.from_numpy(c16).to(device))
    if sq8:
        ix.enable_sq8()
    return ix


def quant_mirror(c16):
    """numpy fp32 mirror of the row quantizer: int8 codes, scales, fp64 residual norms."""
    c = c16.astype(np.float32)
    s = (np.abs(c).max(1) / np.float32(127)).astype(np.float32)
    safe = np.where(s > 0, s, np.float32(1))
    code = np.clip(np.rint(c / safe[:, None]), -127, 127)
    code = np.where(s[:, None] > 0, code, 0).astype(np.int8)
    resid = np.sqrt(((c.astype(np.float64) - s[:, None].astype(np.float64) * code) ** 2).sum(1))
    return code, s, resid


def shadow(ix):
    import torch
    q8, s, e = ix.get_rows_sq8(np.arange(ix.size, dtype=np.int64))
    torch.cuda.synchronize()
    return q8.cpu().numpy(), s.cpu().numpy(), e.cpu().numpy()


# ---- quantizer and bound -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unit", "dominant", "ip"])
def test_quantizer_matches_numpy_mirror(gpu_device, kind):
    n, d = 5003, 384
    c = {"unit": osearch.synth_unit_rows(n, d, 11), "dominant": dominant(n, d, 12), "ip": raw_ip(n, d, 13)}[kind]
    c[17] = 0                       # a zero row
    ix = make_index(c, gpu_device)
    q8, s, e = shadow(ix)
    code, s_ref, resid = quant_mirror(c)
    assert np.array_equal(q8, code)
    assert np.array_equal(s.view(np.uint32), s_ref.view(np.uint32))
    assert s[17] == 0 and e[17] == 0 and not q8[17].any()
    assert (e.astype(np.float64) >= resid * (1 - 1e-6)).all()
    assert (e.astype(np.float64) <= resid * (1 + 1e-5) + 1e-30).all()


@pytest.mark.parametrize("kind,metric", [("unit", "cos"), ("clustered", "cos"), ("dominant", "cos"),
                                         ("ip", "ip"), ("zeros", "cos")])
def test_error_bound_holds_for_every_row(gpu_device, kind, metric):
    import torch
    n, d, b = 20000, 384, 70
    gen = {"unit": osearch.synth_unit_rows, "clustered": clustered, "dominant": dominant, "ip": raw_ip,
           "zeros": osearch.synth_unit_rows}[kind]
    c = gen(n, d, 21)
    q = gen(b, d, 22)
    if kind == "zeros":
        c[::97] = 0
        q[3] = 0
    ix = make_index(c, gpu_device)
    at, delta = ix.debug_scores_sq8(torch.from_numpy(q).to(gpu_device))
    torch.cuda.synchronize()
    at = at.cpu().numpy().astype(np.float64)
    delta = delta.cpu().numpy().astype(np.float64)
    exact = q.astype(np.float64) @ c.astype(np.float64).T
    err = np.abs(exact - at)
    assert (err <= delta[:, None]).all(), float((err - delta[:, None]).max())
    ratio = float((err / np.maximum(delta[:, None], 1e-30)).max())
    print(kind, "max |a - a~| / delta", ratio, "mean delta", float(delta.mean()))


def test_integer_mfma_fragment_map(gpu_device):
    """Exact integer data with s_r = t_q = 1 (every row and query holds a +-127): a~ is the integer
    dot product D itself, for an asymmetric operand pair."""
    import torch
    rng = np.random.default_rng(5)
    n, d, b = 96, 384, 40
    c = rng.integers(-127, 128, (n, d)).astype(np.float32)
    q = rng.integers(-127, 128, (b, d)).astype(np.float32)
    c[np.arange(n), rng.integers(0, d, n)] = 127
    q[np.arange(b), rng.integers(0, d, b)] = -127
    ix = make_index(c.astype(np.float16), gpu_device)
    at, _ = ix.debug_scores_sq8(torch.from_numpy(q.astype(np.float16)).to(gpu_device))
    torch.cuda.synchronize()
    want = q.astype(np.int64) @ c.astype(np.int64).T
    assert np.array_equal(at.cpu().numpy().astype(np.int64), want)


# ---- exactness ---------------------------------------------------------------------------------
def check_sq8_search(ix, q16, c16, k, device, oracle_rows=None, expect_clean=False):
    """search(sq8=True) == search() (FLAT) == the C oracle, with the fallback; returns the raw SQ8 flags."""
    import torch
    qd = torch.from_numpy(q16).to(device)
    _, _, _, raw_flags = ix.search_raw(qd, k, want_exact=True, sq8=True)
    s8, i8, e8 = ix.search(qd, k, want_exact=True, sq8=True)
    s0, i0, e0 = ix.search(qd, k, want_exact=True)
    torch.cuda.synchronize()
    assert torch.equal(i8, i0) and torch.equal(e8, e0) and torch.equal(s8, s0)
    sel = slice(None) if oracle_rows is None else slice(0, oracle_rows)
    os_, oi = c_oracle.search(q16[sel], c16, k)
    assert np.array_equal(i8[sel].cpu().numpy(), oi)
    assert np.array_equal(e8[sel].cpu().numpy(), os_)
    assert np.array_equal(s8[sel].cpu().numpy(), os_.astype(np.float32))
    raw_flags = raw_flags.cpu().numpy()
    if expect_clean:
        # no candidate overflow; a rescoring set wider than the merge holds (RF_FLAG_TIE_OVERFLOW) can
        # happen on random data (|R| against RF_RESCORE_CAP) and is answered by FLAT
        assert not (raw_flags & 1).any(), raw_flags
    return raw_flags


@pytest.mark.parametrize("n,b,k", [
    (1, 1, 1), (31, 63, 10), (33, 64, 64), (8192, 65, 10), (8193, 1, 10), (8193, 200, 64),
    (100_000, 63, 1), (100_000, 64, 10), (100_000, 65, 64), (100_000, 200, 10),
])
def test_sq8_search_equals_flat_and_oracle(gpu_device, n, b, k):
    c = osearch.synth_unit_rows(n, 384, 31)
    q = osearch.synth_unit_rows(b, 384, 32)
    check_sq8_search(make_index(c, gpu_device), q, c, k, gpu_device, expect_clean=n > 8192 and k <= 10)


def test_sq8_search_1m(gpu_device):
    """The headline shape: 1 M x 384, B in {1, 64, 200}, k = 10, against the exhaustive kernel."""
    import torch
    c = osearch.synth_unit_rows(1_000_000, 384, 1234)
    ix = make_index(c, gpu_device)
    for b in (1, 64, 200):
        q = osearch.synth_unit_rows(b, 384, 5678 + b)
        qd = torch.from_numpy(q).to(gpu_device)
        _, _, _, f8 = ix.search_raw(qd, 10, want_exact=True, sq8=True)
        s8, i8, e8 = ix.search(qd, 10, want_exact=True, sq8=True)
        s2, i2, e2 = ix.search_exhaustive(qd, 10, want_exact=True)
        torch.cuda.synchronize()
        f8 = f8.cpu().numpy()
        assert not (f8 & 1).any()
        print("1M B =", b, "queries flagged by SQ8 (rescoring set overflow):", int((f8 != 0).sum()))
        assert torch.equal(i8, i2) and torch.equal(e8, e2) and torch.equal(s8, s2)
        os_, oi = c_oracle.search(q[:2], c, 10)
        assert np.array_equal(i8[:2].cpu().numpy(), oi) and np.array_equal(e8[:2].cpu().numpy(), os_)


@pytest.mark.parametrize("kind", ["clustered", "ip", "dominant"])
def test_sq8_search_other_data(gpu_device, kind):
    n, b, k = 60_000, 64, 10
    gen = {"clustered": clustered, "ip": raw_ip, "dominant": dominant}[kind]
    c = gen(n, 384, 41)
    q = gen(b, 384, 42)
    flags = check_sq8_search(make_index(c, gpu_device), q, c, k, gpu_device, expect_clean=kind == "clustered")
    print(kind, "queries flagged by SQ8:", int((flags != 0).sum()))


def test_sq8_dim768_and_ties(gpu_device):
    """dim 768 (the other BASELINE dim), and exact ties: 40 000 rows made of 500 distinct rows, so
    every score occurs 80 times and the ranking falls back on row-ascending order."""
    c = osearch.synth_unit_rows(30_000, 768, 51)
    q = osearch.synth_unit_rows(33, 768, 52)
    check_sq8_search(make_index(c, gpu_device), q, c, 10, gpu_device, expect_clean=True)
    base = osearch.synth_unit_rows(500, 384, 53)
    c = np.tile(base, (80, 1))
    q = osearch.synth_unit_rows(20, 384, 54)
    q[:5] = base[:5]
    check_sq8_search(make_index(c, gpu_device), q, c, 64, gpu_device)
    check_sq8_search(make_index(c, gpu_device), q, c, 1, gpu_device)


def test_all_identical_corpus_falls_back_and_stays_exact(gpu_device):
    """Every row equal: every row is a candidate (SQ8 flags the overflow), FLAT flags it too, the
    exhaustive kernel answers; ties by row id."""
    row = osearch.synth_unit_rows(1, 384, 61)
    c = np.repeat(row, 30_000, axis=0)
    q = osearch.synth_unit_rows(5, 384, 62)
    flags = check_sq8_search(make_index(c, gpu_device), q, c, 10, gpu_device)
    assert flags.all()


def test_sq8_refuses_search_without_shadow(gpu_device):
    import torch
    from rag_fin_amd import _lib
    from rag_fin_amd.store import GpuIndex
    ix = GpuIndex(384, 100, gpu_device)
    with pytest.raises(_lib.RagfinError, match="no SQ8 shadow"):
        ix.search_raw(torch.zeros((1, 384), dtype=torch.float16, device=gpu_device), 5, sq8=True)


# ---- candidate superset (experiments build: rf_debug_workspace_offset) --------------------------
_CAND_CHILD = r"""
import json, sys
import numpy as np, torch
from oracle import c_oracle, search as osearch
from rag_fin_amd import _lib
from rag_fin_amd.store import GpuIndex
lib = _lib.load_library()
dev = torch.device("cuda:0")
_lib.check(lib.rf_set_tuning(b"fold_dbg", 2))    # the merge leaves the candidate counters
off_cnt = lib.rf_debug_workspace_offset(b"cand_cnt")
off_cand = lib.rf_debug_workspace_offset(b"cand")
out = {}
for (n, b, k, kind) in json.loads(sys.argv[1]):
    if kind == "clustered":
        rng = np.random.default_rng(71)
        cen = rng.standard_normal((1024, 384)).astype(np.float32)
        x = cen[rng.integers(0, 1024, n + b)] + 0.05 * rng.standard_normal((n + b, 384)).astype(np.float32)
        x = osearch.l2_normalize_f32(x).astype(np.float16)
        c, q = x[:n], x[n:]
    else:
        c = osearch.synth_unit_rows(n, 384, 73)
        q = osearch.synth_unit_rows(b, 384, 74)
    ix = GpuIndex(384, n, dev)
    ix.add(torch.from_numpy(c).to(dev))
    ix.enable_sq8()
    s, i, e, f = ix.search_raw(torch.from_numpy(q).to(dev), k, want_exact=True, sq8=True)
    torch.cuda.synchronize()
    ws = ix.workspace
    cnt = ws[off_cnt:off_cnt + 64 * 8 * 4].view(torch.int32).view(64, 8).cpu().numpy()
    cand = ws[off_cand:off_cand + 64 * 8 * 2048 * 8].view(torch.int32).view(64, 8, 2048, 2).cpu().numpy()
    _, oi = c_oracle.search(q, c, k)
    fl = f.cpu().numpy()
    missing, counts = 0, []
    for qi in range(b):
        if fl[qi] & 1:      # candidate lists overflowed: the query is not proven by SQ8 (FLAT answers it)
            continue
        rows = set(np.concatenate([cand[qi, sh, :min(cnt[qi, sh], 2048), 0] for sh in range(8)]).tolist())
        counts.append(len(rows))
        missing += sum(1 for r in oi[qi].tolist() if r not in rows)
    ok = fl == 0
    out["%d_%d_%d_%s" % (n, b, k, kind)] = dict(missing=missing, counts=counts, flags=fl.tolist(),
                                               ids_equal=bool(np.array_equal(i.cpu().numpy()[ok], oi[ok])))
_lib.check(lib.rf_set_tuning(b"fold_dbg", 0))
print("RESULT " + json.dumps(out))
"""


def test_candidates_contain_exact_topk(gpu_device):
    shapes = [(100_000, 64, 10, "unit"), (100_000, 40, 64, "unit"), (200_000, 64, 10, "clustered")]
    env = dict(os.environ, RAGFIN_LIB="exp")
    r = subprocess.run([sys.executable, "-c", _CAND_CHILD, json.dumps(shapes)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    for shape, res in json.loads(line[len("RESULT "):]).items():
        if shape.endswith("_10_unit"):
            assert not any(x & 1 for x in res["flags"]), shape
        assert sum(1 for x in res["flags"] if not x & 1) >= len(res["flags"]) // 2, shape
        assert res["missing"] == 0, shape
        assert res["ids_equal"], shape
        print(shape, "candidates per query: mean", np.mean(res["counts"]), "max", max(res["counts"]))


# ---- upkeep of the shadow --------------------------------------------------------------------------
def assert_shadow_fresh(ix, device):
    """The shadow (and its N' / E trackers, seen through delta_q) equals a fresh attach over the rows."""
    import torch
    rows = ix.get_rows(np.arange(ix.size, dtype=np.int64)).cpu().numpy()
    fresh = make_index(rows, device)
    a, b = shadow(ix), shadow(fresh)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    q = torch.from_numpy(osearch.synth_unit_rows(3, ix.dim, 81)).to(device)
    _, d1 = ix.debug_scores_sq8(q)
    _, d2 = fresh.debug_scores_sq8(q)
    torch.cuda.synchronize()
    assert torch.equal(d1, d2)
    return rows


def test_shadow_upkeep_adds_compaction_reset(gpu_device):
    import torch
    d = 384
    c = np.concatenate([osearch.synth_unit_rows(30_000, d, 91), dominant(3_000, d, 92)])
    ix = make_index(c[:0], gpu_device, capacity=40_000)
    ix.enable_sq8()
    for s0, s1 in ((0, 5), (5, 40), (40, 10_001), (10_001, 33_000)):    # chunked adds, ragged blocks
        ix.add(torch.from_numpy(c[s0:s1]).to(gpu_device))
    assert_shadow_fresh(ix, gpu_device)
    keep = np.flatnonzero(np.random.default_rng(3).random(33_000) > 0.3)
    keep = keep[keep != 30_500]                        # drop a dominant row: N' / E recomputed
    ix.compact(keep, window_rows=4096)
    rows = assert_shadow_fresh(ix, gpu_device)
    assert np.array_equal(rows, c[keep])
    q = osearch.synth_unit_rows(64, d, 93)
    check_sq8_search(ix, q, rows, 10, gpu_device, oracle_rows=8)
    ix.add(torch.from_numpy(c[:777]).to(gpu_device))   # append after a compaction
    assert_shadow_fresh(ix, gpu_device)
    ix.reset()
    ix.add(torch.from_numpy(c[100:9000]).to(gpu_device))
    rows = assert_shadow_fresh(ix, gpu_device)
    check_sq8_search(ix, q, rows, 10, gpu_device, oracle_rows=8)


def test_store_sq8_grow_delete_upsert_drop_save_load(gpu_device, tmp_path):
    from rag_fin_amd.store import CorpusStore
    d = 384
    rng = np.random.default_rng(7)
    st = CorpusStore("t", dim=d, capacity=4096, device=gpu_device)
    st.create_index("embedding", {"index_type": "SQ8", "metric_type": "COSINE"})

    def batch(keys):
        v = rng.standard_normal((len(keys), d)).astype(np.float32)
        return [list(keys), [f"t{x}" for x in keys], v, ["Q1_FY2024"] * len(keys), ["table"] * len(keys),
                ["income"] * len(keys), [float(x) for x in keys]]

    st.insert(batch(range(0, 6000)))
    st.insert(batch(range(6000, 14000)))                # grows past the capacity: re-attached
    assert st.index.sq8 and st.index.capacity >= 14000
    assert_shadow_fresh(st.index, gpu_device)
    st.delete("id in [%s]" % ",".join(str(x) for x in range(0, 14000, 3)))
    st.upsert(batch(range(1, 3000, 3)))
    rows = assert_shadow_fresh(st.index, gpu_device)
    q = osearch.l2_normalize_f32(rng.standard_normal((5, d)).astype(np.float32))
    hits = st.search(q, limit=10, output_fields=["id"])
    q16 = q.astype(np.float16)
    _, oi = c_oracle.search(q16, rows, 10)
    assert [[h.id for h in hs] for hs in hits] == [[st.columns["id"][r] for r in row] for row in oi]
    st.save(str(tmp_path / "c"))
    assert json.load(open(tmp_path / "c" / "columns.json"))["index_type"] == "SQ8"
    st2 = CorpusStore.load_from(str(tmp_path / "c"), device=gpu_device)
    assert st2.index_type == "SQ8" and st2.index.sq8 and st2.has_index()
    assert_shadow_fresh(st2.index, gpu_device)
    hits2 = st2.search(q, limit=10, output_fields=["id"])
    assert [[h.id for h in hs] for hs in hits2] == [[h.id for h in hs] for hs in hits]
    st.drop()
    st.insert(batch(range(100, 9300)))
    assert st.index.sq8
    assert_shadow_fresh(st.index, gpu_device)


# ---- threads and the store level ---------------------------------------------------------------------
def test_concurrent_sq8_and_flat_searches(gpu_device):
    import torch
    c = osearch.synth_unit_rows(150_000, 384, 101)
    q = torch.from_numpy(osearch.synth_unit_rows(64, 384, 102)).to(gpu_device)
    ix = make_index(c, gpu_device)
    refs = [ix.search_raw(q, 10, want_exact=True, sq8=sq8) for sq8 in (False, True)]
    torch.cuda.synchronize()
    results, errors = {}, []

    def worker(t):
        try:
            st = torch.cuda.Stream(gpu_device)
            ws = ix.new_workspace()
            with torch.cuda.stream(st):
                outs = [((t + j) % 2, ix.search_raw(q, 10, want_exact=True, workspace=ws, sq8=(t + j) % 2 == 1))
                        for j in range(6)]
            st.synchronize()
            results[t] = outs
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    assert len(results) == 4
    for outs in results.values():
        for path, got in outs:
            # a query whose rescoring set overflowed keeps an arbitrary part of it (flagged, answered
            # by FLAT): compare the flags, and the outputs of the proven queries
            assert torch.equal(got[3], refs[path][3])
            ok = refs[path][3] == 0
            for x, y in zip(got[:3], refs[path][:3]):
                assert torch.equal(x[ok], y[ok])


def test_vector_rag_over_sq8_store_matches_flat(gpu_device):
    from rag_fin_amd.rag import VectorRAG
    from rag_fin_amd.store import CorpusStore
    d, n = 384, 20_000
    rng = np.random.default_rng(111)
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    texts = [f"chunk {i}" for i in range(n)]

    class Emb:
        def encode(self, xs):
            return np.stack([np.random.default_rng(abs(hash(x)) % (1 << 32)).standard_normal(d).astype(np.float32)
                             for x in xs])

    stores = []
    for itype in ("FLAT", "SQ8"):
        st = CorpusStore("t", dim=d, capacity=n, device=gpu_device)
        st.create_index("embedding", {"index_type": itype, "metric_type": "COSINE"})
        st.insert([list(range(n)), texts, vecs, ["Q1_FY2024"] * n, ["table"] * n, ["income"] * n,
                   [float(i) for i in range(n)]])
        stores.append(st)
    flat, sq8 = (VectorRAG(embedder=Emb(), store=s) for s in stores)
    for query in ("revenue Q1", "net income", "operating cash flow", "eps diluted"):
        assert flat.search(query, top_k=10) == sq8.search(query, top_k=10)
