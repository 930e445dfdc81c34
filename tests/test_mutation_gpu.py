"""delete / upsert on the GPU: rf_index_compact leaves the index bit-identical to a fresh build of
the surviving rows (tiles, pad rows, max_norm2 word), searches after a delete equal the C oracle
on the survivors (ids, ranks, fp64 scores bit-exact, flags 0 on the raw path), and the store's
delete / upsert / save / filter mirror / threads behave."""
import ctypes
import threading
from ctypes import c_void_p

import numpy as np
import pytest

from oracle import c_oracle, search as osearch

pytestmark = pytest.mark.gpu

N, D = 100_003, 384
_C = {}


def corpus():
    if "c" not in _C:
        _C["c"] = osearch.synth_unit_rows(N, D, 21)
    return _C["c"]


def make_index(c16, device, capacity=None):
    import torch
    from rag_fin_amd.store import GpuIndex
    ix = GpuIndex(c16.shape[1], max(capacity or c16.shape[0], 1), device)
    if c16.shape[0]:
        ix.add(torch.from_numpy(np.ascontiguousarray(c16)).to(device))
    return ix


def live_bytes(ix, n):
    KS = ix.dim // 16
    return ix.storage[:((n + 31) // 32) * KS * 1024]


def norm_word(ix):
    return int(ix.storage[-256:-252].cpu().numpy().view(np.uint32)[0])


def pad_rows_are_zero(ix, n):
    if n % 32 == 0:
        return True
    KS = ix.dim // 16
    nb = (n + 31) // 32
    last = ix.storage[(nb - 1) * KS * 1024:nb * KS * 1024].cpu().numpy().reshape(KS, 2, 32, 16)
    return not last[:, :, n % 32:, :].any()


def pattern(name, n, rng):
    keep = np.ones(n, dtype=bool)
    if name == "none":
        pass
    elif name == "first":
        keep[0] = False
    elif name == "last":
        keep[-1] = False
    elif name == "run":
        keep[1000:5017] = False            # crosses many block boundaries, not block aligned
    elif name == "rand10":
        keep[rng.random(n) < 0.1] = False
    elif name == "all_but_one":
        keep[:] = False
        keep[n // 3] = True
    elif name == "all":
        keep[:] = False
    else:
        raise ValueError(name)
    return np.flatnonzero(keep)


@pytest.mark.parametrize("window", [None, 32])
@pytest.mark.parametrize("name", ["none", "first", "last", "run", "rand10", "all_but_one", "all"])
def test_compacted_index_is_a_fresh_build_of_the_survivors(gpu_device, name, window):
    import torch
    c16 = corpus()
    keep = pattern(name, N, np.random.default_rng(5))
    ix = make_index(c16, gpu_device)
    ix.compact(keep, window_rows=window)
    n2 = keep.size
    assert ix.size == n2
    if n2:
        fresh = make_index(c16[keep], gpu_device)
        torch.cuda.synchronize()
        assert torch.equal(live_bytes(ix, n2), live_bytes(fresh, n2))
        assert norm_word(ix) == norm_word(fresh)
        assert pad_rows_are_zero(ix, n2)
    else:   # as rf_index_reset left it (a fresh index has not written its tracker before its first add)
        torch.cuda.synchronize()
        assert norm_word(ix) == 0
        # then it behaves like a new index
        extra = osearch.synth_unit_rows(1000, D, 22)
        ix.add(torch.from_numpy(extra).to(gpu_device))
        q16 = osearch.synth_unit_rows(8, D, 23)
        _, ids, exact = ix.search(torch.from_numpy(q16).to(gpu_device), 10, want_exact=True)
        es, ei = c_oracle.search(q16, extra, 10)
        assert np.array_equal(ids.cpu().numpy(), ei) and np.array_equal(exact.cpu().numpy(), es)
        fresh = make_index(extra, gpu_device)
        torch.cuda.synchronize()
        assert norm_word(ix) == norm_word(fresh) and torch.equal(live_bytes(ix, 1000), live_bytes(fresh, 1000))


def test_max_norm2_is_recomputed_over_the_survivors(gpu_device):
    import torch
    rng = np.random.default_rng(7)
    base = osearch.synth_unit_rows(4099, D, 24).astype(np.float32)
    scale = rng.uniform(0.25, 2.0, size=(4099, 1)).astype(np.float32)
    scale[1234] = 4.0                                 # the largest norm, alone
    c16 = (base * scale).astype(np.float16)
    ix = make_index(c16, gpu_device)
    before = norm_word(ix)
    keep = np.flatnonzero(np.arange(4099) != 1234)
    ix.compact(keep)
    fresh = make_index(c16[keep], gpu_device)
    torch.cuda.synchronize()
    assert norm_word(ix) == norm_word(fresh) < before
    assert torch.equal(live_bytes(ix, keep.size), live_bytes(fresh, keep.size))


def test_compact_argument_checks(gpu_device):
    import torch
    from rag_fin_amd import _lib
    lib = _lib.load_library()
    c16 = osearch.synth_unit_rows(100, D, 25)
    ix = make_index(c16, gpu_device)
    keep = torch.arange(50, dtype=torch.int64, device=gpu_device)
    scratch = torch.empty(32 * D * 2 + 64, dtype=torch.uint8, device=gpu_device)
    kp, sp = keep.data_ptr(), scratch.data_ptr()
    with torch.cuda.device(gpu_device):
        st = _lib.current_stream_ptr()
        assert lib.rf_index_compact(ix.handle, c_void_p(kp), 101, c_void_p(sp), 32 * D * 2, st) == -1   # > size
        assert lib.rf_index_compact(ix.handle, c_void_p(kp), -1, c_void_p(sp), 32 * D * 2, st) == -1
        assert lib.rf_index_compact(ix.handle, None, 50, c_void_p(sp), 32 * D * 2, st) == -1
        assert lib.rf_index_compact(ix.handle, c_void_p(kp), 50, None, 32 * D * 2, st) == -1
        assert lib.rf_index_compact(ix.handle, c_void_p(kp + 4), 50, c_void_p(sp), 32 * D * 2, st) == -1
        assert lib.rf_index_compact(ix.handle, c_void_p(kp), 50, c_void_p(sp + 8), 32 * D * 2, st) == -1
        assert lib.rf_index_compact(ix.handle, c_void_p(kp), 50, c_void_p(sp), 32 * D * 2 - 1, st) == -3
    assert ix.size == 100
    with pytest.raises(ValueError, match="ascending"):
        ix.compact([3, 2])
    with pytest.raises(ValueError, match="ascending"):
        ix.compact([5, 100])
    with pytest.raises(ValueError, match="multiple of 32"):
        ix.compact([1, 2], window_rows=48)
    ix.compact(np.arange(50, 100))              # n_keep < size with the Python default window
    torch.cuda.synchronize()
    assert torch.equal(live_bytes(ix, 50), live_bytes(make_index(c16[50:], gpu_device), 50))


# ---- search after a delete = the oracle on the survivors ---------------------------------------------
@pytest.fixture(scope="module")
def deleted_index(gpu_device):
    c16 = corpus()
    rng = np.random.default_rng(9)
    keep = np.ones(N, dtype=bool)
    keep[rng.random(N) < 0.1] = False
    keep[20_000:33_333] = False
    keep = np.flatnonzero(keep)
    ix = make_index(c16, gpu_device)
    ix.compact(keep, window_rows=4096)
    return ix, np.ascontiguousarray(c16[keep])


@pytest.mark.parametrize("B", [1, 64, 256])
def test_search_after_delete_equals_the_oracle(gpu_device, deleted_index, B):
    import torch
    ix, s16 = deleted_index
    q16 = osearch.synth_unit_rows(B, D, 30 + B)
    scores, ids, exact, flags = ix.search_raw(torch.from_numpy(q16).to(gpu_device), 10, want_exact=True)
    torch.cuda.synchronize()
    assert int(flags.abs().sum()) == 0
    es, ei = c_oracle.search(q16, s16, 10)
    assert np.array_equal(ids.cpu().numpy(), ei)
    assert np.array_equal(exact.cpu().numpy(), es)
    assert np.array_equal(scores.cpu().numpy(), es.astype(np.float32))


def test_large_limit_after_delete_equals_the_oracle(gpu_device, deleted_index):
    import torch
    ix, s16 = deleted_index
    q16 = osearch.synth_unit_rows(4, D, 40)
    scores, ids, exact = ix.search_large(torch.from_numpy(q16).to(gpu_device), 100, want_exact=True)
    es, ei = c_oracle.search(q16, s16, 100)
    assert np.array_equal(ids.cpu().numpy(), ei) and np.array_equal(exact.cpu().numpy(), es)


def test_filtered_search_after_delete_equals_the_oracle(gpu_device, deleted_index):
    import torch
    from rag_fin_amd import _lib
    ix, s16 = deleted_index
    n = s16.shape[0]
    mask = np.zeros(n, dtype=bool)
    mask[n // 4:n // 4 + n // 8] = True
    mask[np.random.default_rng(3).random(n) < 0.01] = True
    lib = _lib.load_library()
    words = np.packbits(np.pad(mask, (0, (-n) % 32)).reshape(-1, 8), axis=1, bitorder="little").reshape(-1)
    filt = torch.empty(lib.rf_filter_bytes(n), dtype=torch.uint8, device=gpu_device)
    w = torch.from_numpy(words.view(np.int32).copy()).to(gpu_device)
    with torch.cuda.device(gpu_device):
        _lib.check(lib.rf_filter_from_mask(c_void_p(w.data_ptr()), n, c_void_p(filt.data_ptr()),
                                           _lib.current_stream_ptr()))
    q16 = osearch.synth_unit_rows(64, D, 41)
    scores, ids, exact, flags = ix.search_raw(torch.from_numpy(q16).to(gpu_device), 10, want_exact=True, filt=filt)
    torch.cuda.synchronize()
    assert int(flags.abs().sum()) == 0
    S = np.flatnonzero(mask)
    es, ei = c_oracle.search(q16, s16[S], 10)
    assert np.array_equal(ids.cpu().numpy(), S[ei]) and np.array_equal(exact.cpu().numpy(), es)


# ---- the store --------------------------------------------------------------------------------------
PERIODS = ["Q1_FY2024", "Q2_FY2024", "Q3_FY2024", "Q4_FY2024"]


def cols_for(keys, v16, tag="v1"):
    import torch
    n = len(keys)
    return [list(keys), [f"{tag}:{k}" for k in keys], torch.from_numpy(np.ascontiguousarray(v16)),
            [PERIODS[int(k[1:]) % 4] for k in keys], ["c"] * n, ["s"] * n, [float(k[1:]) for k in keys]]


def expect_search(store_keys, rows16, q16, k):
    es, ei = c_oracle.search(q16, rows16, k)
    return es, [[store_keys[i] for i in r if i >= 0] for r in ei]


def test_store_delete_upsert_save_and_filter_mirror(gpu_device, tmp_path):
    import torch
    from rag_fin_amd.store import CorpusStore
    n0 = 6007
    v = osearch.synth_unit_rows(n0, D, 50)
    keys = [f"k{i}" for i in range(n0)]
    st = CorpusStore("t", dim=D, capacity=n0, device=gpu_device)
    st.insert(cols_for(keys, v))
    model = dict(zip(keys, v))                              # pk -> fp16 row, in row order
    st.search(v[:1], limit=3, expr='period == "Q1_FY2024"')  # the filter mirror is synced to all rows

    res = st.delete('period == "Q2_FY2024"')
    gone = [k for k in keys if int(k[1:]) % 4 == 1]
    assert res.delete_count == len(gone) and res.primary_keys == gone
    for k in gone:
        del model[k]
    res = st.delete('id in ["k0", "k6006", "k1", "nope"]')  # k1 is already gone
    assert res.delete_count == 2 and sorted(res.primary_keys) == ["k0", "k6006"]
    del model["k0"], model["k6006"]
    assert st.num_entities == len(model) and st.index.size == len(model)
    assert st.query('id in ["k0", "k2", "k5"]') == [{"id": "k2"}]
    assert st.query('period == "Q2_FY2024"') == []

    # upsert: 3 existing keys with new vectors, 2 new keys
    up_keys = ["k2", "k3", "k4000", "k7001", "k7002"]         # three exist, two are new
    up_v = osearch.synth_unit_rows(5, D, 51)
    assert st.upsert(cols_for(up_keys, up_v, tag="v2")).upsert_count == 5
    for k, r in zip(up_keys, up_v):
        model.pop(k, None)
        model[k] = r
    assert st.num_entities == len(model) and st.columns["id"][-5:] == up_keys
    hits = st.search(torch.from_numpy(up_v).to(gpu_device), limit=1, output_fields=["text"])
    for k, hh in zip(up_keys, hits):
        assert hh[0].id == k and hh[0].entity.text == f"v2:{k}"

    mkeys, mrows = list(model), np.stack(list(model.values()))
    assert st.columns["id"] == mkeys
    q16 = osearch.synth_unit_rows(16, D, 52)
    qt = torch.from_numpy(q16).to(gpu_device)              # fp16 queries are searched as given
    for limit in (10, 100):
        scores, rows = st.search_rows(qt, limit)
        es, ei = c_oracle.search(q16, mrows, limit)
        assert np.array_equal(rows, ei) and np.array_equal(scores, es.astype(np.float32))

    # filter mirror after m deletes + m adds (the collection's length is the same as before)
    m = st.delete('id in ["k8", "k9", "k10"]').delete_count
    for k in ("k8", "k9", "k10"):
        model.pop(k, None)
    add_keys = [f"z{i}" for i in range(m)]
    add_v = osearch.synth_unit_rows(m, D, 53)
    c = cols_for(add_keys, add_v)
    c[3] = ["Q9_FY2099"] * m
    st.insert(c)
    model.update(zip(add_keys, add_v))
    assert [r["id"] for r in st.query('period == "Q9_FY2099"')] == add_keys
    rows_q3 = [j for j, p in enumerate(st.columns["period"]) if p == "Q3_FY2024"]
    assert st.filter_rows('period == "Q3_FY2024"').tolist() == rows_q3
    mkeys, mrows = list(model), np.stack(list(model.values()))
    S = np.array(rows_q3)
    hits = st.search(qt[:4], limit=5, expr='period == "Q3_FY2024"')
    es, ei = c_oracle.search(q16[:4], mrows[S], 5)
    assert [[h.id for h in hh] for hh in hits] == [[mkeys[S[i]] for i in r] for r in ei]

    # save / load after the mutations
    st.save(str(tmp_path / "c"))
    st2 = CorpusStore.load_from(str(tmp_path / "c"), device=gpu_device)
    s1, r1 = st.search_rows(qt, 10)
    s2, r2 = st2.search_rows(qt, 10)
    assert np.array_equal(r1, r2) and np.array_equal(s1, s2) and st2.columns == st.columns
    torch.cuda.synchronize()
    assert torch.equal(live_bytes(st.index, len(model)), live_bytes(st2.index, len(model)))
    assert norm_word(st.index) == norm_word(st2.index)


def test_searches_while_another_thread_upserts(gpu_device):
    """Every hit's text (written as pk|version) must belong to the vector that produced its score."""
    import torch
    from rag_fin_amd.store import CorpusStore
    n0, U, R = 20_000, 64, 12
    v0 = osearch.synth_unit_rows(n0, D, 60)
    keys = [f"k{i}" for i in range(n0)]
    st = CorpusStore("t", dim=D, capacity=n0 + U, device=gpu_device)
    c = cols_for(keys, v0)
    c[1] = [f"{k}|0" for k in keys]
    st.insert(c)
    hot = [f"k{i}" for i in range(0, n0, n0 // U)][:U]
    vers = {0: {k: v0[int(k[1:])] for k in hot}}
    for r in range(1, R + 1):
        vers[r] = dict(zip(hot, osearch.synth_unit_rows(U, D, 1000 + r)))
    q16 = np.stack([vers[0][k] for k in hot[:8]]) + np.stack([vers[R][k] for k in hot[8:16]])
    q16 = osearch.l2_normalize_f32(q16.astype(np.float32)).astype(np.float16)
    qt = torch.from_numpy(q16).to(gpu_device)
    errors, checked = [], [0]

    def searcher(t):
        for it in range(15):
            for b, hh in enumerate(st.search(qt, limit=10 if (t + it) % 2 else 100, output_fields=["text"])):
                for h in hh:
                    pk, ver = h.entity.text.split("|")
                    if pk != h.id:
                        errors.append(("pk", h.id, pk))
                        continue
                    row = vers[int(ver)][pk] if pk in vers[0] else v0[int(pk[1:])]
                    want = np.float32(osearch.exact_scores(q16[b:b + 1], row[None])[0, 0])
                    if np.float32(h.score) != want:
                        errors.append(("score", pk, ver, float(h.score), float(want)))
                    checked[0] += 1

    def upserter():
        for r in range(1, R + 1):
            c = cols_for(hot, np.stack([vers[r][k] for k in hot]))
            c[1] = [f"{k}|{r}" for k in hot]
            st.upsert(c)
    ts = [threading.Thread(target=searcher, args=(t,)) for t in range(3)] + [threading.Thread(target=upserter)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts)
    assert not errors, errors[:5]
    assert checked[0] > 0 and st.num_entities == n0
    assert [r["text"] for r in st.query(f'id in ["{hot[0]}"]', output_fields=["text"])] == [f"{hot[0]}|{R}"]
