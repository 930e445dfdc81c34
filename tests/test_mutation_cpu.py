"""delete(expr) / upsert on CPU: the host bookkeeping of CorpusStore and ShardedCorpusStore with a
CPU double of GpuIndex (fp16 rows in numpy, compact = take the kept rows), the error cases,
service.ingest(upsert=True), the store's readers/writer lock, gloo world-2 / world-3 sharded
delete + upsert against a single-store oracle, and the host-side argument check of
rf_index_compact.  The device side (rf_index_compact, the filter mask, the search) is covered
by tests/test_mutation_gpu.py."""
import os
import socket
import threading
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import search as osearch
from rag_fin_amd import _lib, filter_expr, service
from rag_fin_amd.store import SCALAR_FIELDS, CorpusStore, _RWLock

PERIODS = ["Q1_FY2024", "Q2_FY2024", "Q3_FY2024", "Q4_FY2024"]


class CpuIndex:
    """CPU double of rag_fin_amd.store.GpuIndex: fp16 rows in a numpy array, oracle search."""

    def __init__(self, dim, capacity, device=None):
        self.dim, self.capacity = dim, int(capacity)
        self.device = torch.device("cpu")
        self.rows = np.zeros((0, dim), dtype=np.float16)
        self.compactions = []

    @property
    def size(self):
        return self.rows.shape[0]

    def add(self, rows):
        assert self.size + rows.shape[0] <= self.capacity
        self.rows = np.concatenate([self.rows, rows.numpy().astype(np.float16)])

    def reset(self):
        self.rows = self.rows[:0]

    def get_rows(self, ids):
        return torch.from_numpy(self.rows[np.asarray(ids, dtype=np.int64)])

    def to_fp16(self, x, normalize=True):
        x = np.asarray(x, dtype=np.float32)
        return torch.from_numpy((osearch.l2_normalize_f32(x) if normalize else x).astype(np.float16))

    def compact(self, keep_rows, window_rows=None):
        keep = np.asarray(keep_rows, dtype=np.int64)
        assert keep.size == 0 or (keep[0] >= 0 and keep[-1] < self.size and (np.diff(keep) > 0).all())
        self.compactions.append(keep.copy())
        self.rows = self.rows[keep]

    def search_host(self, q16, k, filt=None):
        assert filt is None
        s, i = osearch.search(q16.numpy(), self.rows, k)
        return s.astype(np.float32), i

    def search_large(self, q16, k, id_base=0, want_exact=False, filt=None):
        s, i = osearch.search(q16.numpy(), self.rows, k, id_base)
        out = (torch.from_numpy(s.astype(np.float32)), torch.from_numpy(i))
        return out + (torch.from_numpy(s),) if want_exact else out


class HostStore(CorpusStore):
    """CorpusStore on the CPU double; the row mask of an expression comes from the parser's host
    reference semantics instead of rf_filter_eval (the device path is the GPU test's)."""

    def __init__(self, dim=32, capacity=16):
        super().__init__("t", dim=dim, capacity=capacity, index=CpuIndex(dim, capacity))

    def _grow(self, need):
        self.index.capacity = max(need, 2 * self.index.capacity)

    def flush(self):
        pass

    def _match_mask(self, expr):
        node = filter_expr.parse(expr)
        return np.array([node.eval({f: self.columns[f][r] for f in SCALAR_FIELDS})
                         for r in range(self.num_entities)], dtype=bool)

    def _expr_rows(self, expr):
        return np.flatnonzero(self._match_mask(expr))


def vecs(n, d, seed):
    return osearch.synth_unit_rows(n, d, seed).astype(np.float32)


def batch(keys, v, tag="v1"):
    n = len(keys)
    return [list(keys), [f"{tag}:{k}" for k in keys], v, [PERIODS[int(k[1:]) % 4] for k in keys],
            ["c"] * n, ["s"] * n, [float(k[1:]) for k in keys]]


def c16_of(v):
    return osearch.l2_normalize_f32(v).astype(np.float16)


class Model:
    """What the collection must hold: pk -> (fp16 row, text), in row order."""

    def __init__(self):
        self.keys, self.rows, self.texts = [], [], []

    def insert(self, b):
        r16 = c16_of(np.asarray(b[2], dtype=np.float32))
        self.keys += b[0]
        self.rows += list(r16)
        self.texts += b[1]

    def delete(self, keys):
        ks = set(keys)
        keep = [j for j, k in enumerate(self.keys) if k not in ks]
        self.keys = [self.keys[j] for j in keep]
        self.rows = [self.rows[j] for j in keep]
        self.texts = [self.texts[j] for j in keep]

    def upsert(self, b):
        self.delete(b[0])
        self.insert(b)

    def matrix(self, d):
        return np.array(self.rows, dtype=np.float16).reshape(-1, d)


def check_store(st, model, d, seed=99):
    assert st.num_entities == len(model.keys) == st.index.size
    assert st.columns["id"] == model.keys and st.columns["text"] == model.texts
    assert all(len(st.columns[f]) == len(model.keys) for f in SCALAR_FIELDS)
    assert st._pk_row == {k: j for j, k in enumerate(model.keys)}
    assert np.array_equal(st.index.rows.view(np.uint16), model.matrix(d).view(np.uint16))
    q = vecs(5, d, seed)
    q16 = c16_of(q)
    for limit in (7, 100):
        s, r = st.search_rows(q, limit)
        ws, wi = osearch.search(q16, model.matrix(d), limit)
        kk = min(limit, len(model.keys))
        assert np.array_equal(r, wi[:, :kk]) and np.array_equal(s, ws[:, :kk].astype(np.float32))
    hits = st.search(q[:2], limit=3, output_fields=["id", "text"])
    for b, hh in enumerate(hits):
        for h in hh:
            assert h.entity.text == model.texts[model.keys.index(h.id)]


def test_delete_by_expression_and_by_keys_bookkeeping():
    d = 32
    st, m = HostStore(d), Model()
    for lo, hi in ((0, 70), (70, 203)):
        b = batch([f"k{i}" for i in range(lo, hi)], vecs(hi - lo, d, lo + 1))
        st.insert(b)
        m.insert(b)
    res = st.delete('period == "Q2_FY2024"')
    gone = [k for k in m.keys if int(k[1:]) % 4 == 1]
    m.delete(gone)
    assert res.delete_count == len(gone) == len(res.primary_keys) and res.primary_keys == gone
    check_store(st, m, d)
    assert st.query('id in ["k1", "k2", "k5"]') == [{"id": "k2"}]
    res = st.delete('id in ["k0", "k202", "nope", "k0"]')
    m.delete(["k0", "k202"])
    assert res.delete_count == 2 and sorted(res.primary_keys) == ["k0", "k202"]
    check_store(st, m, d)
    # a run of rows, then everything but one
    run = [k for k in m.keys if 40 <= int(k[1:]) < 120]
    assert st.delete("primary_value >= 40 and primary_value < 120").delete_count == len(run)
    m.delete(run)
    check_store(st, m, d)
    keep1 = m.keys[17]
    st.delete(f'id != "{keep1}"')
    m.delete([k for k in m.keys if k != keep1])
    check_store(st, m, d)


def test_delete_that_matches_nothing_touches_nothing():
    d = 32
    st = HostStore(d)
    st.insert(batch([f"k{i}" for i in range(40)], vecs(40, d, 3)))
    cols = {f: list(c) for f, c in st.columns.items()}
    res = st.delete('period == "Q9_FY2099"')
    assert res.delete_count == 0 and res.primary_keys == []
    assert st.index.compactions == [] and st.columns == cols
    assert st.delete('id in ["nope"]').delete_count == 0 and st.index.compactions == []


def test_upsert_replaces_existing_keys_at_the_end_and_appends_new_ones():
    d = 32
    st, m = HostStore(d), Model()
    b = batch([f"k{i}" for i in range(50)], vecs(50, d, 5))
    st.insert(b)
    m.insert(b)
    up = batch(["k3", "k60", "k10", "k61"], vecs(4, d, 6), tag="v2")
    res = st.upsert(up)
    m.upsert(up)
    assert res.upsert_count == 4 and res.primary_keys == ["k3", "k60", "k10", "k61"]
    assert st.num_entities == 52 and st.columns["id"][-4:] == ["k3", "k60", "k10", "k61"]
    assert st.query('id in ["k3"]', output_fields=["text"]) == [{"text": "v2:k3", "id": "k3"}]
    check_store(st, m, d)
    # same keys again: count unchanged
    up2 = batch(["k61", "k3"], vecs(2, d, 7), tag="v3")
    st.upsert(up2)
    m.upsert(up2)
    assert st.num_entities == 52
    check_store(st, m, d)


def test_errors_leave_the_collection_as_it_was():
    d = 32
    st = HostStore(d)
    st.insert(batch([f"k{i}" for i in range(20)], vecs(20, d, 8)))
    before = {f: list(c) for f, c in st.columns.items()}
    for bad in ("", "   ", None):
        with pytest.raises(ValueError, match="non-empty"):
            st.delete(bad)
    with pytest.raises(ValueError):
        st.delete('colour == "red"')                        # unknown field
    with pytest.raises(ValueError):
        st.delete("period ==")                              # malformed
    with pytest.raises(ValueError, match="duplicate"):
        st.upsert(batch(["k1", "k30", "k1"], vecs(3, d, 9)))
    with pytest.raises(ValueError, match="embeddings"):
        st.upsert(batch(["k1", "k2"], vecs(3, d, 9)))       # 2 keys, 3 vectors: nothing may be deleted first
    with pytest.raises(ValueError, match="7 columns"):
        st.upsert(batch(["k1"], vecs(1, d, 9))[:6])
    with pytest.raises(ValueError, match="duplicate primary key"):
        st.insert(batch(["k4"], vecs(1, d, 9)))             # insert still refuses an existing key
    assert st.columns == before and st.index.compactions == []


def test_unknown_field_is_refused_by_the_real_mask_path_without_a_gpu():
    # CorpusStore._match_mask itself (no host override): the expression is parsed before any device work
    d = 32
    st = CorpusStore("t", dim=d, capacity=8, index=CpuIndex(d, 8))
    with pytest.raises(ValueError):
        st.delete('colour == "red"')
    assert st.delete('period == "Q1_FY2024"').delete_count == 0     # empty collection: a no-op


class FakeEmbedder:
    """encode_to_device: a deterministic fp16 unit vector per text (CPU)."""

    dim = 32

    def encode_to_device(self, texts):
        out = np.stack([c16_of(vecs(1, self.dim, sum(t.encode()) % 100_000 + 1))[0] for t in texts])
        return torch.from_numpy(out)


def chunks_of(quarter, n, tag):
    return [{"id": f"{quarter}_c{j}", "text": f"{tag} {quarter} chunk {j}", "period": quarter, "chunk_type": "c",
             "statement_type": "s", "primary_value": float(j)} for j in range(n)]


def test_ingest_upsert_is_idempotent_and_replaces_a_restated_quarter():
    st = HostStore(FakeEmbedder.dim)
    emb = FakeEmbedder()
    q1, q2 = chunks_of("Q1_FY2024", 12, "orig"), chunks_of("Q2_FY2024", 9, "orig")
    assert service.ingest(st, emb, q1 + q2) == 21
    with pytest.raises(ValueError, match="duplicate primary key"):
        service.ingest(st, emb, q2)
    q = vecs(3, FakeEmbedder.dim, 4)
    s0, r0 = st.search_rows(q, 5)
    assert service.ingest(st, emb, q2, upsert=True) == 9          # same chunks again
    assert st.num_entities == 21
    s1, r1 = st.search_rows(q, 5)
    assert np.array_equal(s0, s1)
    assert [st.columns["id"][r] for r in r0.ravel()] == [st.columns["id"][r] for r in r1.ravel()]
    restated = chunks_of("Q2_FY2024", 7, "restated")             # fewer chunks after the restatement
    service.ingest(st, emb, restated, upsert=True)
    assert st.num_entities == 21                                   # 7 replaced; Q2 c7, c8 remain
    got = {r["id"]: r["text"] for r in st.query('period == "Q2_FY2024"', output_fields=["id", "text"])}
    assert got["Q2_FY2024_c0"].startswith("restated") and got["Q2_FY2024_c8"].startswith("orig")


# ---- the store's readers/writer lock -------------------------------------------------------------------
def test_rwlock_readers_share_writers_exclude_and_reentry_works():
    lk = _RWLock()
    inside, peak, log = [0], [0], []
    gate = threading.Barrier(3)

    def reader():
        with lk.read():
            inside[0] += 1
            gate.wait(timeout=10)          # all three readers are in at once, or this times out
            peak[0] = max(peak[0], inside[0])
            with lk.read():                # re-entry
                pass
            inside[0] -= 1
    ts = [threading.Thread(target=reader) for _ in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=20)
    assert peak[0] == 3

    with lk.write():
        with lk.write(), lk.read():        # a writer may write and read again
            pass
    with lk.read():
        with pytest.raises(RuntimeError):
            with lk.write():
                pass

    hold = threading.Event()

    def writer():
        with lk.write():
            log.append("w-in")
            hold.wait(timeout=10)
            log.append("w-out")

    def late_reader():
        with lk.read():
            log.append("r")
    w = threading.Thread(target=writer)
    w.start()
    while "w-in" not in log:
        time.sleep(0.001)
    r = threading.Thread(target=late_reader)
    r.start()
    time.sleep(0.05)
    assert log == ["w-in"]                 # the reader waits for the writer
    hold.set()
    w.join(timeout=10)
    r.join(timeout=10)
    assert log == ["w-in", "w-out", "r"]


def test_search_waits_for_a_running_delete():
    """A delete holds the write lock over index + columns: a search started meanwhile sees the
    collection before or after it, never in between."""
    d = 32
    st, m = HostStore(d), Model()
    b = batch([f"k{i}" for i in range(64)], vecs(64, d, 12))
    st.insert(b)
    m.insert(b)
    in_compact, release = threading.Event(), threading.Event()
    orig = st.index.compact

    def slow_compact(keep, window_rows=None):
        orig(keep, window_rows)
        in_compact.set()
        release.wait(timeout=10)           # index compacted, host columns not yet
    st.index.compact = slow_compact
    t = threading.Thread(target=st.delete, args=('id in ["k0", "k1", "k2"]',))
    t.start()
    assert in_compact.wait(timeout=10)
    out = {}
    s = threading.Thread(target=lambda: out.update(h=st.search(vecs(1, d, 13), limit=5, output_fields=["text"])))
    s.start()
    time.sleep(0.05)
    assert not out                          # blocked behind the writer
    release.set()
    t.join(timeout=10)
    s.join(timeout=10)
    m.delete(["k0", "k1", "k2"])
    for h in out["h"][0]:
        assert h.entity.text == m.texts[m.keys.index(h.id)]
    check_store(st, m, d)


def test_rf_index_compact_refuses_a_null_index_without_a_gpu():
    lib = _lib.load_library()
    assert lib.rf_index_compact(None, None, 0, None, 0, None) == -1
    assert b"null index" in lib.rf_last_error()


# ---- ShardedCorpusStore: COLLECTIVE delete / upsert under gloo ------------------------------------------
class OracleBackend:
    def __init__(self, index):
        self.index = index

    def local_topk(self, q16, k, row_base, workspace=None):
        s, i = osearch.search(q16.numpy(), self.index.rows, k, id_base=row_base)
        return torch.from_numpy(s), torch.from_numpy(i), torch.zeros(q16.shape[0], dtype=torch.int32)

    def local_exhaustive(self, q16, k, row_base):
        s, i = osearch.search(q16.numpy(), self.index.rows, k, id_base=row_base)
        return torch.from_numpy(s), torch.from_numpy(i)

    def merge(self, exact_all, ids_all, k):
        s, i = osearch.merge_shards(exact_all.numpy(), ids_all.numpy(), k)
        return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(i)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


D_SH = 48


def _script():
    """The operations of the sharded run, replayed on a Model for the expected state."""
    steps = [("insert", batch([f"k{i}" for i in range(0, 90)], vecs(90, D_SH, 31))),
             ("insert", batch([f"k{i}" for i in range(90, 91)], vecs(1, D_SH, 32))),
             ("insert", batch([f"k{i}" for i in range(91, 211)], vecs(120, D_SH, 33))),
             ("delete", [f"k{i}" for i in range(0, 45)] + ["k90", "k150", "nope"]),   # rank 0's first slice, mostly
             ("upsert", batch(["k100", "k300", "k46", "k301", "k302"], vecs(5, D_SH, 34), tag="v2")),
             ("delete", [f"k{i}" for i in range(160, 211)]),
             ("insert", batch([f"k{i}" for i in range(400, 407)], vecs(7, D_SH, 35)))]
    return steps


def _sharded_worker(rank, world, port, out_dir):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = ShardedCorpusStore("t", dim=D_SH, capacity=8, index=CpuIndex(D_SH, 8), backend=None)
        st._grow = lambda need: setattr(st.index, "capacity", max(need, 2 * st.index.capacity))
        st._backend_factory = lambda index: OracleBackend(index)
        q = vecs(6, D_SH, 36)
        res, local_sizes = [], []
        for op, arg in _script():
            if op == "insert":
                st.insert(arg)
            elif op == "delete":
                res.append(st.delete("id in [" + ", ".join(repr(k) for k in arg) + "]").delete_count)
            else:
                res.append(st.upsert(arg).upsert_count)
            local_sizes.append(st.local_rows)
        errs = []
        for bad in ('period == "Q1_FY2024"', ""):
            try:
                st.delete(bad)
            except (NotImplementedError, ValueError) as e:
                errs.append(type(e).__name__)
        s10, r10 = st.search_rows(q, 10)
        s100, r100 = st.search_rows(q[:3], 100)
        hits = st.search(q[:2], limit=4, output_fields=["text"])
        st.save(os.path.join(out_dir, "corpus"))
        st2 = ShardedCorpusStore.load_from(os.path.join(out_dir, "corpus"), index_factory=CpuIndex, backend=None)
        st2._backend_factory = lambda index: OracleBackend(index)
        s2, r2 = st2.search_rows(q, 10)
        np.savez(os.path.join(out_dir, f"m{rank}.npz"), res=np.array(res), local_sizes=np.array(local_sizes),
                 errs=np.array(errs), s10=s10, r10=r10, s100=s100, r100=r100, s2=s2, r2=r2,
                 ids=np.array(st.columns["id"]), id_map=st._id_map.numpy(),
                 hit_ids=np.array([[h.id for h in hh] for hh in hits]),
                 hit_text=np.array([[h.entity.text for h in hh] for hh in hits]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_delete_and_upsert_equal_a_single_store(tmp_path, world):
    mp.spawn(_sharded_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    m, counts = Model(), []
    for op, arg in _script():
        if op == "insert":
            m.insert(arg)
        elif op == "delete":
            counts.append(sum(k in m.keys for k in set(arg)))
            m.delete(arg)
        else:
            counts.append(len(arg[0]))
            m.upsert(arg)
    c16 = m.matrix(D_SH)
    q16 = c16_of(vecs(6, D_SH, 36))
    ws, wi = osearch.search(q16, c16, 10)
    wbs, wbi = osearch.search(q16[:3], c16, 100)
    kk = min(100, len(m.keys))
    all_maps, sizes = [], None
    for r in range(world):
        z = np.load(tmp_path / f"m{r}.npz")
        assert z["res"].tolist() == counts
        assert z["errs"].tolist() == ["NotImplementedError", "ValueError"]
        assert z["ids"].tolist() == m.keys
        assert np.array_equal(z["r10"], wi) and np.array_equal(z["s10"], ws.astype(np.float32)), f"rank {r}"
        assert np.array_equal(z["r100"], wbi[:, :kk]) and np.array_equal(z["s100"], wbs[:, :kk].astype(np.float32))
        assert np.array_equal(z["r2"], wi) and np.array_equal(z["s2"], ws.astype(np.float32))
        assert z["hit_ids"].tolist() == [[m.keys[i] for i in wi[b][:4]] for b in range(2)]
        assert z["hit_text"].tolist() == [[m.texts[i] for i in wi[b][:4]] for b in range(2)]
        all_maps.append(z["id_map"])
        sizes = z["local_sizes"] if sizes is None else sizes + z["local_sizes"]
    # every global row is owned by exactly one rank, and the shards ended up uneven
    assert sorted(np.concatenate(all_maps).tolist()) == list(range(len(m.keys)))
    assert len({len(a) for a in all_maps}) > 1
    # the saved corpus is the single-GPU format, in global row order
    mm = np.fromfile(tmp_path / "corpus" / "vectors.f16", dtype=np.float16).reshape(-1, D_SH)
    assert np.array_equal(mm.view(np.uint16), c16.view(np.uint16))


# ---- one ingest check: a bad batch is refused whole, by either store, for insert and upsert --------------
D_BAD = 32


def _plain_store():
    return CorpusStore("t", dim=D_BAD, capacity=16, index=CpuIndex(D_BAD, 16))


def _sharded_store_world_1(tmp_path):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    return ShardedCorpusStore("t", dim=D_BAD, capacity=16, index=CpuIndex(D_BAD, 16))


def _bad_batch(case, what):
    """Batches of 3 for a store that holds k0 .. k4; an upsert batch replaces k1, so a delete made
    before the refusal would show."""
    keys = ["k5", "k6", "k7"] if what == "insert" else ["k1", "k5", "k6"]
    if case == "a key twice in the batch":
        keys[2] = keys[0]
    if case == "a key already present":
        keys[1] = "k3"
    n_vec, d_vec = (2 if case == "embeddings [n - 1, dim]" else 3), (D_BAD + 1 if case == "embeddings [n, dim + 1]" else D_BAD)
    b = batch(keys, vecs(n_vec, d_vec, 41))
    if case == "a column one short":
        b[3] = b[3][:-1]
    return b[:6] if case == "6 columns" else b


BAD_CASES = ["a column one short", "a key twice in the batch", "embeddings [n, dim + 1]", "embeddings [n - 1, dim]",
             "6 columns"]


BAD_PARAMS = [(w, c) for w in ("insert", "upsert") for c in BAD_CASES] + [("insert", "a key already present")]


@pytest.mark.parametrize("what,case", BAD_PARAMS)
@pytest.mark.parametrize("kind", ["CorpusStore", "ShardedCorpusStore"])
def test_a_bad_batch_is_refused_and_changes_nothing(tmp_path, kind, what, case):
    try:
        st = _plain_store() if kind == "CorpusStore" else _sharded_store_world_1(tmp_path)
        st.insert(batch([f"k{i}" for i in range(5)], vecs(5, D_BAD, 40)))
        before = ({f: list(c) for f, c in st.columns.items()}, dict(st._pk_row), st.index.rows.copy())
        with pytest.raises(ValueError):
            getattr(st, what)(_bad_batch(case, what))
        assert st.num_entities == 5 == st.index.size
        assert st.columns == before[0] and all(len(c) == 5 for c in st.columns.values())
        assert st._pk_row == before[1] == {f"k{i}": i for i in range(5)}
        assert np.array_equal(st.index.rows.view(np.uint16), before[2].view(np.uint16)) and st.index.compactions == []
        if kind == "ShardedCorpusStore":
            assert st._id_map.tolist() == list(range(5))
        # the batch without its fault goes through
        getattr(st, what)(_bad_batch(None, what))
        assert st.num_entities == (8 if what == "insert" else 7) == st.index.size
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _bad_batch_worker(rank, world, port, out_dir):
    from rag_fin_amd.sharded_store import ShardedCorpusStore
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = ShardedCorpusStore("t", dim=D_BAD, capacity=16, index=CpuIndex(D_BAD, 16))
        st.insert(batch([f"k{i}" for i in range(5)], vecs(5, D_BAD, 40)))
        rows0, refused, unchanged = st.index.rows.copy(), [], []
        for what, case in BAD_PARAMS:
            try:
                getattr(st, what)(_bad_batch(case, what))
                refused.append(False)
            except ValueError:
                refused.append(True)
            unchanged.append(st.columns["id"] == [f"k{i}" for i in range(5)] and
                             all(len(c) == 5 for c in st.columns.values()) and
                             st._pk_row == {f"k{i}": i for i in range(5)} and st.index.compactions == [] and
                             np.array_equal(st.index.rows.view(np.uint16), rows0.view(np.uint16)))
        np.savez(os.path.join(out_dir, f"bad{rank}.npz"), refused=np.array(refused), unchanged=np.array(unchanged),
                 id_map=st._id_map.numpy())
    finally:
        dist.destroy_process_group()


def test_a_bad_batch_is_refused_by_every_rank_of_a_sharded_store(tmp_path):
    """World 2, batches of 3: rank 0 owns rows [0, 2) of a batch and rank 1 row 2, so a whole
    embedding column that is one row short would pass a check of rank 0's slice alone.  Every rank
    must refuse every case, or the ranks' columns and id maps part ways."""
    mp.spawn(_bad_batch_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    maps = []
    for r in range(2):
        z = np.load(tmp_path / f"bad{r}.npz")
        assert z["refused"].all(), (r, [p for p, ok in zip(BAD_PARAMS, z["refused"]) if not ok])
        assert z["unchanged"].all(), (r, [p for p, ok in zip(BAD_PARAMS, z["unchanged"]) if not ok])
        maps.append(z["id_map"].tolist())
    assert maps == [[0, 1, 2], [3, 4]]


# ---- one loader, one metadata writer: the directory is the one the format's first version wrote ----------
GOLD_STORE = os.path.join(os.path.dirname(__file__), "golden", "store_v1")


class LoadableHostStore(HostStore):
    """HostStore with the constructor signature load_from calls."""

    def __init__(self, name="t", dim=32, capacity=16, device=None, metric_type="COSINE"):
        CorpusStore.__init__(self, name, dim=dim, capacity=capacity, metric_type=metric_type,
                             index=CpuIndex(dim, capacity))


def golden_store():
    """The 5-row, dim-32 store whose saved directory is tests/golden/store_v1."""
    st = LoadableHostStore()
    st.insert(batch([f"k{i}" for i in range(5)], vecs(5, 32, 50), tag="gold"))
    return st


def test_save_load_save_is_byte_identical_to_the_recorded_directory(tmp_path):
    def files(path):
        return {name: open(os.path.join(path, name), "rb").read() for name in ("vectors.f16", "columns.json")}
    want = files(GOLD_STORE)
    assert len(want["vectors.f16"]) == 5 * 32 * 2
    st = golden_store()
    st.save(str(tmp_path / "a"))
    assert sorted(os.listdir(tmp_path / "a")) == ["columns.json", "vectors.f16"]
    assert files(tmp_path / "a") == want
    st2 = LoadableHostStore.load_from(str(tmp_path / "a"))
    assert st2.columns == st.columns and st2._pk_row == st._pk_row and st2.name == "t" and st2.index_type == "FLAT"
    assert np.array_equal(st2.index.rows.view(np.uint16), st.index.rows.view(np.uint16))
    st2.save(str(tmp_path / "b"))
    assert files(tmp_path / "b") == want
