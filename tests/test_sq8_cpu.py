"""The SQ8 index type on CPU: CorpusStore.create_index / drop_index / has_index argument checks on a
CPU double of GpuIndex, the reference's exact IVF_FLAT call, the index_type key of columns.json,
the sharded store's refusal of SQ8, and the new C symbols with their host-side checks.  The
device side (quantizer, bound, exact search) is tests/test_sq8_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import search as osearch
from rag_fin_amd import _lib
from rag_fin_amd.sharded_store import ShardedCorpusStore
from rag_fin_amd.store import CorpusStore

SQ8_SYMBOLS = ["rf_sq8_storage_bytes", "rf_index_attach_sq8", "rf_index_detach_sq8",
               "rf_search_sq8_workspace_bytes", "rf_search_sq8", "rf_search_sq8_profile",
               "rf_debug_scores_sq8", "rf_index_get_rows_sq8"]


class CpuIndex:
    """CPU double of GpuIndex with the SQ8 switch: records enable / disable, searches with the oracle."""

    def __init__(self, dim, capacity, device=None):
        self.dim, self.capacity = dim, int(capacity)
        self.device = torch.device("cpu")
        self.rows = np.zeros((0, dim), dtype=np.float16)
        self.sq8 = False
        self.calls = []

    @property
    def size(self):
        return self.rows.shape[0]

    def add(self, rows):
        self.rows = np.concatenate([self.rows, rows.numpy().astype(np.float16)])

    def reset(self):
        self.rows = self.rows[:0]

    def get_rows(self, ids):
        return torch.from_numpy(self.rows[np.asarray(ids, dtype=np.int64)])

    def to_fp16(self, x, normalize=True):
        x = np.asarray(x, dtype=np.float32)
        return torch.from_numpy((osearch.l2_normalize_f32(x) if normalize else x).astype(np.float16))

    def enable_sq8(self):
        if self.dim % 32:
            raise _lib.RagfinError(-2, "SQ8 needs dim % 32 == 0")
        self.sq8 = True

    def disable_sq8(self):
        self.sq8 = False

    def search_host(self, q16, k, filt=None, sq8=False):
        self.calls.append(("host", int(q16.shape[0]), k, sq8))
        s, i = osearch.search(q16.numpy(), self.rows, k)
        return s.astype(np.float32), i

    def search_large(self, q16, k, id_base=0, want_exact=False, filt=None):
        self.calls.append(("large", int(q16.shape[0]), k, False))
        s, i = osearch.search(q16.numpy(), self.rows, k, id_base)
        return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(i)


class HostStore(CorpusStore):
    def __init__(self, dim=64, capacity=64, metric_type="COSINE"):
        super().__init__("t", dim=dim, capacity=capacity, metric_type=metric_type, index=CpuIndex(dim, capacity))

    def _grow(self, need):
        self.index.capacity = max(need, 2 * self.index.capacity)

    def flush(self):
        pass


def fill(st, n, seed=1):
    v = np.random.default_rng(seed).standard_normal((n, st.dim)).astype(np.float32)
    st.insert([list(range(n)), [f"t{i}" for i in range(n)], v, ["Q1_FY2024"] * n, ["table"] * n,
               ["income"] * n, [float(i) for i in range(n)]])
    return v


def test_reference_ivf_flat_call_is_accepted_and_served_as_flat():
    st = HostStore()
    assert not st.has_index()
    # "chunking_storing (1).py":29, verbatim
    st.create_index("embedding", {"index_type": "IVF_FLAT", "metric_type": "COSINE", "params": {"nlist": 128}})
    assert st.has_index() and st.index_type == "FLAT" and not st.index.sq8
    fill(st, 20)
    st.search(np.ones((1, 64), np.float32), limit=3)
    assert st.index.calls[-1] == ("host", 1, 3, False)


def test_create_index_validation():
    st = HostStore()
    with pytest.raises(ValueError, match="index_type"):
        st.create_index("embedding", {"index_type": "HNSW", "metric_type": "COSINE"})
    with pytest.raises(ValueError, match="COSINE"):
        st.create_index("embedding", {"index_type": "SQ8", "metric_type": "IP"})
    with pytest.raises(ValueError, match="field"):
        st.create_index("text", {"index_type": "FLAT"})
    with pytest.raises(ValueError, match="params"):
        st.create_index("embedding", {"index_type": "FLAT", "params": 3})
    assert not st.has_index() and st.index_type == "FLAT" and not st.index.sq8
    st.create_index("embedding", {"index_type": "flat"})        # case-insensitive, metric defaults
    assert st.has_index() and st.index_type == "FLAT"
    ip = HostStore(metric_type="IP")
    ip.create_index("embedding", {"index_type": "SQ8", "metric_type": "IP"})
    assert ip.index_type == "SQ8" and ip.index.sq8


def test_sq8_switch_and_routing():
    st = HostStore()
    fill(st, 40)
    st.create_index("embedding", {"index_type": "SQ8", "metric_type": "COSINE"})
    assert st.has_index() and st.index_type == "SQ8" and st.index.sq8
    q = np.random.default_rng(5).standard_normal((3, 64)).astype(np.float32)
    st.search(q, limit=5)
    assert st.index.calls[-1] == ("host", 3, 5, True)
    st.search(q, limit=64)
    assert st.index.calls[-1] == ("host", 3, 64, True)
    st.search(q, limit=65)                                       # k > RF_MAX_K: FLAT pages
    assert st.index.calls[-1][0] == "large"
    st.search(np.tile(q, (22, 1)), limit=5)                      # B = 66 > 64: FLAT
    assert st.index.calls[-1] == ("host", 66, 5, False)
    st.search(np.tile(q, (22, 1))[:64], limit=5)                 # B = 64: SQ8
    assert st.index.calls[-1] == ("host", 64, 5, True)
    st.drop_index()
    assert not st.has_index() and st.index_type == "FLAT" and not st.index.sq8
    st.search(q, limit=5)
    assert st.index.calls[-1] == ("host", 3, 5, False)


def test_sq8_refused_for_dim_not_multiple_of_32():
    st = HostStore(dim=48)
    with pytest.raises(_lib.RagfinError):
        st.create_index("embedding", {"index_type": "SQ8"})
    assert st.index_type == "FLAT" and not st.has_index()


def test_columns_json_index_type(tmp_path):
    st = HostStore()
    fill(st, 10)
    st.save(str(tmp_path / "flat"))
    st.create_index("embedding", {"index_type": "IVF_FLAT", "metric_type": "COSINE", "params": {"nlist": 128}})
    st.save(str(tmp_path / "ivf"))
    for d in ("flat", "ivf"):
        meta = json.load(open(tmp_path / d / "columns.json"))
        assert "index_type" not in meta
        assert set(meta) == {"format", "name", "dim", "metric_type", "n", "columns"}
    st.create_index("embedding", {"index_type": "SQ8", "metric_type": "COSINE"})
    st.save(str(tmp_path / "sq8"))
    meta = json.load(open(tmp_path / "sq8" / "columns.json"))
    assert meta["index_type"] == "SQ8"
    assert open(tmp_path / "sq8" / "vectors.f16", "rb").read() == open(tmp_path / "flat" / "vectors.f16", "rb").read()


def test_sharded_store_accepts_flat_and_refuses_sq8():
    st = HostStore()
    ShardedCorpusStore.create_index(st, "embedding", {"index_type": "IVF_FLAT", "metric_type": "COSINE",
                                                      "params": {"nlist": 128}})
    assert st.has_index() and st.index_type == "FLAT"
    with pytest.raises(NotImplementedError):
        ShardedCorpusStore.create_index(st, "embedding", {"index_type": "SQ8", "metric_type": "COSINE"})
    with pytest.raises(ValueError):
        ShardedCorpusStore.create_index(st, "embedding", {"index_type": "DISKANN"})
    assert not st.index.sq8


def test_sq8_symbols_exported_and_host_checks():
    lib = _lib.load_library()
    for name in SQ8_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    # dim 384: 12 KiB of int8 fragments + 256 B of {s_r, e_r} per 32-row block, + the tracker words
    assert lib.rf_sq8_storage_bytes(384, 1000) == 32 * (12 * 1024 + 256) + 256
    assert lib.rf_sq8_storage_bytes(768, 32) == 24 * 1024 + 256 + 256
    for dim in (48, 80, 400, 16):
        assert lib.rf_sq8_storage_bytes(dim, 1000) == 0          # dim % 32 != 0 is refused
    assert lib.rf_sq8_storage_bytes(384, 0) == 0
    # the FLAT sizes stay what they were; the SQ8 workspace is the FLAT one plus its query area
    assert lib.rf_index_storage_bytes(384, 1000) == 32 * 24 * 1024 + 256
    assert lib.rf_search_sq8_workspace_bytes(None) > lib.rf_search_workspace_bytes(None)
    assert lib.rf_index_attach_sq8(None, None, 0, None) == -1
    assert lib.rf_index_detach_sq8(None) == -1
    assert lib.rf_index_get_rows_sq8(None, None, 0, None, None, None, None) == -1
    assert lib.rf_debug_scores_sq8(None, None, 1, 1, None, None, None, 0, None) == -1
    assert lib.rf_search_sq8(None, None, 1, 10, 0, None, None, None, None, None, 0, None) == -1


# ---- the flagged-query ladder with stand-in tiers (store.rerun_flagged; DESIGN §4.4b, "fallback") ----
class Tiers:
    """Stand-ins for the FLAT chain and the exhaustive kernel: each records the queries it was given
    (a query is the row [j, j, ...]) and answers with its own mark, FLAT flagging `flat_flags`."""

    def __init__(self, flat_flags=()):
        self.flat_flags = set(flat_flags)
        self.flat_ran, self.exhaustive_ran, self.filters = [], [], []

    @staticmethod
    def rows(q, k, mark):
        n = q.shape[0]
        qi = q[:, 0].to(torch.int64)
        return (torch.full((n, k), float(mark), dtype=torch.float32) + qi[:, None].float(),
                torch.full((n, k), mark, dtype=torch.int64) + qi[:, None],
                torch.full((n, k), float(mark), dtype=torch.float64) + qi[:, None].double())

    def flat(self, q, k, id_base):
        qi = [int(v) for v in q[:, 0]]
        self.flat_ran.append(qi)
        flags = torch.tensor([1 if j in self.flat_flags else 0 for j in qi], dtype=torch.int32)
        return self.rows(q, k, 1000) + (flags,)

    def exhaustive(self, q, k, id_base, filt):
        self.exhaustive_ran.append([int(v) for v in q[:, 0]])
        self.filters.append(filt)
        return self.rows(q, k, 2000)


def ladder(flags, sq8, filt, tiers, k=3):
    from rag_fin_amd.store import rerun_flagged
    q = torch.arange(8, dtype=torch.float16)[:, None].repeat(1, 4)
    out = [torch.zeros((8, k), dtype=torch.float32), torch.zeros((8, k), dtype=torch.int64),
           torch.zeros((8, k), dtype=torch.float64)]
    f = torch.zeros(8, dtype=torch.int32)
    f[list(flags)] = 1
    bad, rows = rerun_flagged(q, k, 0, f, sq8, filt, tiers.flat, tiers.exhaustive)
    if rows is not None:
        for dst, src in zip(out, rows):
            dst[bad] = src
    return bad, rows, out


def test_ladder_sq8_first_pass_goes_through_flat_then_exhaustive():
    t = Tiers(flat_flags={4})
    bad, rows, (s, i, e) = ladder({1, 4, 6}, True, None, t)
    assert bad.tolist() == [1, 4, 6]
    assert t.flat_ran == [[1, 4, 6]]                 # FLAT ran on exactly the SQ8-flagged queries
    assert t.exhaustive_ran == [[4]]                 # the exhaustive kernel on exactly what FLAT flagged too
    for r in (0, 2, 3, 5, 7):                        # untouched
        assert not s[r].any() and not i[r].any() and not e[r].any()
    # each patched row holds the value of the last tier that ran it
    for r, mark in ((1, 1000), (4, 2000), (6, 1000)):
        assert i[r].tolist() == [mark + r] * 3
        assert s[r].tolist() == [float(mark + r)] * 3 and e[r].tolist() == [float(mark + r)] * 3


@pytest.mark.parametrize("filt", [None, "the-filter"])
def test_ladder_flat_or_filtered_first_pass_goes_straight_to_exhaustive(filt):
    t = Tiers()
    bad, rows, (s, i, e) = ladder({2}, False, filt, t)
    assert bad.tolist() == [2]
    assert t.flat_ran == [] and t.exhaustive_ran == [[2]]
    assert t.filters == [filt]                       # the exhaustive tier receives the filter
    assert i[2].tolist() == [2002] * 3 and s[2].tolist() == [2002.0] * 3
    assert not i[[0, 1, 3, 4, 5, 6, 7]].any()


@pytest.mark.parametrize("sq8", [False, True])
def test_ladder_without_flags_runs_no_tier(sq8):
    t = Tiers()
    bad, rows, (s, i, e) = ladder((), sq8, None, t)
    assert bad.numel() == 0 and rows is None
    assert t.flat_ran == [] and t.exhaustive_ran == []
    assert not s.any() and not i.any() and not e.any()
