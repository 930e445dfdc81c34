"""Shadow-first FLAT search without a GPU: the new entry points are exported and declared, their
host-side argument checks, the workspace-size orderings, and the GpuIndex `shadow` policy against a
stand-in for the library."""
import contextlib
import ctypes
import os
import re

import pytest
import torch

from rag_fin_amd import _lib
from rag_fin_amd import index as rindex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RF_ERR_INVALID = -1


def test_symbols_exported_and_declared():
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "ragfin.h")).read()
    for name in ("rf_index_set_shadow_first", "rf_search_fp16"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
    assert _lib.SIGNATURES["rf_search_fp16"] == _lib.SIGNATURES["rf_search"]


def test_host_side_argument_checks():
    lib = _lib.load_library()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every case below fails its checks first
    big = 1 << 30
    assert lib.rf_index_set_shadow_first(None, 1) == RF_ERR_INVALID and b"null" in lib.rf_last_error()
    assert lib.rf_search_fp16(None, fake, 1, 10, 0, fake, fake, None, fake, fake, big, None) == RF_ERR_INVALID
    assert lib.rf_search_fp16(fake, None, 1, 10, 0, fake, fake, None, fake, fake, big, None) == RF_ERR_INVALID
    assert lib.rf_search_fp16(fake, fake, 0, 10, 0, fake, fake, None, fake, fake, big, None) == RF_ERR_INVALID
    assert lib.rf_search_fp16(fake, fake, 1, _lib.RF_MAX_K + 1, 0, fake, fake, None, fake, fake, big, None) != 0
    assert lib.rf_search_fp16(fake, ctypes.c_void_p(4100), 1, 10, 0, fake, fake, None, fake, fake, big, None) == RF_ERR_INVALID
    assert lib.rf_search_fp16(fake, fake, 1, 10, 0, fake, fake, None, fake, fake, 16, None) != 0   # workspace too small
    assert b"workspace" in lib.rf_last_error()


def test_workspace_size_orderings():
    lib = _lib.load_library()
    flat, sq8, grouped = (lib.rf_search_workspace_bytes(None), lib.rf_search_sq8_workspace_bytes(None),
                          lib.rf_search_grouped_workspace_bytes(None))
    assert grouped > sq8 > flat > 4 * 1024 * 1024    # a null index has no shadow: the FLAT size


# ---- GpuIndex(shadow=...) against a stand-in library -------------------------------------------------
class FakeLib:
    FLAT, SQ8, GROUPED = 1000, 1500, 2000

    def __init__(self):
        self.reset()

    def reset(self):   # (one stand-in models the library state of ONE index: reset before building another)
        self.calls, self.attached, self.min_rows = [], False, 0

    def rf_index_storage_bytes(self, dim, capacity):
        return 64

    def rf_index_create(self, handle_ref, dim, capacity, storage, nbytes, device):
        return 0

    def rf_index_destroy(self, handle):
        return 0

    def rf_sq8_storage_bytes(self, dim, capacity):
        return 0 if dim % 32 else 64

    def rf_index_attach_sq8(self, handle, storage, nbytes, stream):
        self.calls.append("attach")
        self.attached = True
        return 0

    def rf_index_detach_sq8(self, handle):
        self.calls.append("detach")
        self.attached = False
        return 0

    def rf_index_set_shadow_first(self, handle, min_rows):
        self.calls.append(("shadow_first", min_rows))
        self.min_rows = min_rows
        return 0

    def rf_search_workspace_bytes(self, handle):   # as the library: the SQ8 size while shadow-first is on
        return self.SQ8 if self.attached and self.min_rows > 0 else self.FLAT

    def rf_search_sq8_workspace_bytes(self, handle):
        return self.SQ8

    def rf_search_grouped_workspace_bytes(self, handle):
        return self.GROUPED


@pytest.fixture
def fake_lib(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(rindex, "require_gpu", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(_lib, "load_library", lambda: lib)
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    return lib


def test_auto_follows_shadow_min_rows(fake_lib, monkeypatch):
    shipped = rindex.GpuIndex.SHADOW_MIN_ROWS
    if shipped is None:                                  # "auto" is off as shipped: never attaches
        ix = rindex.GpuIndex(384, 1 << 22)
        assert not ix.shadow_first and not ix.sq8 and fake_lib.calls == []
        monkeypatch.setattr(rindex.GpuIndex, "SHADOW_MIN_ROWS", 1 << 19)
    m = rindex.GpuIndex.SHADOW_MIN_ROWS
    assert m & (m - 1) == 0 and m > 100_000              # a power of two above the launch-bound 100 k rows
    ix = rindex.GpuIndex(384, m)
    assert ix.shadow_first and not ix.sq8                # .sq8 stays "the caller enabled SQ8"
    assert fake_lib.calls == ["attach", ("shadow_first", m)]
    assert ix.workspace_bytes == FakeLib.SQ8             # read after the switch: covers the query area
    assert ix.workspace.numel() >= FakeLib.GROUPED
    fake_lib.reset()
    assert not rindex.GpuIndex(384, m - 1).shadow_first and fake_lib.calls == []      # below the cut
    assert not rindex.GpuIndex(48, 2 * m).shadow_first and fake_lib.calls == []       # dim % 32 != 0


def test_true_forces_false_never(fake_lib):
    ix = rindex.GpuIndex(384, 100, shadow=True)
    assert ix.shadow_first and fake_lib.calls == ["attach", ("shadow_first", 1)]
    fake_lib.reset()
    ix = rindex.GpuIndex(384, 1 << 22, shadow=False)
    assert not ix.shadow_first and ix.workspace_bytes == FakeLib.FLAT and fake_lib.calls == []
    with pytest.raises(_lib.RagfinError):
        rindex.GpuIndex(48, 100, shadow=True)
    for bad in ("yes", 1, 0, None, 1.0):                 # 1 == True, but only a bool or "auto" is taken
        with pytest.raises(ValueError):
            rindex.GpuIndex(384, 100, shadow=bad)
    import numpy as np
    fake_lib.reset()
    assert rindex.GpuIndex(384, 100, shadow=np.bool_(True)).shadow_first


def test_enable_sq8_reuses_the_shadow_and_disable_keeps_it(fake_lib):
    ix = rindex.GpuIndex(384, 100, shadow=True)
    fake_lib.calls.clear()
    ix.enable_sq8()
    assert ix.sq8 and fake_lib.calls == []               # reused: no second attach
    ix.disable_sq8()
    assert not ix.sq8 and fake_lib.attached and fake_lib.calls == []
    with pytest.raises(_lib.RagfinError, match="SQ8 not enabled"):   # sq8=True needs enable_sq8
        ix.search_raw(torch.zeros((1, 384), dtype=torch.float16), 5, sq8=True)
    fake_lib.reset()
    plain = rindex.GpuIndex(384, 100, shadow=False)
    plain.enable_sq8()
    plain.disable_sq8()
    assert fake_lib.calls == ["attach", "detach"] and not plain.sq8


def test_ladder_predicate_mirrors_the_librarys_chain_choice(fake_lib, monkeypatch):
    """The fp16 tier is put behind a plain first pass only where rf_search took the shadow chain:
    switch set, size >= min_rows, size > RF_SMALL_ROWS, at most 64 queries (plain_chain in api.hip)."""
    monkeypatch.setattr(rindex.GpuIndex, "SHADOW_MIN_ROWS", 1 << 19)
    size = [0]
    fake_lib.rf_index_size = lambda handle: size[0]
    ix = rindex.GpuIndex(384, 1 << 20)
    for n, b, want in ((1 << 20, 64, True), (1 << 20, 65, False), ((1 << 19) - 1, 64, False), (1 << 19, 1, True)):
        size[0] = n
        assert ix._plain_chain_is_shadow(b) is want, (n, b)
    fake_lib.reset()
    forced = rindex.GpuIndex(384, 100_000, shadow=True)
    for n, want in ((8192, False), (8193, True)):
        size[0] = n
        assert forced._plain_chain_is_shadow(64) is want, n
    fake_lib.reset()
    assert not rindex.GpuIndex(384, 1 << 20, shadow=False)._plain_chain_is_shadow(64)
