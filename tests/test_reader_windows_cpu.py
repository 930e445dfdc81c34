"""CPU tests of the reader's sliding windows: the window layout (plan_windows) and the numpy definition of the
stitched decode (window_owners, stitch_reference) that tests/test_reader_windows_gpu.py holds rf_stitch_spans to."""
import numpy as np
import pytest

from rag_fin_amd.reader import plan_windows, span_reference, stitch_reference, window_owners


# ---- plan_windows ---------------------------------------------------------------------------------------------------
def test_layouts_worked_by_hand():
    assert plan_windows(10, 4, 2) == [(0, 4), (2, 4), (4, 4), (6, 4)]       # step 2; 6 + 4 reaches 10
    assert plan_windows(10, 4, 0) == [(0, 4), (4, 4), (8, 2)]               # no overlap
    assert plan_windows(9, 4, 1) == [(0, 4), (3, 4), (6, 3)]
    assert plan_windows(5, 4, 3) == [(0, 4), (1, 4)]                        # step 1
    assert plan_windows(11, 4, 2) == [(0, 4), (2, 4), (4, 4), (6, 4), (8, 3)]
    assert plan_windows(4, 4, 2) == [(0, 4)] and plan_windows(3, 4, 0) == [(0, 3)] and plan_windows(0, 4, 3) == [(0, 0)]


@pytest.mark.parametrize("room,doc_stride", [(1, 0), (4, 0), (4, 3), (7, 2), (50, 40), (381, 128)])
def test_windows_cover_the_context_and_ascend(room, doc_stride):
    for L in list(range(0, 3 * room + 3)) + [10 * room + 1, 1100]:
        plan = plan_windows(L, room, doc_stride)
        first = [f for f, _ in plan]
        end = [f + n for f, n in plan]
        if L <= room:
            assert plan == [(0, L)]
            continue
        assert first[0] == 0 and end[-1] == L
        assert all(a < b for a, b in zip(first, first[1:])) and all(a < b for a, b in zip(end, end[1:]))
        assert all(n == room for _, n in plan[:-1]) and 1 <= plan[-1][1] <= room
        assert all(b - a == room - doc_stride for a, b in zip(first, first[1:]))
        assert all(e >= f for e, f in zip(end, first[1:]))                  # no gap: [0, L) is covered
        assert all(e < L for e in end[:-1])                                 # it stops at the FIRST window that reaches L


@pytest.mark.parametrize("room,doc_stride", [(4, -1), (4, 4), (4, 5), (1, 1), (0, 0)])
def test_a_stride_outside_the_room_is_refused(room, doc_stride):
    with pytest.raises(ValueError):
        plan_windows(10, room, doc_stride)


# ---- the owner rule ------------------------------------------------------------------------------------------------
def test_owner_is_the_window_with_the_most_context_and_ties_go_to_the_lower_window():
    # by hand, L = 10, windows of 4 every 2: token 2 has margin 1 in window 0 (2 left, 1 right) and 0 in window 1
    assert window_owners(plan_windows(10, 4, 2)).tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 3]
    # token 2: margin 1 in window 0 (min(2, 1)) and 1 in window 1 (min(1, 2)): the tie stays with window 0
    assert window_owners([(0, 4), (1, 4)]).tolist() == [0, 0, 0, 1, 1]
    # tokens 3 and 5 tie (margin 1 on either side of a seam) and stay with the lower window; token 4 is the
    # middle of window 1 (margin 2)
    assert window_owners([(0, 5), (2, 5), (4, 5)]).tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 2]
    assert window_owners([(0, 3)]).tolist() == [0, 0, 0] and window_owners([(0, 0)]).tolist() == []
    assert window_owners([(0, 2), (3, 2)]).tolist() == [0, 0, -1, 1, 1]     # (a gap: no owner)


# ---- stitch_reference ----------------------------------------------------------------------------------------------
def rows(plan, seg):
    return [(f, n, seg) for f, n in plan]


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("max_answer_len,n_best", [(1, 1), (30, 16), (64, 5), (3, 16)])
def test_one_window_is_span_reference_shifted_by_seg(max_answer_len, n_best):
    rng = np.random.default_rng(max_answer_len * 100 + n_best)
    for seg, count in ((5, 20), (1, 1), (9, 2), (4, 0), (0, 7)):
        T = seg + count + 1                                                 # [CLS] question [SEP] context [SEP]
        logits = (rng.standard_normal((1, T + 3, 2)) * 2).round(1).astype(np.float32)   # (rounded: equal z occur)
        got, z_null, ls, le = stitch_reference(logits, [(0, count, seg)], max_answer_len, n_best)
        want, w_null, ws, we = span_reference(logits[0, :, 0], logits[0, :, 1], seg, T, max_answer_len, n_best)
        if seg == 0:
            # ([CLS] inside the context: span_reference counts position 0 once, the stitched decode has the null
            # slot beside the context's tokens -- the spans agree, the normalisers need not)
            ws = we = None
        assert [(i, j) for i, j, _ in got] == [(i - seg, j - seg) if i >= 0 else (i, j) for i, j, _ in want]
        assert np.array_equal(bits([z for _, _, z in got]), bits([z for _, _, z in want]))
        assert bits(z_null) == bits(w_null)
        if ws is not None:
            assert abs(ls - ws) <= 1e-12 * max(1, abs(ws)) and abs(le - we) <= 1e-12 * max(1, abs(we))


def triple_loop(logits, windows, max_answer_len, n_best):
    """The definition again, token by token and candidate by candidate."""
    L = max(f + n for f, n, _ in windows)
    S, E = [], []
    for t in range(L):
        best, own = -1, None
        for w, (f, n, g) in enumerate(windows):
            if f <= t < f + n and min(t - f, f + n - 1 - t) > best:
                best, own = min(t - f, f + n - 1 - t), w
        f, n, g = windows[own]
        S.append(logits[own, g + t - f, 0])
        E.append(logits[own, g + t - f, 1])
    cand = []
    for i in range(L):
        for j in range(i, L):
            if j - i + 1 <= max_answer_len:
                cand.append((np.float32(S[i] + E[j]), i, j))
    cand.sort(key=lambda c: (-float(c[0]), c[1], c[2]))
    spans = [(i, j, z) for z, i, j in cand[:n_best]] + [(-1, -1, np.float32(-np.inf))] * max(0, n_best - len(cand))
    z0 = [np.float32(logits[w, 0, 0] + logits[w, 0, 1]) for w in range(len(windows))]
    null = min(range(len(windows)), key=lambda w: (float(z0[w]), w))

    def lse(v):
        v = np.array(v, dtype=np.float64)
        return float(v.max() + np.log(np.exp(v - v.max()).sum()))
    return spans, z0[null], lse([logits[null, 0, 0]] + S), lse([logits[null, 0, 1]] + E)


@pytest.mark.parametrize("L,room,doc_stride,max_answer_len,n_best", [
    (40, 12, 4, 30, 16), (37, 9, 8, 64, 16), (23, 10, 0, 5, 7), (5, 8, 3, 30, 16), (1, 4, 1, 1, 1), (31, 6, 3, 1, 16)])
def test_it_agrees_with_a_plain_triple_loop(L, room, doc_stride, max_answer_len, n_best):
    rng = np.random.default_rng(L)
    seg = 3
    windows = rows(plan_windows(L, room, doc_stride), seg)
    for scale in (2.0, 0.3):                                                # 0.3 rounded to 0.5: many equal z
        logits = (rng.standard_normal((len(windows), seg + room + 1, 2)) * scale * 2).round() / 2
        logits = logits.astype(np.float32)
        got, want = stitch_reference(logits, windows, max_answer_len, n_best), triple_loop(logits, windows, max_answer_len, n_best)
        assert [(i, j) for i, j, _ in got[0]] == [(i, j) for i, j, _ in want[0]]
        assert np.array_equal(bits([z for _, _, z in got[0]]), bits([z for _, _, z in want[0]]))
        assert bits(got[1]) == bits(want[1])
        assert abs(got[2] - want[2]) <= 1e-12 and abs(got[3] - want[3]) <= 1e-12


def test_all_zero_logits_rank_by_start_then_end():
    windows = rows(plan_windows(20, 8, 4), 2)
    got, z_null, ls, le = stitch_reference(np.zeros((len(windows), 11, 2), np.float32), windows, 3, 16)
    assert [(i, j) for i, j, _ in got] == [(i, j) for i in range(20) for j in range(i, min(i + 3, 20))][:16]
    assert all(bits(z) == 0 for _, _, z in got) and bits(z_null) == 0
    assert abs(ls - np.log(21)) < 1e-12 and abs(le - np.log(21)) < 1e-12     # the null slot + 20 tokens


def test_the_service_reads_the_stride_beside_the_model_directory(monkeypatch):
    from rag_fin_amd import service
    monkeypatch.setattr(service, "build_rag", lambda *a, **kw: kw)
    monkeypatch.setenv("RAGFIN_MODEL_DIR", "/nowhere")
    monkeypatch.setenv("READER_MODEL_DIR", "/nowhere/reader")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("READER_DOC_STRIDE", raising=False)
    assert service.build_rag_from_env()["reader_doc_stride"] is None        # unset: cut
    monkeypatch.setenv("READER_DOC_STRIDE", "128")
    kw = service.build_rag_from_env()
    assert kw["reader_doc_stride"] == 128 and kw["reader_dir"] == "/nowhere/reader"


def test_empty_contexts():
    logits = np.ones((2, 6, 2), np.float32)
    logits[1, 0] = (-1.0, 0.5)                                              # the smaller s[0] + e[0]: the null slot
    got, z_null, ls, le = stitch_reference(logits, [(0, 0, 3), (0, 0, 3)], 30, 4)   # L == 0: the null slot alone
    assert got == [(-1, -1, np.float32(-np.inf))] * 4 and z_null == np.float32(-0.5) and (ls, le) == (-1.0, 0.5)
    got, z_null, ls, le = stitch_reference(np.zeros((0, 6, 2), np.float32), [], 30, 2)   # no windows
    assert got == [(-1, -1, np.float32(-np.inf))] * 2 and z_null == -np.inf and ls == le == -np.inf
