"""GPU tests of the reader's sliding windows: rf_stitch_spans (csrc/reader_windows.hip) against
rag_fin_amd.reader.stitch_reference -- on the device's own window logits, on planted logits through ctypes, for
placement stability, against rf_answer_spans on one-window contexts, end to end through predict(doc_stride=...),
and its argument checks.  Seeded random weights, two layers, the span head of tests/test_reader_gpu.py.

Bounds of every device-against-reference comparison (check): spans, their order, the z bits and the z_null bits
are equal; each log-sum-exp is within 2^-24 |lse| + (L + 2) 2^-52 of the reference's fp64 value -- the kernel's one
rounding to fp32 plus the error of an fp64 sum of L + 1 terms."""
import ctypes

import numpy as np
import pytest

from rag_fin_amd.reader import plan_windows, stitch_reference
from test_reader_gpu import CFG2, HEAD_SCALE, TOL, build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model2(gpu_device):
    return build(CFG2, 5, gpu_device)[0]


# ---- layouts, the raw call, the comparison --------------------------------------------------------------------------
def layout(contexts, T, seg, doc_stride):
    """contexts: per context a token count (cut by plan_windows with the room T - seg - 1 of a pair row) or an
    explicit list of (first, count); [] = a context without windows.  -> (windows int32 [W, 3], ctx_win [C + 1])."""
    windows, ctx_win = [], [0]
    for c in contexts:
        plan = plan_windows(c, T - seg - 1, doc_stride) if isinstance(c, int) else c
        windows += [(f, n, seg) for f, n in plan]
        ctx_win.append(len(windows))
    return np.array(windows, dtype=np.int32).reshape(-1, 3), np.array(ctx_win, dtype=np.int32)


def window_ids(rng, windows, T, vocab=2000):
    """Pair rows for the windows: random ids (the decode sees logits alone, so overlapping windows need not hold
    the same tokens), lens = seg + count + 1 ([SEP] closes the row)."""
    lens = (windows[:, 2] + windows[:, 1] + 1).astype(np.int32)
    return rng.integers(1, vocab, (len(windows), T)).astype(np.int32), lens


def stitch_raw(device, logits, windows, ctx_win, max_answer_len, n_best):
    """rf_stitch_spans through ctypes on host arrays -> host (spans [C, n_best, 2], z [C, n_best], norm [C, 3])."""
    import torch
    from rag_fin_amd import _lib
    lib = _lib.load_library()
    W, T, C = logits.shape[0], logits.shape[1], len(ctx_win) - 1
    win = np.zeros((W, 4), dtype=np.int32)
    win[:, :3] = windows
    longest = int((windows[:, 0] + windows[:, 1]).max()) if W else 0
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (logits.astype(np.float32), win, ctx_win.astype(np.int32))]
    out = torch.empty(C * n_best * 3 + 3 * C, dtype=torch.int32, device=device)
    ws = torch.empty(lib.rf_stitch_workspace_bytes(W, C, longest), dtype=torch.uint8, device=device)
    p = ctypes.c_void_p
    with torch.cuda.device(device):
        _lib.check(lib.rf_stitch_spans(p(dev[0].data_ptr()), W, T, p(dev[1].data_ptr()), p(dev[2].data_ptr()), C,
                                       max_answer_len, n_best, p(out.data_ptr()), p(out.data_ptr() + 4 * C * n_best * 3),
                                       p(ws.data_ptr()), ws.numel(), _lib.current_stream_ptr()))
    host = out.cpu().numpy()
    rows = host[:C * n_best * 3].reshape(C, n_best, 3)
    return rows[:, :, :2].copy(), rows[:, :, 2].copy().view(np.float32), host[C * n_best * 3:].view(np.float32).reshape(C, 3).copy()


def check(got, logits, windows, ctx_win, max_answer_len, n_best, name=""):
    """Every context of a call against stitch_reference on the same logits, by the module docstring's bounds."""
    spans, z, norm = got
    C = len(ctx_win) - 1
    assert spans.shape == (C, n_best, 2) and z.shape == (C, n_best) and norm.shape == (C, 3)
    worst = 0.0
    for c in range(C):
        r = slice(int(ctx_win[c]), int(ctx_win[c + 1]))
        want, z_null, ls, le = stitch_reference(logits[r], windows[r], max_answer_len, n_best)
        L = int((windows[r, 0] + windows[r, 1]).max()) if r.stop > r.start else 0
        assert [tuple(p) for p in spans[c]] == [(i, j) for i, j, _ in want], (name, c, spans[c], want)
        assert np.array_equal(z[c].view(np.uint32), np.array([v for _, _, v in want], np.float32).view(np.uint32)), (name, c, z[c], want)
        assert norm[c, 0].view(np.uint32) == np.float32(z_null).view(np.uint32), (name, c, norm[c], z_null)
        for g, ref in ((norm[c, 1], ls), (norm[c, 2], le)):
            if np.isinf(ref):
                assert g == ref, (name, c, g, ref)
                continue
            d, bound = abs(float(g) - ref), 2.0 ** -24 * abs(ref) + (L + 2) * 2.0 ** -52
            worst = max(worst, d / bound)
            assert d <= bound, (name, c, float(g), ref, d, bound)
    print(f"stitch {name}: worst |lse - fp64| / bound = {worst:.3f}")


def forward(rd, rng, windows, T):
    """The windows' logits as the device's forward writes them -> (device tensor [W, T, 2], its host copy)."""
    ids, lens = window_ids(rng, windows, T)
    logits = rd.span_ids(ids, lens, windows[:, 2], 1, 1, want_logits=True).logits
    return logits, logits.cpu().numpy()


def host_of(batch):
    h = batch.cpu()
    return h.spans.numpy(), h.z.numpy(), h.norm.numpy()


# ---- on the device's own logits ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_windows(model2):
    """One context of 200 tokens at T = 96: seg 10, room 85, doc_stride 20 -> windows (0, 85), (65, 85), (130, 70)."""
    windows, ctx_win = layout([200], 96, 10, 20)
    assert windows[:, :2].tolist() == [[0, 85], [65, 85], [130, 70]]
    return (windows, ctx_win) + forward(model2, np.random.default_rng(96), windows, 96)


@pytest.mark.parametrize("max_answer_len,n_best", [(1, 1), (1, 16), (64, 1), (64, 16), (30, 5)])
def test_three_windows_equal_the_reference(model2, three_windows, max_answer_len, n_best):
    windows, ctx_win, dev, host = three_windows
    got = host_of(model2.stitch_logits(dev, windows, ctx_win, max_answer_len, n_best))
    check(got, host, windows, ctx_win, max_answer_len, n_best, f"3win_L{max_answer_len}_n{n_best}")
    assert (got[0][0, :, 0] >= 0).all() and (got[0][0, :, 1] < 200).all()


# contexts of 1, 2 and 7 windows, an empty one (L = 0: one window without tokens), one without windows (in the
# middle and at the end), one whose last window holds a single token, one of two tokens (3 candidates < n_best)
MIXED = [50, 120, [], 450, 0, [(0, 85), (85, 1)], 2, []]


def test_a_mixed_batch_equals_the_reference(model2):
    windows, ctx_win = layout(MIXED, 96, 10, 20)
    assert np.diff(ctx_win).tolist() == [1, 2, 0, 7, 1, 2, 1, 0]
    dev, host = forward(model2, np.random.default_rng(7), windows, 96)
    got = host_of(model2.stitch_logits(dev, windows, ctx_win, 30, 16))
    check(got, host, windows, ctx_win, 30, 16, "mixed")
    spans, z, norm = got
    for c in (2, 7):                                                        # no windows: nothing at all
        assert (spans[c] == -1).all() and (z[c] == -np.inf).all() and (norm[c] == -np.inf).all()
    assert (spans[4] == -1).all() and np.isfinite(norm[4]).all()            # L = 0: the null slot alone
    assert norm[4, 1] == host[ctx_win[4], 0, 0] and norm[4, 2] == host[ctx_win[4], 0, 1]
    assert (spans[6, :3] >= 0).all() and (spans[6, 3:] == -1).all()         # (0, 0), (0, 1), (1, 1) in some order


def test_stitch_ids_runs_the_windows_in_buckets_into_one_buffer(model2):
    """stitch_ids: the same windows through length-sorted buckets (batch_tokens = 500: several of them), the logits
    in one buffer in the windows' order, one decode -- against the reference on that buffer."""
    windows, ctx_win = layout(MIXED, 96, 10, 20)
    ids, lens = window_ids(np.random.default_rng(7), windows, 96)
    batch = model2.stitch_ids(ids, lens, windows, ctx_win, 30, 16, batch_tokens=500)
    assert batch.logits.data_ptr() == batch.packed.data_ptr() + 4 * 8 * 17 * 3     # views of ONE buffer
    logits = batch.logits.cpu().numpy()
    live = np.arange(96)[None, :] < lens[:, None]
    assert logits[live].all() and not logits[~live].any()                   # every row landed in its own place
    one, _ = forward(model2, np.random.default_rng(7), windows, 96)
    assert np.abs(one.cpu().numpy() - logits).max() < 2 * TOL               # (each within TOL of the mirror, whatever the bucket)
    check(host_of(batch), logits, windows, ctx_win, 30, 16, "stitch_ids")


def test_a_context_of_1100_tokens_crosses_tiles_and_seams(model2):
    """T = 64, room 50, doc_stride 40: 106 windows ten tokens apart, three selection tiles; 64-token spans are
    longer than a window and cross the tile edges at 512 and 1024."""
    windows, ctx_win = layout([1100], 64, 13, 40)
    assert len(windows) == 106
    dev, host = forward(model2, np.random.default_rng(1100), windows, 64)
    for max_answer_len, n_best in ((64, 16), (30, 16)):
        got = host_of(model2.stitch_logits(dev, windows, ctx_win, max_answer_len, n_best))
        check(got, host, windows, ctx_win, max_answer_len, n_best, f"L1100_{max_answer_len}")


def test_zero_head_ranks_by_start_then_end_across_seams_and_tiles(gpu_device):
    rd = build(dict(CFG2, layers=1), 4, gpu_device, zero_head=True)[0]
    windows, ctx_win = layout([600, 30], 64, 13, 40)
    dev, host = forward(rd, np.random.default_rng(3), windows, 64)
    assert not host.any()
    got = host_of(rd.stitch_logits(dev, windows, ctx_win, 3, 16))
    check(got, host, windows, ctx_win, 3, 16, "zero_head")
    want = [(i, j) for i in range(600) for j in range(i, min(i + 3, 600))][:16]
    assert [tuple(p) for p in got[0][0]] == want and [tuple(p) for p in got[0][1]] == want
    assert not got[1].view(np.uint32).any() and not got[2][:, 0].view(np.uint32).any()
    for c, L in ((0, 600), (1, 30)):                                        # log(null slot + L tokens)
        assert abs(float(got[2][c, 1]) - np.log(L + 1)) <= 2.0 ** -24 * np.log(L + 1) + (L + 2) * 2.0 ** -52


# ---- planted logits through ctypes, no forward ------------------------------------------------------------------------
PT, PSEG = 512, 1                                                           # pair rows of 512: room 510


def planted(rng, L, doc_stride=128, quantum=None):
    """Random logits for one context of L tokens in windows of 510 -> (logits, windows, ctx_win, plant).
    plant(t, s=None, e=None) sets S[t] / E[t] where the decode reads them: in the owner of t."""
    from rag_fin_amd.reader import window_owners
    windows, ctx_win = layout([L], PT, PSEG, doc_stride)
    logits = rng.standard_normal((len(windows), PT, 2)).astype(np.float32)
    if quantum:
        logits = (np.round(logits / quantum) * quantum).astype(np.float32)
    owner = window_owners(windows)

    def plant(t, s=None, e=None):
        w = owner[t]
        for k, v in ((0, s), (1, e)):
            if v is not None:
                logits[w, PSEG + t - windows[w, 0], k] = v
    return logits, windows, ctx_win, plant


def test_the_longest_context(gpu_device):
    """L = 65 536 = RF_READER_MAX_CONTEXT: 128 tiles; the best spans planted at the very end, where the keys
    (i << 6) | (j - i) are largest, and across the last tile edge."""
    logits, windows, ctx_win, plant = planted(np.random.default_rng(65536), 65536)
    plant(65535, s=9.0, e=9.0)                                              # (65535, 65535)
    plant(65472, s=8.5)                                                     # (65472, 65535): 64 tokens
    plant(65000, s=7.5)                                                     # tile 126 ...
    plant(65030, e=9.5)                                                     # ... into tile 127 (65024 is the edge)
    got = stitch_raw(gpu_device, logits, windows, ctx_win, 64, 16)
    check(got, logits, windows, ctx_win, 64, 16, "L65536")
    assert [tuple(p) for p in got[0][0, :3]] == [(65535, 65535), (65472, 65535), (65000, 65030)]


def test_equal_z_at_and_across_tile_edges(gpu_device):
    """Logits in steps of 1/4 (equal z everywhere) and the value 10 planted at starts and ends 511 / 512 / 1023 /
    1024 and around them: many spans of z = 20 exactly, ranked by (i, j) across two tile edges."""
    logits, windows, ctx_win, plant = planted(np.random.default_rng(5), 2000, quantum=0.25)
    for t in (500, 511, 512, 1000, 1023, 1024):
        plant(t, s=10.0)
    for t in (511, 512, 520, 1023, 1024, 1040):
        plant(t, e=10.0)
    for n_best in (16, 5):
        got = stitch_raw(gpu_device, logits, windows, ctx_win, 64, n_best)
        check(got, logits, windows, ctx_win, 64, n_best, f"ties_n{n_best}")
    assert (got[1] == 20.0).all() and tuple(got[0][0, 0]) == (500, 511) and tuple(got[0][0, 4]) == (511, 512)
    got = stitch_raw(gpu_device, logits, windows, ctx_win, 1, 16)           # single tokens: 4 of z = 20, then ties
    check(got, logits, windows, ctx_win, 1, 16, "ties_len1")
    assert [tuple(p) for p in got[0][0, :4]] == [(511, 511), (512, 512), (1023, 1023), (1024, 1024)]


def test_the_best_sixteen_in_one_tile_and_one_per_tile(gpu_device):
    logits, windows, ctx_win, plant = planted(np.random.default_rng(6), 2000)
    for k in range(20):                                                     # all in tile 2 (1024 .. 1535)
        plant(1100 + 3 * k, s=6.0 + 0.125 * k)
        plant(1101 + 3 * k, e=6.0)
    got = stitch_raw(gpu_device, logits, windows, ctx_win, 30, 16)
    check(got, logits, windows, ctx_win, 30, 16, "one_tile")
    assert (got[0][0] >= 1024).all() and (got[0][0] < 1536).all()
    logits, windows, ctx_win, plant = planted(np.random.default_rng(7), 16 * 512)
    for t in range(16):                                                     # one per tile; the rest stay below 16
        plant(512 * t + 100, s=10.0 + 0.25 * t)
        plant(512 * t + 105, e=10.0)
    got = stitch_raw(gpu_device, logits, windows, ctx_win, 30, 16)
    check(got, logits, windows, ctx_win, 30, 16, "one_per_tile")
    assert [tuple(p) for p in got[0][0]] == [(512 * t + 100, 512 * t + 105) for t in range(15, -1, -1)]


def test_minus_infinity_logits(gpu_device):
    """-inf among the logits: candidates of z = -inf rank last, by (i, j); a tile whose starts are all -inf; a
    context with five finite tokens; a null slot of -inf."""
    rng = np.random.default_rng(8)
    logits, windows, ctx_win, plant = planted(rng, 1300)
    for t in rng.choice(1300, 400, replace=False):
        plant(int(t), s=-np.inf)
    for t in rng.choice(1300, 400, replace=False):
        plant(int(t), e=-np.inf)
    for t in range(512, 1024):
        plant(t, s=-np.inf)
    got = stitch_raw(gpu_device, logits, windows, ctx_win, 64, 16)
    check(got, logits, windows, ctx_win, 64, 16, "inf_mixed")
    assert np.isfinite(got[1]).all() and ((got[0][0, :, 0] < 512) | (got[0][0, :, 0] >= 1024)).all()
    logits, windows, ctx_win, plant = planted(rng, 600)
    keep = {3: 1.0, 4: 2.0, 300: 0.5, 511: 1.5, 512: 1.25}
    for t in range(600):
        plant(t, s=keep.get(t, -np.inf), e=keep.get(t, -np.inf))
    logits[1, 0] = (-np.inf, 0.0)                                           # window 1 is the null slot: z_null = -inf
    got = stitch_raw(gpu_device, logits, windows, ctx_win, 2, 16)
    check(got, logits, windows, ctx_win, 2, 16, "inf_sparse")
    # finite: (3, 3), (3, 4), (4, 4), (300, 300), (511, 511), (511, 512), (512, 512); then z = -inf from (0, 0) on
    assert np.isfinite(got[1][0, :7]).all() and (got[1][0, 7:] == -np.inf).all() and tuple(got[0][0, 7]) == (0, 0)
    assert got[2][0, 0] == -np.inf


# ---- reproducibility --------------------------------------------------------------------------------------------------
def test_same_context_same_bits_alone_in_front_and_behind_others_and_across_calls(gpu_device):
    rng = np.random.default_rng(11)
    T, seg = 128, 9
    mine, _ = layout([1500], T, seg, 60)
    others, others_ctx = layout([40, 700, 0, 118, 2000, [], 300, 119], T, seg, 30)
    mine_logits = rng.standard_normal((len(mine), T, 2)).astype(np.float32)
    other_logits = rng.standard_normal((len(others), T, 2)).astype(np.float32)
    n_other = np.diff(others_ctx)

    def run(front):
        parts = [(mine, mine_logits), (others, other_logits)]
        counts = [len(mine)] + n_other.tolist()
        if not front:
            parts, counts = parts[::-1], n_other.tolist() + [len(mine)]
        windows, logits = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        ctx_win = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        got = stitch_raw(gpu_device, logits, windows, ctx_win, 64, 16)
        c = 0 if front else 8
        return got[0][c], got[1][c].view(np.uint32), got[2][c].view(np.uint32)

    alone = stitch_raw(gpu_device, mine_logits, mine, np.array([0, len(mine)], np.int32), 64, 16)
    check(alone, mine_logits, mine, np.array([0, len(mine)], np.int32), 64, 16, "alone")
    alone = (alone[0][0], alone[1][0].view(np.uint32), alone[2][0].view(np.uint32))
    for other in (run(True), run(False), run(False)):
        assert all(np.array_equal(a, b) for a, b in zip(alone, other))


# ---- one-window contexts: the decode rf_answer_spans performs -----------------------------------------------------------
def test_one_window_contexts_equal_rf_answer_spans(model2):
    """Rows that fit their window, each a context of one window: the same spans (shifted by seg), z bits and
    z_null bits as k_qa_spans decodes from the same logits in the same call."""
    lens = np.array([96, 40, 41, 30, 77, 50, 12], dtype=np.int32)
    seg = np.array([12, 38, 38, 29, 33, 1, 9], dtype=np.int32)              # contexts of 83, 1, 2, 0, 43, 48, 2 tokens
    ids = np.random.default_rng(96).integers(1, 2000, (7, 96)).astype(np.int32)
    for max_answer_len, n_best in ((30, 16), (64, 5), (1, 1)):
        pair = model2.span_ids(ids, lens, seg, max_answer_len, n_best, want_logits=True)
        windows = np.stack([np.zeros(7, np.int32), lens - seg - 1, seg], axis=1)
        ours = host_of(model2.stitch_logits(pair.logits, windows, np.arange(8, dtype=np.int32), max_answer_len, n_best))
        theirs = pair.cpu()
        spans, z, norm = theirs.spans.numpy(), theirs.z.numpy(), theirs.norm.numpy()
        shift = np.where(spans >= 0, seg[:, None, None], 0)
        assert np.array_equal(ours[0], spans - shift)
        assert np.array_equal(ours[1].view(np.uint32), z.view(np.uint32))
        assert np.array_equal(ours[2][:, 0].view(np.uint32), norm[:, 0].view(np.uint32))
        # the normalisers: the same set of terms ([CLS] + context), each side rounded to fp32 once
        assert (np.abs(ours[2][:, 1:].astype(np.float64) - norm[:, 1:]) <= 2 * 2.0 ** -24 * np.abs(norm[:, 1:]) + 1e-12).all()
        check(ours, pair.logits.cpu().numpy(), windows, np.arange(8, dtype=np.int32), max_answer_len, n_best, "one_window")


# ---- end to end ---------------------------------------------------------------------------------------------------------
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(200)] + list("abcdefghij") + [".", ","]


@pytest.fixture(scope="module")
def text_reader(gpu_device):
    from oracle import encoder as oenc
    from rag_fin_amd.reader import ExtractiveReader
    from rag_fin_amd.tokenizer import WordPieceTokenizer
    cfg = dict(oenc.MINILM_L6, layers=2, vocab_size=len(VOCAB), max_position=64)
    return ExtractiveReader.from_random(cfg, 6, tokenizer=WordPieceTokenizer(VOCAB), device=gpu_device,
                                        head_scale=HEAD_SCALE, max_length=64)


def text(rng, n_words):
    return "  " + " ".join(f"W{rng.integers(0, 200)}" + rng.choice(["", ".", ",", "  "]) for _ in range(n_words))


def tokenised_windows(rd, question, contexts, doc_stride):
    """The test's own pair rows: (ids, lens, windows, ctx_win, per-context token offsets)."""
    tok = rd.tokenizer
    q = tok.encode(question, 66)[1:-1]
    seg, room = len(q) + 2, rd.max_length - len(q) - 3
    rows, windows, ctx_win, offsets = [], [], [0], []
    for c in contexts:
        cid, off = tok.encode_with_offsets(c, 100000)
        cid, off = cid[1:-1], off[1:-1]
        for f, n in plan_windows(len(cid), room, doc_stride):
            rows.append([tok.cls_id] + q + [tok.sep_id] + cid[f:f + n] + [tok.sep_id])
            windows.append((f, n, seg))
        ctx_win.append(len(rows))
        offsets.append(off)
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    ids = np.full((len(rows), int(lens.max())), tok.pad_id, dtype=np.int32)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
    return ids, lens, np.array(windows, dtype=np.int32), np.array(ctx_win, dtype=np.int32), offsets


QUESTION = "w3 w77 w150 w9 w21"


def test_long_contexts_are_read_to_their_end(text_reader):
    rd = text_reader
    rng = np.random.default_rng(1)
    contexts = [text(rng, 24), text(rng, 110), text(rng, 300)]
    ids, lens, windows, ctx_win, offsets = tokenised_windows(rd, QUESTION, contexts, 16)
    assert [len(o) for o in offsets][0] < 57 < [len(o) for o in offsets][1] < 250 < [len(o) for o in offsets][2] < 600
    assert np.diff(ctx_win)[0] == 1 and np.diff(ctx_win)[2] > 6
    # the expectation, on the CPU: stitch_reference on the window logits + the token offsets
    logits = rd.span_ids(ids, lens, windows[:, 2], 1, 1, want_logits=True).logits.cpu().numpy()
    want, nulls, max_lse = [], [], 0.0
    for c in range(3):
        r = slice(ctx_win[c], ctx_win[c + 1])
        spans, z_null, ls, le = stitch_reference(logits[r], windows[r], 30, 16)
        max_lse = max(max_lse, abs(ls), abs(le))
        seen = set()
        for i, j, z in spans:
            key = (c, offsets[c][i][0], offsets[c][j][1])
            if key not in seen:
                seen.add(key)
                want.append((float(z) - ls - le,) + key)
        nulls.append((float(z_null) - ls - le, c, 0, 0))
    want.sort(key=lambda h: (-np.exp(h[0]), h[1], h[2], h[3]))
    first_window_end = offsets[2][windows[ctx_win[2], 1] - 1][1]            # last character the first window holds
    assert any(c == 2 and end > first_window_end for _, c, _, end in want)  # (the CPU side's own condition)
    assert 40 <= len(want) <= 48

    got = rd.predict(QUESTION, contexts, top_k=500, doc_stride=16)          # everything the three contexts give
    assert got == rd.predict(QUESTION, contexts, top_k=500, doc_stride=16)  # bit-identical across calls
    assert all(h["answer"] == contexts[h["context_index"]][h["start"]:h["end"]] and h["answer"] for h in got)
    keys = [(h["context_index"], h["start"], h["end"]) for h in got]
    assert len(set(keys)) == len(keys)
    assert [(-h["score"],) + k for h, k in zip(got, keys)] == sorted((-h["score"],) + k for h, k in zip(got, keys))
    assert keys == [h[1:] for h in want]
    assert got[:7] == rd.predict(QUESTION, contexts, top_k=7, doc_stride=16)
    # two normalisers, each within 2^-24 |lse| + (L + 2) 2^-52 of the reference's (L < 600)
    tol = 2 * (2.0 ** -24 * max_lse + 602 * 2.0 ** -52)
    assert all(abs(np.log(h["score"]) - w[0]) <= tol for h, w in zip(got, want))
    assert any(h["context_index"] == 2 and h["end"] > first_window_end for h in got)
    # cut mode never sees past the first window
    cut = rd.predict(QUESTION, contexts, top_k=500)
    assert cut and not any(h["context_index"] == 2 and h["end"] > first_window_end for h in cut)
    assert cut == rd.predict(QUESTION, contexts, top_k=500, doc_stride=None)
    # the instance's stride is the default of predict
    rd.doc_stride = 16
    try:
        assert rd.predict(QUESTION, contexts, top_k=500) == got
    finally:
        rd.doc_stride = None
    # the null candidate: exactly one more entry per context, the span scores untouched
    both = rd.predict(QUESTION, contexts, top_k=500, handle_impossible_answer=True, doc_stride=16)
    null_hits = [h for h in both if h["answer"] == "" and h["start"] == h["end"] == 0]
    assert sorted(h["context_index"] for h in null_hits) == [0, 1, 2]
    assert [h for h in both if h["answer"]] == got
    for h in null_hits:
        assert abs(np.log(h["score"]) - nulls[h["context_index"]][0]) <= tol


def test_contexts_that_fit_give_the_cut_modes_answers(text_reader):
    """One window per context: the same answers in the same order; ln score within 4 (2^-24 max |lse| + 1e-12) --
    two normalisers, each rounded once on either side."""
    rd = text_reader
    rng = np.random.default_rng(2)
    contexts = [text(rng, n) for n in (5, 18, 1, 25, 11)]
    ids, lens, windows, ctx_win, _ = tokenised_windows(rd, QUESTION, contexts, 16)
    assert (np.diff(ctx_win) == 1).all()                                    # they all fit
    norm = rd.stitch_ids(ids, lens, windows, ctx_win, 30, 16).cpu().norm.numpy()
    tol = 4 * (2.0 ** -24 * float(np.abs(norm[:, 1:]).max()) + 1e-12)
    for kw in (dict(top_k=1), dict(top_k=12), dict(top_k=100, handle_impossible_answer=True)):
        a, b = rd.predict(QUESTION, contexts, doc_stride=16, **kw), rd.predict(QUESTION, contexts, **kw)
        assert len(a) == len(b) > 0
        for x, y in zip(a, b):
            assert {k: x[k] for k in ("answer", "start", "end", "context_index")} == {k: y[k] for k in ("answer", "start", "end", "context_index")}
            assert abs(np.log(x["score"]) - np.log(y["score"])) <= tol, (x, y, tol)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_launched(gpu_device):
    import torch
    from rag_fin_amd import _lib
    lib = _lib.load_library()
    windows, ctx_win = layout([100, 30], 64, 13, 40)
    W = len(windows)
    win = np.zeros((W, 4), np.int32)
    win[:, :3] = windows
    logits, win_d, ctx_d = (torch.from_numpy(a).to(gpu_device) for a in (np.zeros((W, 64, 2), np.float32), win, ctx_win))
    out = torch.full((2 * 16 * 3 + 6,), 12345, dtype=torch.int32, device=gpu_device)
    need = lib.rf_stitch_workspace_bytes(W, 2, 100)
    assert need > 0 and lib.rf_stitch_workspace_bytes(W, 0, 100) == 0 and lib.rf_stitch_workspace_bytes(-1, 2, 100) == 0
    assert lib.rf_stitch_workspace_bytes(W, 2, _lib.RF_READER_MAX_CONTEXT) == need
    assert lib.rf_stitch_workspace_bytes(W, 2, _lib.RF_READER_MAX_CONTEXT + 1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    p = ctypes.c_void_p
    good = dict(logits=logits.data_ptr(), W=W, T=64, win=win_d.data_ptr(), ctx=ctx_d.data_ptr(), C=2, mal=30, nb=16,
                spans=out.data_ptr(), norm=out.data_ptr() + 4 * 96, ws=ws.data_ptr(), nws=need)

    def call(**kw):
        a = {**good, **kw}
        with torch.cuda.device(gpu_device):
            rc = lib.rf_stitch_spans(p(a["logits"]), a["W"], a["T"], p(a["win"]), p(a["ctx"]), a["C"], a["mal"], a["nb"],
                                     p(a["spans"]), p(a["norm"]), p(a["ws"]), a["nws"], _lib.current_stream_ptr())
        torch.cuda.synchronize()
        return rc

    for kw in (dict(nb=0), dict(nb=17), dict(mal=0), dict(mal=65), dict(C=0), dict(W=-1), dict(T=0), dict(logits=None),
               dict(win=None), dict(ctx=None), dict(spans=None), dict(norm=None), dict(ws=None)):
        assert call(**kw) == -1, kw                                       # RF_ERR_INVALID
    assert call(T=513) == -2 and "512" in lib.rf_last_error().decode()
    assert call(nws=need - 1) == -3 and call(nws=0) == -3                   # RF_ERR_CAPACITY
    assert (out.cpu().numpy() == 12345).all()                               # a refused call writes nothing
    assert call() == 0 and not (out.cpu().numpy() == 12345).any()           # (and the good call writes every slot)


def test_a_context_beyond_the_limit_is_refused_on_the_host(text_reader):
    from rag_fin_amd import _lib
    assert _lib.RF_READER_MAX_CONTEXT == 65536
    with pytest.raises(ValueError, match="RF_READER_MAX_CONTEXT"):
        text_reader.predict(QUESTION, ["w1 " * (_lib.RF_READER_MAX_CONTEXT + 1)], doc_stride=16)
    with pytest.raises(ValueError):                                         # a stride that leaves no step
        text_reader.predict(QUESTION, ["w1 w2"], doc_stride=60)
