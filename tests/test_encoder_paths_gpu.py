"""GPU tests of the one BERT forward behind seven entry points (encode_enqueue, csrc/encoder.hip) where the slot
count B * T, which picks the kernels, and the packed count M = sum(lens), which every kernel reads from device
memory, diverge: M at and next to the 64 / 128 / 256-token tile edges of the direct, DMA and wide paths, a single
live workgroup, M = 0, empty rows between live ones (a); both sides of every slot threshold (b); whatever the
workspace holds beyond M (c); and every head on the direct and the wide path and on a nearly empty stream (d).
The batches are tests/encoder_path_cases.py's; tests/test_encoder_path_cases_cpu.py proves their path classes.

No tolerance is new: every comparison with an oracle uses the constant of the existing test module of that entry
point, imported from it (each is 3 x a maximum measured on the MI355X); the achieved errors of this file are in
profiles/encoder_paths_measurements.jsonl.  The other assertions are bit identities, which need none: a row's output
does not depend on its neighbours, on the path's tile width (dma | dma_wide) or on what the workspace held."""
import ctypes
import functools

import numpy as np
import pytest

import encoder_path_cases as epc
from oracle import encoder as oenc
from test_encoder_gpu import TOL, TOL_COS, TOL_L2

# (the shared batches are read-only arrays; torch warns when it wraps one, and nothing here writes through it)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def emb(gpu_device):
    from rag_fin_amd.embedder import Embedder
    return Embedder(epc.weights()[0], epc.CFG, device=gpu_device)


def encode32(emb, ids, lens):
    return emb.encode_ids(ids, lens, out_dtype="float32").cpu().numpy()


def oracle_errors(got, want):
    """(max-abs, largest per-row L2, largest 1 - cos) of fp32 rows against the float64 oracle's."""
    got = got.astype(np.float64)
    cos = (got * want).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(want, axis=1)
    return float(np.abs(got - want).max()), float(np.linalg.norm(got - want, axis=1).max()), float(1 - cos.min())


def assert_within_encoder_bounds(got, want, name):
    from conftest import record_measurement
    e, l2, cos = oracle_errors(got, want)
    record_measurement(f"encoder_paths_{name}", max_abs_f32=e, l2_max=l2, one_minus_cos=cos, rows=len(want))
    print(f"encoder_paths_{name}: max_abs {e:.3e} (TOL {TOL}), l2 {l2:.3e} (TOL_L2 {TOL_L2}), 1 - cos {cos:.3e} (TOL_COS {TOL_COS})")
    assert e < TOL, e
    assert l2 < TOL_L2, l2
    assert cos < TOL_COS, cos
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-6      # fp32 rounding of a unit vector


# ---- a. packed-count edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", epc.EDGE_CASES, ids=epc.edge_id)
def test_packed_count_edges_match_the_oracle_and_their_dense_twin(emb, case):
    """M live tokens in a batch whose slots select the path: empty rows give exact zeros, live rows the oracle's
    vectors, and the same live rows between non-empty neighbours (the same ids, the empty rows given random positive
    lengths: same shape, same kernels) give the same bits -- tests/test_encoder_gpu.py::
    test_a_sequence_gives_the_same_bits_wherever_it_sits states why nothing may depend on a row's neighbours."""
    ids, lens, dense = epc.edge_batch(*case)
    live, want = epc.edge_oracle(*case)
    got = encode32(emb, ids, lens)
    assert got.shape == (len(lens), 384) and np.isfinite(got).all()
    assert not got[lens == 0].any()
    if len(live):
        assert_within_encoder_bounds(got[live], want, epc.edge_id(case))
    twin = encode32(emb, ids, dense)
    assert np.isfinite(twin).all()
    assert same_bits(got[live], twin[live])


# ---- b. slot boundaries -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boundary_out(emb):
    """name -> the fp32 output of a boundary batch, computed once."""
    return functools.lru_cache(maxsize=None)(lambda name: encode32(emb, *epc.boundary_batch(name)[:2]))


@pytest.mark.parametrize("name", [c[0] for c in epc.BOUNDARY_CASES])
def test_both_sides_of_every_slot_threshold_match_the_oracle(boundary_out, name):
    """1024 | 1025, 8191 | 8192 and 49 151 | 49 152 token slots.  The two T = 1 batches also put 8 191 / 8 192 rows
    through the one-workgroup scan of k_tok_offsets, with a dozen empty rows among them."""
    ids, lens, probes, _ = epc.boundary_batch(name)
    got = boundary_out(name)
    assert got.shape == (len(lens), 384) and np.isfinite(got).all()
    assert np.abs(np.linalg.norm(got[lens > 0], axis=1) - 1).max() < 1e-6
    assert not got[lens == 0].any()
    assert_within_encoder_bounds(got[probes], epc.oracle_rows(ids, lens, probes), f"boundary_{name}")


@pytest.mark.parametrize("below,above,first_slot", epc.BOUNDARY_PAIRS[1:])
def test_shared_sequences_agree_across_the_dma_thresholds(boundary_out, below, above, first_slot):
    """Sixteen sequences sit at the same rows of both batches of a pair.  direct | dma: other kernels, agreement
    within 2 x TOL as tests/test_encoder_gpu.py::test_all_gemm_paths_agree_and_match_the_oracle asserts it;
    dma | dma_wide: the same arithmetic per (token, feature), bit-identical, as that test establishes."""
    from conftest import record_measurement
    ids, lens, _, shared = epc.boundary_batch(below)
    lo, hi = boundary_out(below)[shared], boundary_out(above)[shared]
    want = epc.oracle_rows(ids, lens, shared)
    assert_within_encoder_bounds(lo, want, f"shared_{below}")
    assert_within_encoder_bounds(hi, want, f"shared_{above}")
    diff = float(np.abs(lo - hi).max())
    record_measurement(f"encoder_paths_shared_{below}_vs_{above}", max_abs_diff=diff)
    if first_slot == epc.WIDE_SLOTS:
        assert same_bits(lo, hi)
    else:
        assert diff < 2 * TOL, diff


# ---- c. workspace contents --------------------------------------------------------------------------------------------
FILLS = (0x00, 0xFF, 0x7B)       # zeros; every fp16 a NaN and every int32 -1; every fp16 61 280


def test_the_fill_bytes_are_what_they_are_there_for():
    assert np.isnan(np.array([0xFFFF], np.uint16).view(np.float16)[0]) and np.array([0xFFFFFFFF], np.uint32).view(np.int32)[0] == -1
    assert float(np.array([0x7B7B], np.uint16).view(np.float16)[0]) == 61280.0


@pytest.mark.parametrize("case", epc.WORKSPACE_CASES, ids=epc.edge_id)
def test_encode_does_not_depend_on_workspace_contents(emb, gpu_device, case):
    """The large-batch kernels load whole tiles before they look at M and multiply, in the last partial tile, whatever
    the workspace holds beyond it ("buffers are padded to whole tiles").  A caller-owned workspace of exactly
    rf_encode_workspace_bytes is filled with each byte pattern before a call: the fp16 and the fp32 output must not
    change by a bit, and must be those of encode_ids (a workspace from the caching allocator).  Only memory the
    library itself declares its own is ever read."""
    import torch
    _, B, T, M = case
    ids, lens, _ = epc.edge_batch(*case)
    want16 = emb.encode_ids(ids, lens).cpu().numpy()
    want32 = encode32(emb, ids, lens)
    ids_d = torch.as_tensor(ids).to(gpu_device).contiguous()
    lens_d = torch.as_tensor(lens).to(gpu_device).contiguous()
    ws = torch.empty(emb.lib.rf_encode_workspace_bytes(emb.handle, B, T), dtype=torch.uint8, device=gpu_device)
    for fill in FILLS:
        ws.fill_(fill)
        out16 = torch.full((B, 384), float("nan"), dtype=torch.float16, device=gpu_device)
        out32 = torch.full((B, 384), float("nan"), dtype=torch.float32, device=gpu_device)
        emb._launch(ids_d, lens_d, B, T, out16, out32, ws=ws)
        got16, got32 = out16.cpu().numpy(), out32.cpu().numpy()
        assert np.isfinite(got32).all() and np.isfinite(got16).all(), hex(fill)
        assert same_bits(got32, want32), hex(fill)
        assert same_bits(got16, want16), hex(fill)
    assert int(lens.sum()) == M and np.abs(want32[lens > 0]).max() > 0.01


# ---- d. the heads -----------------------------------------------------------------------------------------------------
# Every head is wrapped to one form: run(ids, lens, seg) -> (rows, extras): rows[b] is row b's numeric output, the
# array the head's fp64 mirror defines (compared by the head's own constant); extras are further per-row outputs of
# the call that are compared by bits only.  mirror(ids, lens, seg) -> the same list in float64.  check_empty(rows,
# extras, b) asserts what the head documents for a row of no tokens.  Every head admits zero-length rows.
class CrossEncoderHead:
    """rf_score_pairs: one logit per pair; a pair of no tokens scores -inf."""
    pair = True

    def __init__(self, device):
        from test_rerank_gpu import CFG2, TOL as tol, build
        self.cfg, self.tol = CFG2, tol
        self.model, self.w16, self.head16 = build(CFG2, 5, device)

    def run(self, ids, lens, seg):
        got = self.model.score_ids(ids, lens, seg).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (len(lens),)
        return [got[b:b + 1] for b in range(len(lens))], {}

    def mirror(self, ids, lens, seg):
        from test_rerank_cpu import mirror_logits
        want = mirror_logits(self.w16, self.head16, self.cfg, ids, lens, seg)[:, 0]
        return [want[b:b + 1] for b in range(len(lens))]

    def check_empty(self, rows, extras, b):
        assert rows[b][0] == -np.inf


class ReaderHead:
    """rf_answer_spans: start / end logits at the positions < len; the best 16 spans, their scores and the three
    normalisers ride along and are compared by bits.  A pair of no tokens has no span and no [CLS] slot."""
    pair = True

    def __init__(self, device):
        from test_reader_gpu import CFG2, TOL as tol, build
        self.cfg, self.tol = CFG2, tol
        self.model, self.w16, self.head16 = build(CFG2, 5, device)

    def run(self, ids, lens, seg):
        host = self.model.span_ids(ids, lens, seg, 30, 16, want_logits=True).cpu()
        logits = host.logits.numpy()
        assert logits.dtype == np.float32 and logits.shape == ids.shape + (2,)
        live = np.arange(ids.shape[1])[None, :] < np.asarray(lens)[:, None]
        assert not logits[~live].any()                              # positions >= len are not written
        return ([logits[b, :lens[b]] for b in range(len(lens))],
                {"spans": host.spans.numpy(), "z": host.z.numpy(), "norm": host.norm.numpy()})

    def mirror(self, ids, lens, seg):
        from test_reader_cpu import mirror_qa_logits
        want = mirror_qa_logits(self.w16, self.head16, self.cfg, ids, lens, seg)
        return [want[b, :lens[b]] for b in range(len(lens))]

    def check_empty(self, rows, extras, b):
        assert rows[b].shape[0] == 0
        assert (extras["spans"][b] == -1).all() and (extras["z"][b] == -np.inf).all() and extras["norm"][b, 0] == -np.inf


class SpladeHead:
    """rf_encode_terms: the dense term weights [V]; a row of no tokens has no terms (all zeros)."""
    pair = False

    def __init__(self, device):
        from rag_fin_amd.sparse_encoder import SparseEncoder
        from test_sparse_encoder_cpu import model
        from test_sparse_encoder_gpu import TOL as tol
        self.cfg, _, w, head, self.w16, self.head16 = model("l2")
        self.tol = tol
        self.model = SparseEncoder(w, head, self.cfg, device=device)

    def run(self, ids, lens, seg):
        got = self.model.encode_ids(ids, lens).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (len(lens), self.cfg["vocab_size"])
        assert not (got < 0).any() and not np.signbit(got).any()
        return list(got), {}

    def mirror(self, ids, lens, seg):
        from rag_fin_amd.sparse_encoder import terms_reference
        return list(terms_reference(self.w16, self.head16, self.cfg, ids, lens))

    def check_empty(self, rows, extras, b):
        assert not rows[b].any()


class ColbertHead:
    """rf_encode_tokens at D = 32, the width tests/test_late_interaction_gpu.py's constant was measured at: one unit
    vector per kept token (documents drop the test's skiplist); a row of no tokens has no vectors."""
    pair = False
    DIM = 32

    def __init__(self, device):
        import torch
        from rag_fin_amd.late_interaction import ColBERT
        from test_late_interaction_cpu import l2_model
        from test_late_interaction_gpu import TOL as tol, projection, skip_bits
        self.cfg, w, self.w16 = l2_model()
        self.tol, self.skip = tol, skip_bits()
        proj, self.proj16 = projection(self.DIM)
        self.model = ColBERT(w, proj, self.cfg, device=device)
        self.model._skip = torch.from_numpy(self.skip.view(np.int32)).to(device)

    def run(self, ids, lens, seg):
        off, vec = self.model.encode_ids(ids, lens, is_query=False)
        off, vec = off.cpu().numpy(), vec.cpu().numpy()
        assert off.dtype == np.int32 and vec.dtype == np.float16 and off[0] == 0
        return [vec[off[b]:off[b + 1]] for b in range(len(lens))], {"count": np.diff(off)}

    def mirror(self, ids, lens, seg):
        from rag_fin_amd.late_interaction import tokens_reference
        return tokens_reference(self.w16, self.proj16, self.cfg, ids, lens, skip=self.skip)

    def check_empty(self, rows, extras, b):
        assert rows[b].shape[0] == 0 and extras["count"][b] == 0


class TaggerHead:
    """rf_tag_logits at nine labels: the logits of the positions < len; the entity count of rf_group_entities on those
    logits rides along.  A row of no tokens has no logits and no entities."""
    pair = False

    def __init__(self, device):
        from rag_fin_amd.tagger import TokenClassifier, random_tag_head
        from test_tagger_gpu import CFG2, HEAD_SCALE, TOL as tol, labels_of
        self.cfg, self.tol = CFG2, tol
        w = oenc.random_weights(CFG2, 5)
        head = random_tag_head(384, 9, 5, head_scale=HEAD_SCALE)
        self.model = TokenClassifier(w, head, labels_of(9), CFG2, device=device)
        self.w16, self.head16 = oenc.round_weights_fp16(w), oenc.round_weights_fp16(head)

    def run(self, ids, lens, seg):
        dev = self.model.tag_ids(ids, lens)
        logits = dev.cpu().numpy()
        assert logits.dtype == np.float32 and logits.shape == ids.shape + (9,)
        live = np.arange(ids.shape[1])[None, :] < np.asarray(lens)[:, None]
        assert not logits[~live].any()                              # positions >= len are not written
        groups = self.model.group(dev, lens, max_entities=16).cpu()
        return [logits[b, :lens[b]] for b in range(len(lens))], {"count": groups.count.numpy(), "ent": groups.ent.numpy()}

    def mirror(self, ids, lens, seg):
        from test_tagger_cpu import mirror_tag_logits
        want = mirror_tag_logits(self.w16, self.head16, self.cfg, ids, lens)
        return [want[b, :lens[b]] for b in range(len(lens))]

    def check_empty(self, rows, extras, b):
        assert rows[b].shape[0] == 0 and extras["count"][b] == 0 and (extras["ent"][b] == -1).all()


class SentenceHead:
    """rf_encode_sentences with a Normalize module, CLS or MAX pooling: unit vectors, bounded per component by
    tests/test_embedder_families_gpu.py's TOL_NORM of the mode; an empty set gives the zero vector."""
    pair = False

    def __init__(self, device, mode):
        from rag_fin_amd.embedder import Embedder
        from test_embedder_families_gpu import CFG, SEED, TOL_NORM
        self.cfg, self.mode, self.tol = CFG, mode, TOL_NORM[mode]
        w = oenc.random_weights(CFG, SEED)
        self.w16 = oenc.round_weights_fp16(w)
        self.model = Embedder(w, CFG, device=device, pooling=mode, normalize=True)

    def run(self, ids, lens, seg):
        got = self.model.encode_ids(ids, lens, out_dtype="float32").cpu().numpy()
        assert got.shape == (len(lens), 384)
        return list(got), {}

    def mirror(self, ids, lens, seg):
        from rag_fin_amd.embedder import pool_reference
        hidden = oenc.encode(self.w16, self.cfg, ids, lens, return_hidden=True)
        return list(pool_reference(hidden, lens, None, self.mode, True))

    def check_empty(self, rows, extras, b):
        assert not rows[b].any()


HEADS = {"cross_encoder": CrossEncoderHead, "reader": ReaderHead, "splade": SpladeHead, "colbert": ColbertHead,
         "tagger": TaggerHead, "sentence_cls": lambda device: SentenceHead(device, "cls"),
         "sentence_max": lambda device: SentenceHead(device, "max")}


@pytest.fixture(scope="module")
def heads(gpu_device):
    return functools.lru_cache(maxsize=None)(lambda name: HEADS[name](gpu_device))


def head_error(got_rows, want_rows):
    """The largest |got - mirror| over the rows' defined outputs (a pair of -inf counts as equal)."""
    worst = 0.0
    for g, w in zip(got_rows, want_rows):
        assert g.shape == w.shape, (g.shape, w.shape)
        if g.size == 0:
            continue
        g = g.astype(np.float64)
        fin = np.isfinite(w)
        assert np.array_equal(g[~fin], w[~fin]) and np.isfinite(g[fin]).all()
        if fin.any():
            worst = max(worst, float(np.abs(g - w)[fin].max()))
    return worst


def assert_within_head_bound(head, name, got_rows, want_rows):
    from conftest import record_measurement
    err = head_error(got_rows, want_rows)
    record_measurement(f"encoder_paths_{name}", max_abs=err, bound=head.tol, rows=len(want_rows))
    print(f"encoder_paths_{name}: max |got - mirror| = {err:.3e} (the head's constant: {head.tol})")
    assert err < head.tol, err


def assert_rows_same_bits(a, b, rows_a, rows_b):
    (ra, xa), (rb, xb) = a, b
    for i, j in zip(rows_a, rows_b):
        assert same_bits(ra[i], rb[j]), (i, j)
        for k in xa:
            assert same_bits(xa[k][i], xb[k][j]), (k, i, j)


@pytest.mark.parametrize("name", list(HEADS))
def test_head_on_the_direct_path(heads, name):
    """40 x 64 = 2 560 slots, k_linear's 64-token tiles: ragged, the lengths 1, 31, 32, 33, 64 among the rows, the
    second segment of a pair starting at 1, 31, 32, 33.  Every row against the head's mirror."""
    head = heads(name)
    b = epc.head_batch("direct", head.cfg["vocab_size"])
    seg = b["seg"] if head.pair else None
    rows, _ = head.run(b["ids"], b["lens"], seg)
    assert_within_head_bound(head, f"{name}_direct_40x64", rows, head.mirror(b["ids"], b["lens"], seg))


@pytest.mark.parametrize("name", list(HEADS))
def test_head_on_the_dma_and_the_wide_path(heads, name):
    """64 x 128 (k_linear_dma<0>, 128-token workgroups) and 384 x 128 (k_linear_dma<1>, 256-token ones) whose first 64
    rows are those same rows: their outputs are bit-identical between the two calls; eight rows among the last 64 of
    the wide batch against the head's mirror."""
    head = heads(name)
    b = epc.head_batch("wide", head.cfg["vocab_size"])
    ids, lens, probes = b["ids"], b["lens"], b["probes"]
    seg = b["seg"] if head.pair else None
    wide = head.run(ids, lens, seg)
    narrow = head.run(ids[:64], lens[:64], None if seg is None else seg[:64])
    assert_rows_same_bits(narrow, wide, range(64), range(64))
    want = head.mirror(ids[probes], lens[probes], None if seg is None else seg[probes])
    assert_within_head_bound(head, f"{name}_wide_384x128", [wide[0][p] for p in probes], want)


@pytest.mark.parametrize("name", list(HEADS))
def test_head_on_a_nearly_empty_stream(heads, name):
    """64 x 128 with three live rows (33, 1 and 95 tokens at rows 0, 31 and 63: M = 129, one token into the second
    128-token tile): the live rows against the mirror and against their bits in the dense twin of the batch; the empty
    rows give what the head documents.  Every head admits zero-length rows, so the case applies to all of them."""
    head = heads(name)
    b = epc.head_batch("sparse", head.cfg["vocab_size"])
    ids, lens = b["ids"], b["lens"]
    seg, dense_seg = (b["seg"], b["dense_seg"]) if head.pair else (None, None)
    live = np.flatnonzero(lens)
    got = head.run(ids, lens, seg)
    for r in np.flatnonzero(lens == 0):
        head.check_empty(got[0], got[1], r)
    want = head.mirror(ids[live], lens[live], None if seg is None else seg[live])
    assert_within_head_bound(head, f"{name}_sparse_64x128_M129", [got[0][r] for r in live], want)
    dense = head.run(ids, b["dense"], dense_seg)
    assert_rows_same_bits(got, dense, live, live)


def test_token_vectors_do_not_depend_on_workspace_contents(heads, gpu_device):
    """rf_encode_tokens (its projection kernel reads the hidden rows tile-wise) at 64 x 128, M = 129, through the C
    ABI -- ColBERT.encode_ids takes no workspace -- with a caller-owned workspace of exactly
    rf_encode_tokens_workspace_bytes filled with each byte pattern: the offsets and the vectors are those of
    encode_ids, bit for bit."""
    import torch
    from rag_fin_amd import _lib
    head = heads("colbert")
    col = head.model
    _, B, T, M = epc.WORKSPACE_CASES[1]
    ids, lens, _ = epc.edge_batch(*epc.WORKSPACE_CASES[1])
    off0, vec0 = (t.cpu().numpy() for t in col.encode_ids(ids, lens, is_query=False))
    n = int(off0[-1])
    assert 0 < n <= M and M == 129
    ids_d = torch.as_tensor(ids).to(gpu_device).contiguous()
    lens_d = torch.as_tensor(lens).to(gpu_device).contiguous()
    h = col.encoder.handle
    tok_head = _lib.TokenHead(col._proj.data_ptr(), col.dim, col._skip.data_ptr(), int(col.cfg["vocab_size"]))
    ws = torch.empty(col.lib.rf_encode_tokens_workspace_bytes(h, B, T), dtype=torch.uint8, device=gpu_device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    for fill in FILLS:
        ws.fill_(fill)
        off = torch.full((B + 1,), -7, dtype=torch.int32, device=gpu_device)
        vec = torch.full((B * T, col.dim), float("nan"), dtype=torch.float16, device=gpu_device)
        with torch.cuda.device(gpu_device):
            _lib.check(col.lib.rf_encode_tokens(h, p(ids_d), p(lens_d), B, T, ctypes.byref(tok_head), p(off), p(vec),
                                                p(ws), ws.numel(), _lib.current_stream_ptr()))
        got_off, got_vec = off.cpu().numpy(), vec.cpu().numpy()
        assert np.array_equal(got_off, off0), hex(fill)
        assert np.isfinite(got_vec[:n]).all() and same_bits(got_vec[:n], vec0[:n]), hex(fill)
