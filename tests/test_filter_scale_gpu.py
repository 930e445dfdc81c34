"""The filter buffer above 1 048 576 rows, where its tile plan leaves the regime every other test runs in.

plan_tiles (csrc/filter.hip) cuts the mask into at most 1024 tiles of 32 * ceil(nblk / 32768) words.
Up to 1 048 576 rows a tile is 32 words; the sizes here are the first ones past each threshold:
  1 048 577   tile_words   64  second trip of k_filter_eval's wave loop; the last tile is ONE word
  8 388 641   tile_words  288  k_filter_compact: a full 256-word chunk, then a partial one, the running
                               output offset carried across them
  33 554 465  tile_words 1056  k_filter_copy: a second stride of its 1024 threads
Each test asserts header word 3 (n_tiles, written by the device) against oracle.filter_program.plan:
that, with the plan table of tests/test_filter_reference_cpu.py, is the proof that the regime was
reached.  Every buffer is allocated here and prefilled with 0xA5 bytes."""
from ctypes import c_void_p

import numpy as np
import pytest

from oracle import c_oracle, filter_program as fp, search as osearch
from rag_fin_amd import _lib

pytestmark = pytest.mark.gpu

TILE_WORDS = {1_048_576: 32, 1_048_577: 64, 8_388_641: 288, 33_554_465: 1056}


def new_buffer(n, device):
    import torch
    return torch.full((_lib.load_library().rf_filter_bytes(n),), 0xA5, dtype=torch.uint8, device=device)


def defined_parts(buf, n):
    """(header, the nblk mask words, the first hdr[2] block entries); what lies behind is scratch."""
    raw = buf.cpu().numpy().view(np.uint32)
    nblk = (n + 31) // 32
    a = (nblk * 4 + 15) // 16 * 16 // 4
    hdr = raw[:4].tolist()
    return hdr, raw[4:4 + nblk].copy(), raw[4 + a:4 + a + min(hdr[2], nblk)].copy()


def from_mask(words, n, device):
    import torch
    lib = _lib.load_library()
    buf = new_buffer(n, device)
    w = torch.from_numpy(words.view(np.int32)).to(device)
    with torch.cuda.device(device):
        _lib.check(lib.rf_filter_from_mask(c_void_p(w.data_ptr()), n, c_void_p(buf.data_ptr()), _lib.current_stream_ptr()))
    torch.cuda.synchronize(device)
    return buf


def clear_past(words, n):
    out = words.copy()
    if n % 32:
        out[-1] &= np.uint32((1 << (n % 32)) - 1)
    return out


def check_buffer(buf, n, want_words):
    """The four assertions: header {n, popcount, non-zero words, plan(n).n_tiles}, mask, block list."""
    hdr, mask, blocks = defined_parts(buf, n)
    want_blocks = np.flatnonzero(want_words).astype(np.uint32)
    assert hdr == [n, fp.popcount(want_words), want_blocks.size, fp.plan(n)[2]]
    assert np.array_equal(mask, want_words), np.flatnonzero(mask != want_words)[:8]
    assert np.array_equal(blocks, want_blocks), np.flatnonzero(blocks != want_blocks)[:8]
    return hdr, mask, blocks


def mixture(n, rng):
    """Mask words drawn as uint32 (no per-row array): ~30 % of the words non-zero, and on top of that
    whole tiles of zero words, whole tiles without a zero word, non-zero words first and last in the
    two tiles either side of a tile edge, and a last word with every bit set (garbage past n)."""
    nblk, tw, nt = fp.plan(n)
    assert nt >= 16
    words = rng.integers(1, 2 ** 32, nblk, dtype=np.uint64).astype(np.uint32)
    words[rng.random(nblk) >= 0.3] = 0
    tile = lambda t: slice(t * tw, (t + 1) * tw)   # noqa: E731
    for t in (1, nt // 2):
        words[tile(t)] = 0
    for t in (2, nt // 2 + 1):
        words[tile(t)] = rng.integers(1, 2 ** 32, tw, dtype=np.uint64).astype(np.uint32)
    for t in (5, 6, nt - 3, nt - 2):          # the edges 5|6 and nt-3|nt-2: last word of one, first of the next
        words[t * tw] = 0x80000001
        words[(t + 1) * tw - 1] = 0x00010000
    words[-1] = 0xFFFFFFFF
    for t in (1, nt // 2):
        assert not words[tile(t)].any()
    for t in (2, nt // 2 + 1):
        assert words[tile(t)].all()
    return words


@pytest.mark.parametrize("n", sorted(TILE_WORDS))
def test_from_mask_in_every_tile_regime(gpu_device, n):
    nblk, tw, nt = fp.plan(n)
    assert tw == TILE_WORDS[n]
    words = mixture(n, np.random.default_rng(n))
    want = clear_past(words, n)
    assert want[-1] != 0 and (n % 32 == 0 or want[-1] != words[-1])
    assert 0.25 < np.count_nonzero(want) / nblk < 0.4
    a = check_buffer(from_mask(words, n, gpu_device), n, want)
    b = defined_parts(from_mask(words, n, gpu_device), n)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("n", [1_048_577, 8_388_641])
def test_eval_in_the_second_and_third_regime(gpu_device, n):
    """(lo <= primary_value < hi AND chunk_type in a code set) OR row in a list, the columns the
    program does not read passed as NULL."""
    import torch
    lib = _lib.load_library()
    nblk, tw, nt = fp.plan(n)
    assert tw == TILE_WORDS[n]
    rng = np.random.default_rng(n)
    vals = rng.standard_normal(n)
    vals[rng.integers(0, n, n // 20)] = np.nan
    vals[rng.integers(0, n, n // 20)] = -0.0
    codes = rng.integers(0, 10, n, dtype=np.int32)
    edge = (nt // 3 + 1) * tw * 32              # the first row of a tile; edge - 1 is the last row of the one before
    listed = np.array([0, edge - 1, edge, n - 1], dtype=np.uint32)
    vals[listed] = np.nan                        # only the row list lets these through
    code_set = np.array([(1 << 1) | (1 << 3) | (1 << 4) | (1 << 7)], dtype=np.uint32)
    lo, hi = -0.0, 1.0
    prog = [(fp.FOP_RANGE, 3, 0, 0, fp.FRANGE_LO_INCL, lo, hi), (fp.FOP_CODESET, 1, 0, 1, 0, 0.0, 0.0),
            (fp.FOP_AND, 0, 0, 0, 0, 0.0, 0.0), (fp.FOP_ROWLIST, 0, 0, listed.size, 0, 0.0, 0.0),
            (fp.FOP_OR, 0, 0, 0, 0, 0.0, 0.0)]
    ops = (_lib.FilterOp * len(prog))()
    for i, (op, col, off, ln, flags, a, b) in enumerate(prog):
        ops[i].op, ops[i].column, ops[i].off, ops[i].len, ops[i].flags, ops[i].lo, ops[i].hi = op, col, off, ln, flags, a, b

    with np.errstate(invalid="ignore"):
        want_rows = (vals >= lo) & (vals < hi) & np.isin(codes, [1, 3, 4, 7])
    assert not want_rows[listed].any() and want_rows[vals == 0].any()
    want_rows[listed] = True
    want = fp.pack_rows(want_rows)
    if n == 1_048_577:
        assert (nblk - 1) % tw == 0 and want[-1] == 1    # the last tile: one word, one row, non-zero

    vals_d = torch.from_numpy(vals).to(gpu_device)
    codes_d = torch.from_numpy(codes).to(gpu_device)
    cs_d = torch.from_numpy(code_set.view(np.int32)).to(gpu_device)
    rl_d = torch.from_numpy(listed.view(np.int32)).to(gpu_device)
    ptrs = (c_void_p * _lib.RF_FILTER_COLUMNS)(None, c_void_p(codes_d.data_ptr()), None, c_void_p(vals_d.data_ptr()))
    buf = new_buffer(n, gpu_device)
    with torch.cuda.device(gpu_device):
        _lib.check(lib.rf_filter_eval_bitmaps(ops, len(prog), c_void_p(cs_d.data_ptr()), c_void_p(rl_d.data_ptr()), None,
                                              ptrs, n, c_void_p(buf.data_ptr()), _lib.current_stream_ptr()))
    torch.cuda.synchronize(gpu_device)
    check_buffer(buf, n, want)


def test_dense_search_reads_a_block_list_of_the_second_regime(gpu_device):
    """One consumer: rf_search_filtered over 1 048 577 rows against the CPU oracle on the passing rows."""
    import torch
    from rag_fin_amd.store import GpuIndex
    n, d, B, k = 1_048_577, 64, 7, 10
    nblk, tw, nt = fp.plan(n)
    assert tw == 64
    c16 = osearch.synth_unit_rows(n, d, 21)
    q16 = osearch.synth_unit_rows(B, d, 22)
    rng = np.random.default_rng(23)
    edge = 300 * tw * 32
    S = np.unique(np.concatenate([rng.integers(0, n, 2000), [edge - 1, edge, n - 1]]))
    words = np.zeros(nblk, dtype=np.uint32)
    np.bitwise_or.at(words, S >> 5, (np.uint32(1) << (S & 31).astype(np.uint32)))
    filt = from_mask(words, n, gpu_device)
    assert defined_parts(filt, n)[0] == [n, S.size, np.count_nonzero(words), nt]
    ix = GpuIndex(d, n, gpu_device)
    ix.add(torch.from_numpy(c16).to(gpu_device))
    scores, ids, exact, flags = ix.search_raw(torch.from_numpy(q16).to(gpu_device), k, want_exact=True, filt=filt)
    torch.cuda.synchronize()
    assert int(flags.abs().sum()) == 0
    es, ei = c_oracle.search(q16, c16[S], k)
    ei = S[ei]
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, ei), f"ids differ at {np.argwhere(ids != ei)[:5]}"
    assert np.array_equal(exact.cpu().numpy(), es)
    assert np.array_equal(scores.cpu().numpy(), es.astype(np.float32))
