"""k_filter_eval against the numpy interpreter (oracle/filter_program.py) over random postfix programs.

The programs come from the seeded generator of tests/test_filter_reference_cpu.py as raw rf_filter_op
arrays, not from the expression compiler: stacks up to RF_FILTER_MAX_DEPTH = 32 (the bool stack
fills its register), RF_FILTER_MAX_OPS = 64 operations, NOT on a deep stack, code sets of 0 and 1
words over columns with negative and out-of-set codes, empty and one-row row lists, bitmap leaves
shorter than the row words, ranges over +-inf / +-0.0 bounds in all four inclusivity combinations
against NaN, +-0.0, +-inf and subnormal values.  What the set holds is counted on the CPU there
(test_the_generated_programs_hold_what_the_gpu_test_claims_to_run); here every program's mask words,
header counts and block list must equal the interpreter's, launched through rf_filter_eval_bitmaps
into a buffer prefilled with 0xA5."""
from ctypes import c_void_p

import numpy as np
import pytest

from oracle import filter_program as fp
from rag_fin_amd import _lib
from test_filter_reference_cpu import N_MAIN, N_PROGRAMS, N_SUBSET, SMALL_NS, interpret, program_set

pytestmark = pytest.mark.gpu


def ops_array(prog):
    arr = (_lib.FilterOp * len(prog))()
    for i, (op, col, off, ln, flags, lo, hi) in enumerate(prog):
        arr[i].op, arr[i].column, arr[i].off, arr[i].len = op, col, off, ln
        arr[i].flags, arr[i].lo, arr[i].hi = flags, lo, hi
    return arr


def run_set(ps, device):
    """Every program of the set through the kernel -> [(header, mask words, valid block entries)]."""
    import torch
    lib = _lib.load_library()
    n = ps.n
    nblk = (n + 31) // 32
    a = (nblk * 4 + 15) // 16 * 16 // 4
    dev = lambda x, t: torch.from_numpy(np.ascontiguousarray(x).view(t)).to(device)   # noqa: E731
    cols = [dev(ps.codes[c], np.int32) for c in range(3)] + [dev(ps.values, np.float64)]
    pools = [dev(ps.code_sets, np.int32), dev(ps.row_lists, np.int32), dev(ps.bitmaps, np.int32)]
    ptrs = (c_void_p * _lib.RF_FILTER_COLUMNS)(*[c_void_p(t.data_ptr()) for t in cols])
    buf = torch.empty(lib.rf_filter_bytes(n), dtype=torch.uint8, device=device)
    out = []
    with torch.cuda.device(device):
        for prog in ps.programs:
            buf.fill_(0xA5)   # nothing may rely on what an earlier program, or the allocator, left behind
            ops = ops_array(prog)
            _lib.check(lib.rf_filter_eval_bitmaps(ops, len(prog), *[c_void_p(t.data_ptr()) for t in pools], ptrs, n,
                                                  c_void_p(buf.data_ptr()), _lib.current_stream_ptr()))
            raw = buf.cpu().numpy().view(np.uint32)
            out.append((raw[:4].tolist(), raw[4:4 + nblk].copy(), raw[4 + a:4 + a + min(int(raw[2]), nblk)].copy()))
    return out


def check_set(ps, device):
    got = run_set(ps, device)
    assert len(got) == len(ps.programs)
    bad = []
    for i, (prog, (hdr, mask, blocks)) in enumerate(zip(ps.programs, got)):
        words = fp.pack_rows(interpret(ps, prog))
        want_blocks = np.flatnonzero(words).astype(np.uint32)
        ok = (hdr == [ps.n, fp.popcount(words), want_blocks.size, fp.plan(ps.n)[2]] and np.array_equal(mask, words)
              and np.array_equal(blocks, want_blocks))
        if not ok:
            bad.append((i, len(prog), hdr, np.flatnonzero(mask != words)[:4].tolist()))
    assert not bad, f"{len(bad)} of {len(got)} programs differ from the interpreter, the first: {bad[:3]}"


def test_two_hundred_random_programs_equal_the_interpreter(gpu_device):
    ps = program_set(N_MAIN)
    assert len(ps.programs) == N_PROGRAMS
    check_set(ps, gpu_device)


@pytest.mark.parametrize("n", SMALL_NS)
def test_the_forced_shapes_at_the_word_and_ballot_edges(gpu_device, n):
    ps = program_set(n, N_SUBSET)
    assert len(ps.programs) == N_SUBSET
    check_set(ps, gpu_device)
