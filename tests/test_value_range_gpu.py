"""Exact search across the finite fp16 value range: corpora from
oracle/adversarial.value_range whose components lie far from the exponent of a unit row --
subnormals, values at the largest finite fp16, one row whose norm dominates max_norm2, per-row
scales over 2^24, cancelling signs.  NaN and inf inputs are out of scope.

Bar, as in tests/test_search_gpu.py: ids and ranks equal to the C oracle's, fp64 scores bit-equal,
fp32 scores == float32(oracle).  tests/test_near_ties_cpu.py asserts the premises (the share of
subnormals, and that an MFMA path flushing them would give another top-10).

The eps bound itself is asserted through debug_scores at every dim the debug kernel has: for every
(query, row) |mfma - exact| <= dim 2^-23 |q| |c|, the bound of DESIGN 4.4 before its 1.25 slack,
norms in fp64.  Where it comes from: an fp16 product is exact in fp32, the accumulation takes at
most dim roundings of relative size 2^-24 (round to nearest) on partial sums bounded by
sum |q_d c_d| <= |q| |c|; 2^-23 leaves a factor 2 for an accumulator that truncates.  The worst
ratio per dim and kind goes to record_measurement (profiles/value_range_measurements.jsonl)."""
import numpy as np
import pytest

from oracle import adversarial as adv, c_oracle, search as osearch
from test_search_gpu import check_against_oracle, make_index

pytestmark = pytest.mark.gpu

DIMS = (64, 384, 1024)
SIZES = (3_000, 20_011)
B, K = 16, 10


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", ["tiny", "huge", "mixed", "cancel"])
def test_parity_with_oracle(gpu_device, kind, dim, n):
    """tiny: scaled by 2^-10 (2^-11 at dim 64), mostly subnormal components; huge: scaled by 2^10 with components at
    +-65504, scores up to ~1e10 whose fp32 form must still be float32(oracle); mixed: per-row and
    per-query scales 2^U[-12, 12]; cancel: +-large components, scores near 0 beside |q| |c|.

    The raw path runs unflagged, with one exception that follows from the bound itself: in the
    cancel corpus eps = 1.25 dim 2^-23 (24 sqrt(dim)) (48 sqrt(dim)) grows with dim^2 while the
    scores keep a spread of ~48 * 8 = 384.  At dim 384 2 eps is 50, an eighth of the spread; at dim
    1024 it is 362, so the rescoring set holds a large share of the corpus and overflows
    RF_RESCORE_CAP: there a query may be flagged, one that is not must already be exact, and
    search() answers all of them through the ladder (measured: 7 of 16 queries flagged at 3 000
    rows, 16 of 16 at 20 011)."""
    import torch
    c16, q16 = adv.value_range(kind, n, dim, B, 3)
    ix = make_index(c16, gpu_device)
    if not (kind == "cancel" and dim == 1024):
        check_against_oracle(ix, q16, c16, K, gpu_device)
        return
    scores, ids, exact, flags = ix.search_raw(torch.from_numpy(q16).to(gpu_device), K, want_exact=True)
    clean = np.flatnonzero(flags.cpu().numpy() == 0)
    print(f"cancel, dim {dim}, n {n}: {B - clean.size} of {B} queries flagged")
    os_, oi = c_oracle.search(q16, c16, K)
    assert np.array_equal(ids.cpu().numpy()[clean], oi[clean])
    assert np.array_equal(exact.cpu().numpy()[clean], os_[clean])
    assert np.array_equal(scores.cpu().numpy()[clean], os_[clean].astype(np.float32))
    check_against_oracle(ix, q16, c16, K, gpu_device, raw=False)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", DIMS)
def test_one_outlier_row_inflates_eps_for_every_query(gpu_device, dim, n):
    """Unit rows and one row of norm ~2^13: eps grows ~8 000-fold for every query, so queries may
    be flagged -- search() stays exact; with the outlier deleted search_raw runs unflagged again."""
    import torch
    c16, q16 = adv.value_range("outlier", n, dim, B, 3)
    ix = make_index(c16, gpu_device)
    _, _, _, flags = ix.search_raw(torch.from_numpy(q16).to(gpu_device), K)
    print(f"dim {dim}, n {n}: {int((flags != 0).sum())} of {B} queries flagged with the outlier in")
    check_against_oracle(ix, q16, c16, K, gpu_device, raw=False)
    keep = np.flatnonzero(np.arange(n) != n // 3)
    ix.compact(keep)
    check_against_oracle(ix, q16, np.ascontiguousarray(c16[keep]), K, gpu_device)


@pytest.mark.parametrize("dim", [64, 128, 256, 384, 512, 768, 1024])
@pytest.mark.parametrize("kind", adv.KINDS)
def test_mfma_error_stays_inside_the_eps_bound(gpu_device, kind, dim):
    import torch
    from conftest import record_measurement
    c16, q16 = adv.value_range(kind, 256, dim, 40, 5)
    ix = make_index(c16, gpu_device)
    got = ix.debug_scores(torch.from_numpy(q16).to(gpu_device)).cpu().numpy().astype(np.float64)
    exact = osearch.exact_scores(q16, c16)
    qn = np.sqrt((q16.astype(np.float64) ** 2).sum(axis=1))
    cn = np.sqrt((c16.astype(np.float64) ** 2).sum(axis=1))
    bound = dim * 2.0 ** -23 * qn[:, None] * cn[None, :]
    assert (bound > 0).all()
    ratio = float((np.abs(got - exact) / bound).max())
    print(f"{kind}, dim {dim}: worst |mfma - exact| / (dim 2^-23 |q| |c|) = {ratio:.3e}")
    record_measurement(f"mfma_error_over_eps_bound[{kind}]", dim=dim, ratio=ratio)
    assert ratio <= 1.0, (kind, dim, ratio)
