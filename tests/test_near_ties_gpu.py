"""The exactness margin under weight: near-tie clusters from
oracle/adversarial.py -- rows whose contract scores differ by a fraction of a float32 spacing, so
that no fp32 score can rank them -- embedded in random unit corpora, through every search form.
Only the 2 eps widening of k_threshold / k_merge together with the fp64 rescoring gets these
right; tests/test_near_ties_cpu.py asserts the premises.

Bar, as in tests/test_search_gpu.py: ids and ranks equal to the C oracle's, fp64 scores bit-equal,
fp32 scores == float32(oracle), flags 0 on the raw path unless the case is about overflow.

Corpora: 3 000 rows (the small-corpus path) and 20 011 rows (sample pass, fold, ragged last
block); cluster rows are scattered with a stride that is no multiple of 32, interleaved between
queries.  Each corpus and its oracle ranking (top 64, of which k = 5 and 10 are prefixes) is
computed once and shared."""
import functools

import numpy as np
import pytest

from oracle import adversarial as adv, c_oracle, search as osearch
from test_search_gpu import check_against_oracle, make_index

pytestmark = pytest.mark.gpu

SMALL, LARGE = 3_000, 20_011


@functools.lru_cache(maxsize=4)
def case(n, dim, B, m, n_clusters=None, seed=1234):
    """B queries of which the first n_clusters (default: all) own a cluster of m rows ->
    (corpus, queries, cluster positions, oracle scores f64 [B, 64], oracle ids [B, 64]); read-only."""
    nc = B if n_clusters is None else n_clusters
    qs, cl = zip(*(adv.near_tie_cluster(dim, m, s) for s in range(nc)))
    q16 = np.concatenate([np.stack(qs), osearch.synth_unit_rows(B - nc, dim, seed + 1)]) if nc < B else np.stack(qs)
    c16, pos = adv.embed_clusters(n, dim, seed, cl, stride=adv.scatter_stride(n, nc * m))
    os_, oi = c_oracle.search(q16, c16, 64)
    for a in (c16, q16, os_, oi):
        a.setflags(write=False)
    return c16, q16, pos, os_, oi


def to_dev(a, device):
    import torch
    return torch.from_numpy(np.array(a)).to(device)


def assert_equal(scores, ids, exact, es, ei, what=""):
    ids = ids.cpu().numpy() if hasattr(ids, "cpu") else ids
    assert np.array_equal(ids, ei), f"{what}: ids differ at {np.argwhere(ids != ei)[:5].tolist()}"
    if exact is not None:
        assert np.array_equal(exact.cpu().numpy(), es), f"{what}: fp64 scores differ"
    scores = scores.cpu().numpy() if hasattr(scores, "cpu") else scores
    assert np.array_equal(scores, es.astype(np.float32)), f"{what}: fp32 scores differ"


def cut_is_inside_a_cluster(pos, oi, k):
    """Rank k and rank k + 1 (where the oracle has it) of query 0 are rows of its own cluster."""
    return oi[0, k - 1] in pos[0] and (k >= oi.shape[1] or oi[0, k] in pos[0])


# ---- the plain 64-query sweep -------------------------------------------------------------------------
# dims 64 / 384 / 768 / 1024 = KS 4 / 24 / 48 / 64: both wave counts and every ring shape
SWEEPS = [(SMALL, 64, 64, 33), (SMALL, 384, 3, 97), (SMALL, 768, 16, 97), (SMALL, 1024, 3, 97),
          (LARGE, 64, 64, 33), (LARGE, 384, 64, 97), (LARGE, 768, 33, 97), (LARGE, 1024, 64, 97)]


@pytest.mark.parametrize("k", [5, 10, 64])
@pytest.mark.parametrize("n,dim,B,m", SWEEPS)
def test_every_query_cuts_its_own_cluster(gpu_device, n, dim, B, m, k):
    """k = 5, 10 and (m = 97) 64 cut inside the cluster; k = 64 at dim 64 (m = 33) cuts below it."""
    import torch
    c16, q16, pos, os_, oi = case(n, dim, B, m)
    assert cut_is_inside_a_cluster(pos, oi, k) == (k < m)
    ix = make_index(np.array(c16), gpu_device)
    scores, ids, exact, flags = ix.search_raw(to_dev(q16, gpu_device), k, want_exact=True)
    torch.cuda.synchronize()
    assert int(flags.abs().sum()) == 0, f"flags set: {flags.cpu().numpy()}"
    assert_equal(scores, ids, exact, os_[:, :k], oi[:, :k])


# ---- the sample fold ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 64])
def test_clusters_in_and_across_sampled_blocks(gpu_device, k):
    """Block arithmetic of test_duplicate_rows_in_sample_blocks: blocks j * bs are sampled.  Cluster
    0 lies wholly inside four sampled blocks (24 rows each, 25 in the last), cluster 1 is one run
    of 97 rows that starts inside a sampled block and crosses the unsampled and sampled blocks
    behind it: the best and second best of a lane then differ by less than a float32 spacing."""
    n, dim, m = LARGE, 384, 97
    nblk = (n + 31) // 32
    n_work = max(nblk // 16, 256)
    bs = nblk // n_work
    assert bs >= 2
    c16 = osearch.synth_unit_rows(n, dim, 99)
    q0, rows0 = adv.near_tie_cluster(dim, m, 0)
    q1, rows1 = adv.near_tie_cluster(dim, m, 1)
    at = 0
    for j, cnt in zip((3, 7, 11, 15), (24, 24, 24, 25)):
        base = 32 * j * bs + 5
        c16[base:base + cnt] = rows0[at:at + cnt]
        at += cnt
    base = 32 * 20 * bs + 16
    c16[base:base + m] = rows1
    q16 = np.concatenate([np.stack([q0, q1]), osearch.synth_unit_rows(14, dim, 98)])
    check_against_oracle(make_index(c16, gpu_device), q16, c16, k, gpu_device)


# ---- the wide sweep -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
@pytest.mark.parametrize("B", [130, 256])
def test_wide_sweep_with_clusters_for_first_65th_and_last_query(gpu_device, n, B):
    import torch
    dim, m, k = 384, 97, 10
    qs, cl = zip(*(adv.near_tie_cluster(dim, m, s) for s in range(3)))
    q16 = osearch.synth_unit_rows(B, dim, 78)
    for b, q in zip((0, 64, B - 1), qs):
        q16[b] = q
    c16, pos = adv.embed_clusters(n, dim, 77, cl, stride=adv.scatter_stride(n, 3 * m))
    ix = make_index(c16, gpu_device)
    check_against_oracle(ix, q16, c16, k, gpu_device)
    q = to_dev(q16, gpu_device)
    s1, i1, e1, _ = ix.search_raw(q, k, want_exact=True)
    s1, i1, e1 = s1.clone(), i1.clone(), e1.clone()
    parts = [ix.search_raw(q[a:a + 64].contiguous(), k, want_exact=True) for a in range(0, B, 64)]
    torch.cuda.synchronize()
    for got, j in ((s1, 0), (i1, 1), (e1, 2)):
        assert torch.equal(got, torch.cat([p[j] for p in parts]))


# ---- overflow of the rescoring set ------------------------------------------------------------------------
def test_a_400_row_cluster_overflows_the_rescoring_set_and_the_ladder_answers(gpu_device):
    """400 near-tied rows > RF_RESCORE_CAP (256): the query is flagged (with at most a couple of
    others); search() and search_host() return the oracle's answer through the ladder."""
    n, dim, B, k = LARGE, 384, 8, 10
    c16, q16, pos, os_, oi = case(n, dim, B, 400, n_clusters=1)
    ix = make_index(np.array(c16), gpu_device)
    q = to_dev(q16, gpu_device)
    _, _, _, flags = ix.search_raw(q, k)
    flags = flags.cpu().numpy()
    assert flags[0] != 0 and int((flags != 0).sum()) <= 3, flags
    scores, ids, exact = ix.search(q, k, want_exact=True)
    assert_equal(scores, ids, exact, os_[:, :k], oi[:, :k], "search")
    hs, hi = ix.search_host(q, k)
    assert_equal(hs, hi, None, os_[:, :k], oi[:, :k], "search_host")


# ---- paging -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_page_edge_inside_a_cluster(gpu_device, n):
    """search_large, k = 200: ranks 1..97 of every query are its cluster, so the page edge at 64 falls
    inside it and "strictly after the previous page's last hit" has to hold in fp64."""
    dim, m, B, k = 384, 97, 3, 200
    c16, q16, pos, _, oi64 = case(n, dim, B, m)
    assert all(np.isin(oi64[b], pos[b]).all() for b in range(B))
    ix = make_index(np.array(c16), gpu_device)
    scores, ids, exact = ix.search_large(to_dev(q16, gpu_device), k, want_exact=True)
    os_, oi = c_oracle.search(np.array(q16), np.array(c16), k)
    assert all(np.isin(oi[b, :m], pos[b]).all() for b in range(B))
    assert_equal(scores, ids, exact, os_, oi)


# ---- range search -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_band_edges_on_cluster_rows(gpu_device, n):
    """range_filter = the exact score of the median row of query 0's cluster, radius = that of its
    10th-lowest row: each bound alone and both, alone and inside a filter.  Expected: the oracle's
    radius < score <= range_filter in fp64."""
    from test_filtered_search_gpu import filter_from_mask
    from test_range_search_gpu import check_band
    dim, m, B, k = 384, 97, 3, 64
    c16, q16, pos, _, _ = case(n, dim, B, m)
    c16, q16 = np.array(c16), np.array(q16)
    S = osearch.exact_scores(q16, c16)
    own = np.sort(S[0, pos[0]])
    hi, lo = float(own[m // 2]), float(own[9])
    inside = int(((S[0] > lo) & (S[0] <= hi)).sum())
    assert 30 <= inside <= m // 2 - 9 + 2, inside              # (a tie at either edge may move the count)
    ix = make_index(c16, gpu_device)
    mask = np.random.default_rng(4).random(n) < 0.6
    assert m // 3 < mask[pos[0]].sum() < m
    filt = filter_from_mask(mask, gpu_device)
    for band in ((lo, np.inf), (-np.inf, hi), (lo, hi)):
        check_band(ix, q16, S, band[0], band[1], k, gpu_device)
        check_band(ix, q16, S, band[0], band[1], k, gpu_device, mask=mask, filt=filt)


# ---- filtered search ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_filters_that_thin_the_cluster_and_reject_its_best(gpu_device, n):
    from test_filtered_search_gpu import check_filtered
    dim, m, B = 384, 97, 3
    c16, q16, pos, _, oi = case(n, dim, B, m)
    c16, q16 = np.array(c16), np.array(q16)
    ix = make_index(c16, gpu_device)
    every_other = np.ones(n, dtype=bool)
    for p in pos:
        every_other[p[1::2]] = False
    no_best = np.ones(n, dtype=bool)
    no_best[oi[:, 0]] = False
    for mask in (every_other, no_best):
        for k in (10, 64):
            check_filtered(ix, q16, c16, mask, k, gpu_device)


# ---- SQ8 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_sq8_equals_flat_and_the_oracle(gpu_device, n):
    """The same index with the int8 shadow built.  A query the SQ8 pass leaves unflagged is already
    the oracle's on the raw path; search(sq8=True) is, for every query."""
    import torch
    dim, m, B, k = 384, 97, 8, 10
    c16, q16, pos, os_, oi = case(n, dim, B, m)
    ix = make_index(np.array(c16), gpu_device)
    ix.enable_sq8()
    q = to_dev(q16, gpu_device)
    s8, i8, e8, f8 = ix.search_raw(q, k, want_exact=True, sq8=True)
    torch.cuda.synchronize()
    clean = np.flatnonzero(f8.cpu().numpy() == 0)
    print(f"n = {n}: {clean.size} of {B} queries unflagged by the SQ8 pass")
    assert_equal(s8[clean], i8[clean], e8[clean], os_[clean, :k], oi[clean, :k], "raw SQ8")
    s8, i8, e8 = ix.search(q, k, want_exact=True, sq8=True)
    s0, i0, e0 = ix.search(q, k, want_exact=True)
    assert torch.equal(i8, i0) and torch.equal(e8, e0) and torch.equal(s8, s0)
    assert_equal(s8, i8, e8, os_[:, :k], oi[:, :k], "search(sq8=True)")


# ---- grouped search -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_six_groups_led_by_members_of_one_cluster(gpu_device, n):
    """Six codes dealt at random: every group holds a dozen members of each cluster, so the best
    row of each of the 6 groups is a member of the query's cluster, and with group_size 2 so is
    the second.  Against the grouped oracle of tests/test_grouped_search_gpu.py."""
    from test_grouped_search_gpu import check_grouped
    dim, m, B = 384, 97, 3
    c16, q16, pos, _, _ = case(n, dim, B, m)
    c16, q16 = np.array(c16), np.array(q16)
    codes = np.random.default_rng(6).integers(0, 6, n).astype(np.int32)
    assert all(np.bincount(codes[p], minlength=6).min() >= 2 for p in pos)
    S = osearch.exact_scores(q16, c16)
    ix = make_index(c16, gpu_device)
    for s in (1, 2):
        es, ei = check_grouped(ix, q16, S, codes, 6, 6, s, gpu_device)
        assert all(np.isin(ei[b], pos[b]).all() for b in range(B))


# ---- MMR ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_mmr_over_a_cluster(gpu_device, n):
    """mmr = (64, 0.5): all 64 candidates are members of the cluster, the relevance term is the
    near-tied fp64 score; bit-equal to the numpy mirror fed the oracle's candidates."""
    import torch
    from test_mmr_search_gpu import mmr_oracle
    dim, m, B, k = 384, 97, 3, 10
    c16, q16, pos, _, oi = case(n, dim, B, m)
    c16, q16 = np.array(c16), np.array(q16)
    assert all(np.isin(oi[b], pos[b]).all() for b in range(B))
    want = mmr_oracle(osearch.exact_scores(q16, c16), c16, 64, k, 0.5)
    ix = make_index(c16, gpu_device)
    scores, ids, exact, flags = ix.search_raw(to_dev(q16, gpu_device), k, want_exact=True, mmr=(64, 0.5))
    torch.cuda.synchronize()
    assert int(flags.abs().sum()) == 0
    assert_equal(scores, ids, exact, *want)


# ---- cross-shard merge --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_cluster_split_over_two_shards(gpu_device, n):
    """As test_merge_shards_equals_single_index: two GpuIndex shards with id_base, rf_merge_shards;
    the shard boundary lies in the middle of every cluster."""
    import torch
    from rag_fin_amd.sharded import HipShardBackend
    dim, m, B, k = 384, 97, 3, 10
    c16, q16, pos, os_, oi = case(n, dim, B, m)
    c16 = np.array(c16)
    cut = int(pos[0][m // 2]) + 1
    assert all((p < cut).sum() >= 40 and (p >= cut).sum() >= 40 for p in pos)
    q = to_dev(q16, gpu_device)
    exact_all, ids_all = [], []
    for lo, hi in ((0, cut), (cut, n)):
        e, i, f = HipShardBackend(make_index(c16[lo:hi], gpu_device)).local_topk(q, k, lo)
        assert int(f.abs().sum()) == 0
        exact_all.append(e)
        ids_all.append(i)
    full = make_index(c16, gpu_device)
    scores, gids = HipShardBackend(full).merge(torch.stack(exact_all).contiguous(), torch.stack(ids_all).contiguous(), k)
    s1, i1, _, _ = full.search_raw(q, k, want_exact=True)
    assert torch.equal(gids, i1) and torch.equal(scores, s1)
    assert_equal(scores, gids, None, os_[:, :k], oi[:, :k])
    picked_from = (oi[:, :k] < cut).sum(axis=1)
    assert ((picked_from > 0) & (picked_from < k)).any()        # the answer really draws on both shards


# ---- mutation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_delete_the_best_and_ten_more_then_search_again(gpu_device, n):
    dim, m, B = 384, 97, 3
    c16, q16, pos, _, oi = case(n, dim, B, m)
    c16, q16 = np.array(c16), np.array(q16)
    gone = np.zeros(n, dtype=bool)
    for b in range(B):
        gone[oi[b, 0]] = True
        others = pos[b][pos[b] != oi[b, 0]]
        gone[others[3::9][:10]] = True
    assert gone.sum() == 11 * B
    keep = np.flatnonzero(~gone)
    ix = make_index(c16, gpu_device)
    ix.compact(keep)
    for k in (10, 64):
        check_against_oracle(ix, q16, np.ascontiguousarray(c16[keep]), k, gpu_device)
