"""The premises of tests/test_near_ties_gpu.py and tests/test_value_range_gpu.py, on the CPU: the
corpora of oracle/adversarial.py are what those tests take them for, so that a GPU pass means
something.

Near-tie clusters: the contract's float64 scores of a cluster are pairwise distinct (ties counted
and printed), they span less than one float32 spacing of the score, a float32 scoring sees fewer
distinct values than rows and orders them differently, and both oracles agree on the cluster.
Value range: the tiny corpus is mostly fp16 subnormals and flushing them changes the answer."""
import numpy as np
import pytest

from oracle import adversarial as adv, c_oracle, search as osearch

# (dim, rows of a cluster): the shapes the GPU tests use; 400 rows step two components per row
SHAPES = [(64, 33), (384, 97), (768, 97), (1024, 97), (384, 400)]
SEEDS = range(64)        # the GPU sweeps give each of up to 64 queries a cluster of its own (seed = query)


def rank(s):
    return np.lexsort((np.arange(s.size), -s))


@pytest.mark.parametrize("dim,m", SHAPES)
def test_cluster_premises(dim, m):
    ties = worst_spread = 0
    most_f32 = 0
    for seed in SEEDS:
        q, rows = adv.near_tie_cluster(dim, m, seed)
        assert rows.dtype == np.float16 and rows.shape == (m, dim) and np.array_equal(rows[0], q)
        diff = (rows.view(np.uint16) != q.view(np.uint16)[None, :]).sum(axis=1)
        n_small = adv.default_small(dim)
        assert diff[0] == 0 and (diff[1:n_small + 1] == 1).all() and (diff[n_small + 1:] == 2).all()
        assert len(np.unique(rows.view(np.uint16), axis=0)) == m          # no two rows are the same vector
        s = osearch.exact_scores(q[None, :], rows)[0]
        f = adv.f32_scores(q[None, :], rows)[0]
        ties += m - len(np.unique(s))
        spread = (s.max() - s.min()) / float(np.spacing(np.float32(s.min())))
        worst_spread = max(worst_spread, spread)
        # below ONE float32 spacing of the score (the issue allows two at dim 64; this generator needs one)
        assert spread < 1.0, (seed, spread)
        n_f32 = len(np.unique(f))
        most_f32 = max(most_f32, n_f32)
        assert n_f32 < m, (seed, n_f32)
        assert not np.array_equal(rank(s), rank(f)), seed
        # the same through a float32 rounding of the exact score: what a merge that ranked by the
        # fp32 output would see
        assert not np.array_equal(rank(s), rank(s.astype(np.float32).astype(np.float64))), seed
    print(f"dim {dim}, {m} rows, {len(SEEDS)} seeds: {ties} exact fp64 ties in all, worst spread {worst_spread:.3f} "
          f"float32 spacings, at most {most_f32} distinct float32 scores")
    # a tie is legal (the row id decides) but the clusters must be all but distinct
    assert ties <= len(SEEDS) * m // 50, ties


def test_clusters_are_deterministic_and_seeds_differ():
    a = adv.near_tie_cluster(384, 97, 5)
    b = adv.near_tie_cluster(384, 97, 5)
    c = adv.near_tie_cluster(384, 97, 6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])


@pytest.mark.parametrize("dim,m,k", [(64, 33, 64), (384, 97, 64), (1024, 97, 10)])
def test_both_oracles_agree_on_embedded_clusters(dim, m, k):
    qs, cl = zip(*(adv.near_tie_cluster(dim, m, seed) for seed in range(3)))
    q16 = np.stack(qs)
    c16, pos = adv.embed_clusters(3000, dim, 99, cl, stride=adv.scatter_stride(3000, 3 * m))
    assert len({int(p) // 32 for p in pos[0]}) > m // 2        # scattered over many 32-row blocks
    ps, pi = osearch.search(q16, c16, k)
    cs, ci = c_oracle.search(q16, c16, k)
    assert np.array_equal(pi, ci) and np.array_equal(ps, cs)
    for b in range(3):      # the cluster leads its query's ranking, in the order of its fp64 scores
        s = osearch.exact_scores(q16[b:b + 1], cl[b])[0]
        want = pos[b][rank(s)][:k]                              # positions ascend with the cluster row
        assert np.array_equal(pi[b, :min(k, m)], want[:min(k, m)])
        assert np.isin(pi[b, min(k, m):], pos[b], invert=True).all()


def test_scatter_crosses_blocks_and_partitions():
    for n, total in ((3000, 291), (3000, 2112), (20011, 6208), (20011, 400)):
        s = adv.scatter_stride(n, total)
        assert s % 32 != 0 and 5 + (total - 1) * s < n
    c16, pos = adv.embed_clusters(20011, 64, 1, [adv.near_tie_cluster(64, 33, 0)[1]] * 1, stride=211)
    assert len({int(p) % 32 for p in pos[0]}) > 16


# ---- the fp16 value range ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 384, 1024])
def test_tiny_corpus_is_mostly_subnormal_and_flushing_changes_the_answer(dim):
    c16, q16 = adv.value_range("tiny", 3000, dim, 16, 3)
    sc, sq = adv.subnormal_share(c16), adv.subnormal_share(q16)
    print(f"dim {dim}: subnormal share of the non-zero components: corpus {sc:.3f}, queries {sq:.3f}")
    assert sc >= 0.5 and sq >= 0.5
    _, want = osearch.search(q16, c16, 10)
    _, flushed = osearch.search(adv.flush_subnormals(q16), adv.flush_subnormals(c16), 10)
    changed = int((want != flushed).any(axis=1).sum())
    print(f"dim {dim}: flushing subnormals changes the top-10 of {changed} of 16 queries")
    assert changed >= 1


@pytest.mark.parametrize("kind", adv.KINDS)
def test_value_range_corpora_are_finite_and_what_they_claim(kind):
    for dim in (64, 384, 1024):
        c16, q16 = adv.value_range(kind, 3000, dim, 16, 3)
        assert c16.dtype == np.float16 and np.isfinite(c16).all() and np.isfinite(q16).all()
        S = osearch.exact_scores(q16, c16)
        cn = np.linalg.norm(c16.astype(np.float64), axis=1)
        qn = np.linalg.norm(q16.astype(np.float64), axis=1)
        assert (cn > 0).all() and (qn > 0).all()
        if kind == "huge":
            assert (np.abs(c16.astype(np.float32)) == 65504).any() and np.abs(S).max() > 1e10
        elif kind == "outlier":
            big = np.flatnonzero(cn > 2)
            assert big.tolist() == [3000 // 3] and 0.9 * 2 ** 13 < cn[big[0]] < 1.1 * 2 ** 13
        elif kind == "mixed":
            assert cn.max() / cn.min() > 2 ** 20 and qn.max() / qn.min() > 2 ** 8
        elif kind == "cancel":
            # scores sit near 0 on the scale of |q| |c|
            assert np.abs(S).max() < 0.05 * qn.min() * cn.min()
