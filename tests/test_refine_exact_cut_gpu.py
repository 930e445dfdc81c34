"""The refine stage's cut at the exact k-th score: k_shadow_refine rescores the k rows
behind the k largest lower bounds first (the winners), takes L2 = the smallest of their contract scores,
and keeps another candidate only if its upper bound reaches max(L, L2).  The answers stay those of the
fp16 chain and the C oracle, bit for bit; the lists the merge receives get about three times shorter.
Indexes are built as in tests/test_flat_shadow_gpu.py, with shadow=True."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import record_measurement
from oracle import adversarial as adv, c_oracle, search as osearch
from test_flat_shadow_gpu import make_index

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def unit_case(n, dim):
    """(corpus, 64 queries, oracle scores [64, 64], oracle ids [64, 64]); read-only, a top-k is a prefix."""
    c = osearch.synth_unit_rows(n, dim, 1401)
    q = osearch.synth_unit_rows(64, dim, 1402)
    os_, oi = c_oracle.search(q, c, 64)
    for a in (c, q, os_, oi):
        a.setflags(write=False)
    return c, q, os_, oi


# ---- equality ------------------------------------------------------------------------------------------
# every dim with every k; each size (8 200: the first past RF_SMALL_ROWS) and each batch three or four
# times.  k = 64 at dim 768: the winners' gather takes two stage passes of 32 rows.  k = 1: L2 is one score.
EQUALITY = [(8_200, 64, 1, 1), (20_011, 64, 33, 10), (60_000, 64, 64, 64),
            (20_011, 384, 64, 1), (60_000, 384, 1, 10), (8_200, 384, 33, 64),
            (60_000, 768, 33, 1), (8_200, 768, 64, 10), (20_011, 768, 1, 64), (20_011, 768, 64, 64)]


@pytest.mark.parametrize("n,dim,B,k", EQUALITY)
def test_equals_the_fp16_chain_and_the_oracle(gpu_device, n, dim, B, k):
    import torch
    c, q, os_, oi = unit_case(n, dim)
    ix = make_index(np.array(c), gpu_device)
    assert ix.shadow_first
    qd = torch.from_numpy(np.array(q[:B])).to(gpu_device)
    got = ix.search_raw(qd, k, want_exact=True)
    ref = ix.search_raw(qd, k, want_exact=True, fp16=True)
    torch.cuda.synchronize()
    print("flagged: shadow first", int((got[3] != 0).sum()), "fp16", int((ref[3] != 0).sum()), "of", B)
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    assert not got[3].any()
    s, i, e, _ = (x.cpu().numpy() for x in got)
    assert np.array_equal(i, oi[:B, :k])
    assert np.array_equal(e, os_[:B, :k])
    assert np.array_equal(s, os_[:B, :k].astype(np.float32))


# ---- ties at the cut -----------------------------------------------------------------------------------
def test_thirty_copies_of_the_query_rank_by_row(gpu_device):
    """One row at 30 ids in 30 different 32-row blocks, the query equal to it, k = 10: the ten winners'
    scores all equal L2, and 20 more rows tie it.  The ten lowest ids are the answer; a strict
    comparison in the cut, or a winner missing from the list, returns other rows."""
    import torch
    n, dim, k = 30_000, 384, 10
    c = osearch.synth_unit_rows(n, dim, 1411)
    copies = np.sort(np.random.default_rng(1413).choice(n // 32, 30, replace=False)) * 32 + np.arange(30) % 32
    assert len(set((copies // 32).tolist())) == 30
    c[copies] = c[copies[0]]
    q = osearch.synth_unit_rows(64, dim, 1412)
    q[0] = c[copies[0]]
    s, i, e, f = make_index(c, gpu_device).search_raw(torch.from_numpy(q).to(gpu_device), k, want_exact=True)
    torch.cuda.synchronize()
    s, i, e, f = (x.cpu().numpy() for x in (s, i, e, f))
    assert not f.any(), f
    assert i[0].tolist() == copies[:k].tolist()
    assert (e[0] == e[0, 0]).all() and (s[0] == s[0, 0]).all()
    os_, oi = c_oracle.search(q, c, k)
    assert np.array_equal(i, oi) and np.array_equal(e, os_) and np.array_equal(s, os_.astype(np.float32))


# ---- near ties ------------------------------------------------------------------------------------------
def test_near_tie_clusters_under_the_cut(gpu_device):
    """40 rows within an fp16 ulp or two of their query, k = 10: winners, L2 and the cut all fall inside
    the cluster, where the int8 scores cannot tell the rows apart."""
    import torch
    n, dim, k, m = 20_011, 384, 10, 40
    qs, cl = zip(*(adv.near_tie_cluster(dim, m, 1420 + j) for j in range(8)))
    c, pos = adv.embed_clusters(n, dim, 1421, cl, stride=adv.scatter_stride(n, 8 * m))
    q = np.concatenate([np.stack(qs), osearch.synth_unit_rows(56, dim, 1422)])
    os_, oi = c_oracle.search(q, c, k + 1)
    assert all(np.isin(oi[b], pos[b]).all() for b in range(8))     # ranks k and k + 1 lie in the cluster
    s, i, e, f = make_index(c, gpu_device).search_raw(torch.from_numpy(q).to(gpu_device), k, want_exact=True)
    torch.cuda.synchronize()
    s, i, e, f = (x.cpu().numpy() for x in (s, i, e, f))
    ok = f == 0
    print("unflagged:", int(ok.sum()), "of", len(ok), "| of the cluster queries:", int(ok[:8].sum()))
    assert np.array_equal(i[ok], oi[ok, :k])
    assert np.array_equal(e[ok], os_[ok, :k])
    assert np.array_equal(s[ok], os_[ok, :k].astype(np.float32))


# ---- the refined lists (experiments build, child process) ---------------------------------------------
_LIST_CHILD = r"""
import json
import numpy as np, torch
from oracle import c_oracle, search as osearch
from rag_fin_amd import _lib
from rag_fin_amd.store import GpuIndex
lib = _lib.load_library()
dev = torch.device("cuda:0")
n, d, b, k = 100_000, 384, 64, 10
c = osearch.synth_unit_rows(n, d, 1341)
q = osearch.synth_unit_rows(b, d, 1342)
ix = GpuIndex(d, n, dev, shadow=True)
ix.add(torch.from_numpy(c).to(dev))
qd = torch.from_numpy(q).to(dev)
_lib.check(lib.rf_set_tuning(b"fold_dbg", 2))    # the merge leaves the candidate counters
s, i, e, f = ix.search_raw(qd, k, want_exact=True)
torch.cuda.synchronize()
_lib.check(lib.rf_set_tuning(b"fold_dbg", 0))
ws = ix.workspace
def arr(name, count, dtype):
    off = lib.rf_debug_workspace_offset(name)
    return ws[off:off + count * 4].view(dtype).cpu().numpy()
cnt = arr(b"cand_cnt", 64 * 8, torch.int32).reshape(64, 8)
cand = arr(b"cand", 64 * 8 * 2048 * 2, torch.int32).reshape(64, 8, 2048, 2)
thr = arr(b"thr", 64, torch.float32)
eps = arr(b"eps", 64, torch.float32)
flat_bytes = lib.rf_search_workspace_bytes(None)
q8 = ws[flat_bytes:flat_bytes + b * d].view(torch.int8).view(b, d).cpu().numpy().astype(np.float64)
# the bound of sq8.h in fp64: beta_r = n_q e_r + f_q N' + 2^-18 ((n_q + f_q) N' + n_q E)
at, _ = ix.debug_scores_sq8(qd)
codes, sr, er = ix.get_rows_sq8(np.arange(n, dtype=np.int64))
torch.cuda.synchronize()
at, er32 = at.cpu().numpy(), er.cpu().numpy()
er = er32.astype(np.float64)
Np = float(np.sqrt(((codes.cpu().numpy().astype(np.float64) * sr.cpu().numpy().astype(np.float64)[:, None]) ** 2)
                   .sum(1)).max())
E = float(er.max())
q64 = q.astype(np.float64)
t = (np.abs(q.astype(np.float32)).max(1) / np.float32(127)).astype(np.float64)
nq = np.sqrt((q64 ** 2).sum(1))
fq = np.sqrt(((q64 - t[:, None] * q8) ** 2).sum(1))
slack = 2.0 ** -18 * ((nq + fq) * Np + nq * E)
emitted = at + nq.astype(np.float32)[:, None] * er32[None, :] >= thr[:b, None]   # the emit's test
exact = q64 @ c.astype(np.float64).T
_, oi = c_oracle.search(q, c, k)
fl = f.cpu().numpy()
missing, doubled, worst, lens, lo_cnt, hi_cnt = 0, 0, 0.0, [], [], []
for qi in range(b):
    ent = np.concatenate([cand[qi, sh, :min(cnt[qi, sh], 2048)] for sh in range(8)])
    rows, sc = ent[:, 0], ent[:, 1].copy().view(np.float32)
    lens.append(len(rows))
    doubled += len(rows) - len(set(rows.tolist()))
    missing += sum(1 for r in oi[qi].tolist() if r not in set(rows.tolist()))
    worst = max(worst, float((np.abs(sc.astype(np.float64) - exact[qi, rows]) / eps[qi]).max()))
    idx = np.flatnonzero(emitted[qi])
    a = at[qi, idx].astype(np.float64)
    beta = nq[qi] * er[idx] + fq[qi] * Np + slack[qi]
    lo, hi = a - beta, a + beta
    order = np.argsort(-lo, kind="stable")
    L = lo[order[k - 1]]
    L2 = exact[qi, idx[order[:k]]].min()
    cut = max(L, L2)
    lo_cnt.append(int((hi >= cut + 1e-6).sum()))
    hi_cnt.append(int((hi >= cut - 1e-6).sum()))
print("RESULT " + json.dumps(dict(flags=fl.tolist(), missing=missing, doubled=doubled, worst_err_over_eps=worst,
                                  lens=lens, lo_cnt=lo_cnt, hi_cnt=hi_cnt, emitted=emitted.sum(1).tolist())))
"""


def test_refined_lists_are_cut_at_the_exact_kth_score(gpu_device):
    """100 k x 384, B = 64, k = 10, the seeds of test_refined_lists_hold_the_topk_within_eps: the lists
    read back from the workspace.  Their lengths are those of the rule `upper bound >= max(L, L2)` formed
    in numpy from the int8 scores, e_r and the codes of the index and the quantized queries of the
    workspace; 1e-6 either way absorbs the kernel's directed fp32 roundings of the bounds (an fp32 ulp at
    these magnitudes is 3e-8).  The rule before this one left 87.09375 rows per query (136 at most,
    profiles/flat_shadow_measurements.jsonl); a numpy model of the new one gives 31.28 (60 at most)."""
    env = dict(os.environ, RAGFIN_LIB="exp")
    r = subprocess.run([sys.executable, "-c", _LIST_CHILD], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1][len("RESULT "):])
    lens, lo_cnt, hi_cnt = np.array(res["lens"]), np.array(res["lo_cnt"]), np.array(res["hi_cnt"])
    print("refined list: mean", lens.mean(), "max", lens.max(), "| rule: mean", lo_cnt.mean(), "..", hi_cnt.mean(),
          "| emitted: mean", np.mean(res["emitted"]), "| worst err / eps", res["worst_err_over_eps"])
    record_measurement("refine_exact_cut_list_100k_b64_k10", mean=lens.mean(), max=lens.max(),
                       rule_mean_low=lo_cnt.mean(), rule_mean_high=hi_cnt.mean(),
                       worst_err_over_eps=res["worst_err_over_eps"])
    assert not any(res["flags"])
    assert res["missing"] == 0 and res["doubled"] == 0
    # an fp64 dot rounded once to fp32, against eps = 1.25 dim 2^-23 |q| max|c|
    assert res["worst_err_over_eps"] <= 1.0 / (2.5 * 384), res["worst_err_over_eps"]
    assert (lo_cnt <= lens).all() and (lens <= hi_cnt).all(), (lens - lo_cnt, hi_cnt - lens)
    assert lens.mean() < 87.09375 / 2, lens.mean()
