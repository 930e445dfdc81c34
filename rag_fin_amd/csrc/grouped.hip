// Grouping search (include/ragfin.h, "grouping search"): the best n_groups groups of rows that
// share a dictionary code, each by its best group_size rows -- pymilvus' group_by_field.
//
// The plain chain's threshold sits at the k-th best ROW; a grouped answer reaches down to the
// best rows of the n-th best GROUP, so the threshold here is one per (query, group):
//
//   k_group_sweep<GMAX>   every block (every pass block of a filter) through the MFMA chain of the
//                         scan; per workgroup an LDS table gmax[code][query] of the fp32 scores,
//                         stored as one partition per workgroup (no global atomic)
//   k_group_threshold     per query and code: M_g (the group's maximum), m_{g,s} (the s-th largest
//                         partition maximum); groups that cannot be among the first n_groups get
//                         +inf, the others m_{g,s} - 2 eps
//   k_group_sweep<GEMIT>  the same sweep again; a row is appended when its score reaches the
//                         threshold of ITS group (LDS copy of the table)
//   k_merge_grouped       per query: R_g per group, fp64 chains, top s per group, groups by
//                         their best row
// Why the answer is exact: DESIGN.md 4.4d.
#include "rf_internal.h"
#include <algorithm>

#include "merge_common.h"
#include "scan_common.h"

enum { GMODE_MAX = 0, GMODE_EMIT = 1 };
#define GTAB (RF_GROUP_MAX_CODES * 64)   // entries of the per-workgroup (code, query) table

struct GroupParams {
  const uint4* corpus;   // tiled
  const _Float16* q;     // row-major [B, dim]
  int B;
  uint32_t n_rows;
  uint32_t n_work;       // blocks of the corpus (unfiltered sweep)
  const int32_t* codes;  // [n_rows]
  int n_codes;
  float* gpmax;          // GMAX: [P][64][n_codes]
  const float* gthr;     // GEMIT: [64][RF_GROUP_MAX_CODES]
  uint32_t* cand_cnt;    // [64][RF_CAND_SHARDS]
  uint2* cand;           // [64][RF_CAND_SHARDS][cap]
  uint32_t cap;
  // the masked sweep (FILTER): the filter's pass blocks, counted on the device
  const uint32_t* hdr;
  const uint32_t* mask;
  const uint32_t* blocks;
  uint32_t n_blocks;
};

// gmax[idx] = max(gmax[idx], x) on the order-preserving encoding; the LDS atomic is issued only
// on improvement (a plain read first).  A NaN stays out.
__device__ __forceinline__ void gmax_update(uint32_t* tab, uint32_t idx, float x) {
  if (x == x) {
    const uint32_t o = rf_f2ord(x);
    if (o > tab[idx]) atomicMax(&tab[idx], o);
  }
}

// What a block's scores do.  cv: the code of row row0 + (lane & 31), or -1 for a row without a
// group (past the end, rejected by the filter, code outside [0, n_codes)): such a row enters no
// maximum and is never appended, whatever the thresholds are (they may be -inf).
// A block whose 32 rows share one code takes the fast path: one table entry per query.
template <int JB, int MODE>
__device__ __forceinline__ void group_block(const f32x16 (&acc)[JB], int cv, uint32_t row0, int lane,
                                            uint32_t* tab, EmitState& es, const GroupParams& p) {
  const int h = lane >> 5;
  const int ql = lane & 31;
  const int c0 = __builtin_amdgcn_readfirstlane(cv);
  const bool uniform = __ballot(cv != c0) == 0ull;   // wave-uniform
  if (uniform && c0 < 0) return;                     // no row of the block has a group
  if (MODE == GMODE_MAX) {
    if (uniform) {
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) {
        float m = max16(acc[jb]);
        m = fmaxf(m, __shfl_xor(m, 32));
        if (lane < 32) gmax_update(tab, (uint32_t)c0 * 64u + jb * 32 + ql, m);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ci = __shfl(cv, (int)acc_row(i, h));
        if (ci >= 0) {
#pragma unroll
          for (int jb = 0; jb < JB; ++jb) gmax_update(tab, (uint32_t)ci * 64u + jb * 32 + ql, acc[jb][i]);
        }
      }
    }
  } else {
    const float* thr = (const float*)tab;
    uint32_t bits = 0u;
    if (uniform) {
      float th[JB];
      bool hit = false;
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) {
        th[jb] = thr[(uint32_t)c0 * 64u + jb * 32 + ql];
        hit |= max16(acc[jb]) >= th[jb];
      }
      if (__ballot(hit) == 0ull) return;
#pragma unroll
      for (int jb = 0; jb < JB; ++jb)
#pragma unroll
        for (int i = 0; i < 16; ++i) bits |= (acc[jb][i] >= th[jb]) ? (1u << (jb * 16 + i)) : 0u;
    } else {
      // mixed block: the threshold is looked up per row
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ci = __shfl(cv, (int)acc_row(i, h));
        const uint32_t at = (uint32_t)(ci < 0 ? 0 : ci) * 64u + ql;
#pragma unroll
        for (int jb = 0; jb < JB; ++jb)
          bits |= (ci >= 0 && acc[jb][i] >= thr[at + jb * 32]) ? (1u << (jb * 16 + i)) : 0u;
      }
    }
    if (__ballot(bits != 0u) != 0ull) emit_append<JB>(acc, bits, row0, lane, es, [&] { emit_flush(es, p, lane); });
  }
}

template <int KS, int R, int JB, int WAVES, int MODE, bool FILTER>
__global__ void __launch_bounds__(WAVES * 64) k_group_sweep(GroupParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32x4* smemQ = (u32x4*)smem_raw;                                                  // JB*KS*64 uint4
  uint32_t* tab = (uint32_t*)(smem_raw + (size_t)JB * KS * RF_FRAG_BYTES);          // [codes][64]
  uint32_t* stage = tab + GTAB;                                                     // GEMIT: 3 * WAVES * SCAP

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  EmitState es = emit_state(stage, wave, WAVES, SCAP);

  uint32_t n_work = p.n_work;
  if constexpr (FILTER) n_work = filter_pass_blocks(p.hdr, p.n_rows, p.n_blocks);
  const uint32_t W = gridDim.x * WAVES;
  const uint32_t gw = blockIdx.x * WAVES + wave;
  const uint32_t cnt = n_work > gw ? (n_work - gw + W - 1) / W : 0u;
  auto block_of = [&](uint32_t w) -> uint32_t {
    if constexpr (FILTER) {
      const uint32_t b = p.blocks[w];
      return b < p.n_blocks ? b : 0u;
    } else {
      return w;
    }
  };

  u32x4 ring[R];
  uint32_t b = 0u;
  if (cnt > 0) {
    b = block_of(gw);
    const uint4* src = p.corpus + (size_t)b * (KS * 64) + lane;
#pragma unroll
    for (int s = 0; s < R; ++s) ring[s] = ld_frag(src + s * 64);
  }
  stage_queries<KS, JB, WAVES>(smemQ, p.q, p.B);
  for (int idx = tid; idx < GTAB; idx += WAVES * 64) {
    // GMAX: 0 is below the encoding of every float; GEMIT: the (query, code) thresholds, transposed
    if (MODE == GMODE_MAX) tab[idx] = 0u;
    else ((float*)tab)[idx] = p.gthr[(size_t)(idx & 63) * RF_GROUP_MAX_CODES + (idx >> 6)];
  }
  __syncthreads();

  // the code of this lane's row of block `blk` (-1: no group), requested ahead of the MFMA chain
  auto code_of = [&](uint32_t blk) -> int {
    const uint32_t row = blk * 32u + (uint32_t)(lane & 31);
    int c = -1;
    if (row < p.n_rows) c = p.codes[row];
    if constexpr (FILTER) {
      if (((p.mask[blk] >> (lane & 31)) & 1u) == 0u) c = -1;
    }
    return (uint32_t)c < (uint32_t)p.n_codes ? c : -1;
  };

  if (cnt > 0) {
    uint32_t w = gw;
    f32x16 acc[JB];
    for (uint32_t i = 0; i + 1 < cnt; ++i, w += W) {
      const uint32_t bn = block_of(w + W);
      const int cv = code_of(b);
      const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
      const uint4* nxt = p.corpus + (size_t)bn * (KS * 64) + lane;
      mfma_block<KS, R, JB, false>(ring, cur, nxt, smemQ, lane, acc);
      group_block<JB, MODE>(acc, cv, b * 32u, lane, tab, es, p);
      b = bn;
    }
    {
      const int cv = code_of(b);
      const uint4* cur = p.corpus + (size_t)b * (KS * 64) + lane;
      mfma_block<KS, R, JB, true>(ring, cur, cur, smemQ, lane, acc);
      group_block<JB, MODE>(acc, cv, b * 32u, lane, tab, es, p);
    }
  }

  if (MODE == GMODE_EMIT) {
    if (es.cnt > 0) emit_flush(es, p, lane);
  } else {
    // this workgroup's partition: [64 queries][n_codes], contiguous
    __syncthreads();
    const int n = 64 * p.n_codes;
    float* out = p.gpmax + (size_t)blockIdx.x * n;
    for (int idx = tid; idx < n; idx += WAVES * 64) {
      const int qi = idx / p.n_codes, c = idx - qi * p.n_codes;
      const uint32_t o = tab[c * 64 + qi];
      out[idx] = o ? rf_ord2f(o) : -INFINITY;
    }
  }
}

// ---- per-(query, group) thresholds ------------------------------------------------------------
// One workgroup of four waves per query slot; wave w takes the codes g = w, w + 4, ...
// M_g = the maximum over the P partitions (the exact maximum MFMA score of the group: the sweep
// was complete), m_{g,s} = the s-th largest partition maximum (-inf with fewer than s finite ones).
// Then wave 0, one lane per code: M_(n) = the n-th largest M_g, and
//   thr[q][g] = +inf               if M_g < M_(n) - 2 eps   (g cannot be among the first n groups)
//             = m_{g,s} - 2 eps    otherwise.
// Query slots past B get +inf everywhere.  The candidate counters start at zero.
#define GTHR_V (RF_GROUP_PARTS / 64)
__global__ void __launch_bounds__(256) k_group_threshold(int B, int n_codes, int n_groups, int gsize,
                                                         const float* __restrict__ gpmax, int P,
                                                         const float* __restrict__ eps_in,
                                                         float* __restrict__ gthr,
                                                         uint32_t* __restrict__ cand_cnt) {
  __shared__ float sM[RF_GROUP_MAX_CODES], sm[RF_GROUP_MAX_CODES];
  const int qi = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  if (tid < RF_GROUP_MAX_CODES) sM[tid] = sm[tid] = -INFINITY;
  __syncthreads();
  if (qi < B) {
    for (int g = wave; g < n_codes; g += 4) {
      float v[GTHR_V];
#pragma unroll
      for (int i = 0; i < GTHR_V; ++i) {
        const int j = lane + 64 * i;
        v[i] = (j < P) ? gpmax[((size_t)j * 64 + qi) * n_codes + g] : -INFINITY;
      }
      float M = -INFINITY, kth = -INFINITY;
      for (int r = 0; r < gsize; ++r) {
        float m = v[0];
#pragma unroll
        for (int i = 1; i < GTHR_V; ++i) m = fmaxf(m, v[i]);
        const float wm = wave_max_xor(m);
        if (r == 0) M = wm;
        kth = wm;
        if (wm == -INFINITY) break;
        const unsigned long long who = __ballot(m == wm);
        const int winner = __ffsll((long long)who) - 1;
        if (lane == winner) {
          bool done = false;
#pragma unroll
          for (int i = 0; i < GTHR_V; ++i)
            if (!done && v[i] == wm) {
              v[i] = -INFINITY;
              done = true;
            }
        }
      }
      if (lane == 0) {
        sM[g] = M;
        sm[g] = kth;
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    float t = INFINITY;
    if (qi < B) {
      const float mine = lane < n_codes ? sM[lane] : -INFINITY;
      float x = mine, Mn = -INFINITY;
      for (int r = 0; r < n_groups; ++r) {
        const float wm = wave_max_xor(x);
        Mn = wm;
        if (wm == -INFINITY) break;
        const unsigned long long who = __ballot(x == wm);
        if (lane == __ffsll((long long)who) - 1) x = -INFINITY;
      }
      const float eps2 = 2.f * eps_in[qi];
      if (lane < n_codes && !(mine < Mn - eps2)) t = sm[lane] - eps2;
    }
    gthr[(size_t)qi * RF_GROUP_MAX_CODES + lane] = t;
    if (lane < RF_CAND_SHARDS) cand_cnt[qi * RF_CAND_SHARDS + lane] = 0u;
  }
}

// ---- grouped merge ------------------------------------------------------------------------------
// One workgroup per query:
//   1. gather the candidates with their codes into LDS;
//   2. per group, rank counting among the group's candidates by (MFMA score, row): the s-th
//      largest gives the cut  ã_(s) - 2 eps  (fewer than s candidates: no cut);
//   3. R = the candidates at or above their group's cut; fp64 chains of the contract for R;
//   4. per group the top s by (exact desc, row asc), groups ranked by their best row; slot
//      j * s + i receives row i of the group of rank j, everything else is padded.
#define GM_NONE 0xFFFFFFFFu

static size_t gmerge_lds_bytes(int dim) {
  return (size_t)RF_CAND_CAP * 8 + (size_t)MERGE_STAGE_ROWS * (dim * 2 + 16) + RF_RESCORE_CAP * 8 +
         RF_GROUP_MAX_CODES * 8 + (size_t)3 * RF_RESCORE_CAP * 4 + (size_t)4 * RF_GROUP_MAX_CODES * 4 + 16 +
         (size_t)dim * 2 + RF_CAND_CAP;
}

__global__ void __launch_bounds__(MERGE_THREADS) k_merge_grouped(
    const _Float16* __restrict__ q, int dim, int KS, const uint4* __restrict__ tiles,
    const int32_t* __restrict__ codes, int n_codes, int n_groups, int gsize, int64_t id_base,
    const uint32_t* __restrict__ cand_cnt, const uint2* __restrict__ cand, uint32_t cap,
    const float* __restrict__ eps_in, float* __restrict__ scores, int64_t* __restrict__ ids,
    double* __restrict__ exact, uint32_t* __restrict__ flags, uint32_t n_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int srow_stride = 2 * KS + 1;
  unsigned long long* skeys = (unsigned long long*)lds;                 // [RF_CAND_CAP]
  uint4* srows = (uint4*)(skeys + RF_CAND_CAP);                         // [32][2 KS + 1]
  double* r_exact = (double*)(srows + MERGE_STAGE_ROWS * srow_stride);     // [RESCORE_CAP]
  double* g_bs = r_exact + RF_RESCORE_CAP;                              // [codes] best fp64 score of the group
  uint32_t* r_row = (uint32_t*)(g_bs + RF_GROUP_MAX_CODES);             // [RESCORE_CAP]
  uint32_t* r_code = r_row + RF_RESCORE_CAP;
  uint32_t* r_in = r_code + RF_RESCORE_CAP;                             // rank inside the group
  float* g_cut = (float*)(r_in + RF_RESCORE_CAP);                       // [codes]
  uint32_t* g_br = (uint32_t*)(g_cut + RF_GROUP_MAX_CODES);             // [codes] row of the group's best
  uint32_t* g_rank = g_br + RF_GROUP_MAX_CODES;
  uint32_t* filled = g_rank + RF_GROUP_MAX_CODES;                       // [RF_MAX_K] output slots written
  uint32_t* r_cnt = filled + RF_GROUP_MAX_CODES;                        // 4 words
  _Float16* qh = (_Float16*)(r_cnt + 4);                                // [dim]
  unsigned char* scode = (unsigned char*)(qh + dim);                    // [RF_CAND_CAP]
  static_assert(RF_MAX_K <= RF_GROUP_MAX_CODES, "filled[] holds one word per output slot");

  const int qi = blockIdx.x;
  const int tid = threadIdx.x;
  const uint32_t s = (uint32_t)gsize;
  const int K = n_groups * gsize;
  bool bad_row = false;
  CandLists L;
  uint32_t fl = cand_lists(L, cand_cnt, cand, cap, qi);
  const uint32_t c = L.c;
  const float eps2 = 2.f * eps_in[qi];

  // ---- 1: gather -----------------------------------------------------------------------------
  for (uint32_t g = tid; g < c; g += MERGE_THREADS) {
    bool bad = false;
    const uint2 e = cand_at(L, g, n_rows, bad);
    const int code = bad ? -1 : codes[e.x];   // a bad row has no group: it takes part in nothing
    bad_row |= bad;
    skeys[g] = cand_key(e);
    scode[g] = (uint32_t)code < (uint32_t)n_codes ? (unsigned char)code : (unsigned char)0xFF;
  }
  if (tid < RF_GROUP_MAX_CODES) {
    g_cut[tid] = -INFINITY;
    g_br[tid] = GM_NONE;
    g_rank[tid] = GM_NONE;
    filled[tid] = 0u;
  }
  if (tid == 0) *r_cnt = 0u;
  for (int d = tid; d < dim; d += MERGE_THREADS) qh[d] = q[(size_t)qi * dim + d];
  __syncthreads();

  // ---- 2: the s-th largest candidate of every group --------------------------------------------
  for (uint32_t g = tid; g < c; g += MERGE_THREADS) {
    const unsigned long long key = skeys[g];
    const unsigned char code = scode[g];
    if (code == 0xFF) continue;
    uint32_t rank = 0u;
    for (uint32_t j = 0; j < c; ++j) rank += (scode[j] == code && skeys[j] > key) ? 1u : 0u;
    if (rank == s - 1u) g_cut[code] = key_score(key) - eps2;   // one candidate per group has this rank
  }
  __syncthreads();
  // ---- 3: R, then the fp64 chains ----------------------------------------------------------------
  for (uint32_t g = tid; g < c; g += MERGE_THREADS) {
    const unsigned long long key = skeys[g];
    const unsigned char code = scode[g];
    if (code == 0xFF) continue;
    if (key_score(key) >= g_cut[code]) {
      const uint32_t slot = atomicAdd(r_cnt, 1u);
      if (slot < RF_RESCORE_CAP) {
        r_row[slot] = key_row(key);
        r_code[slot] = code;
      }
    }
  }
  __syncthreads();
  uint32_t R = *r_cnt;
  if (R > RF_RESCORE_CAP) {
    fl |= RF_FLAG_TIE_OVERFLOW;
    R = RF_RESCORE_CAP;
  }
  rescore_rows(r_row, R, tiles, KS, qh, srows, r_exact);

  // ---- 4: top s per group, groups by their best row ----------------------------------------------
  for (uint32_t i = tid; i < R; i += MERGE_THREADS) {
    const double si = r_exact[i];
    const uint32_t ri = r_row[i], ci = r_code[i];
    uint32_t rank = 0u;
    for (uint32_t j = 0; j < R; ++j) rank += (r_code[j] == ci && ranks_before(r_exact[j], r_row[j], si, ri)) ? 1u : 0u;
    r_in[i] = rank;
    if (rank == 0u) {
      g_bs[ci] = si;
      g_br[ci] = ri;
    }
  }
  __syncthreads();
  if (tid < RF_GROUP_MAX_CODES && g_br[tid] != GM_NONE) {
    uint32_t rank = 0u;
    for (int g = 0; g < RF_GROUP_MAX_CODES; ++g)
      rank += (g_br[g] != GM_NONE && ranks_before(g_bs[g], g_br[g], g_bs[tid], g_br[tid])) ? 1u : 0u;
    g_rank[tid] = rank;
  }
  __syncthreads();
  for (uint32_t i = tid; i < R; i += MERGE_THREADS) {
    const uint32_t gr = g_rank[r_code[i]];
    if (r_in[i] < s && gr < (uint32_t)n_groups) {
      const uint32_t slot = gr * s + r_in[i];
      const size_t o = (size_t)qi * K + slot;
      const double si = r_exact[i];
      scores[o] = (float)si;
      ids[o] = (int64_t)r_row[i] + id_base;
      if (exact) exact[o] = si;
      filled[slot] = 1u;
    }
  }
  __syncthreads();
  for (int j = tid; j < K; j += MERGE_THREADS) {
    if (filled[j]) continue;
    const size_t o = (size_t)qi * K + j;
    scores[o] = -INFINITY;
    ids[o] = -1;
    if (exact) exact[o] = -INFINITY;
  }
  if (flags && __syncthreads_or(bad_row ? 1 : 0)) fl |= RF_FLAG_CAND_OVERFLOW;
  if (tid == 0 && flags) flags[qi] = fl;
  // (the candidate counters stay: k_group_threshold / k_threshold zero them at the start of every
  // search, and a test reads them after a grouped search -- rf_debug_grouped_counters_offset)
}

// ---- host side --------------------------------------------------------------------------------------
template <int KS, int R, int JB, int WAVES, int MODE, bool FILTER>
static int launch_group_sweep(const GroupParams& p, int grid, hipStream_t st) {
  size_t lds = (size_t)JB * KS * RF_FRAG_BYTES + (size_t)GTAB * 4 + (size_t)3 * WAVES * SCAP * 4;
  auto kern = k_group_sweep<KS, R, JB, WAVES, MODE, FILTER>;
  static rf_lds_attr attr;  // per instantiation, per device
  RF_HIP(rf_ensure_lds(attr, (const void*)kern, lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVES * 64), lds, st, p);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

template <int KS, int R, int WAVES, int MODE>
static int launch_group_sweep_jf(int JB, bool filtered, const GroupParams& p, int grid, hipStream_t st) {
  if (filtered)
    return JB == 1 ? launch_group_sweep<KS, R, 1, WAVES, MODE, true>(p, grid, st)
                   : launch_group_sweep<KS, R, 2, WAVES, MODE, true>(p, grid, st);
  return JB == 1 ? launch_group_sweep<KS, R, 1, WAVES, MODE, false>(p, grid, st)
                 : launch_group_sweep<KS, R, 2, WAVES, MODE, false>(p, grid, st);
}

template <int MODE>
static int dispatch_group_sweep(int KS, int JB, bool filtered, const GroupParams& p, int grid, hipStream_t st) {
  // ring depth: the whole block up to dim 256, eight fragments beyond (the emit sweep's depth at dim 384)
  switch (KS) {
    case 4: return launch_group_sweep_jf<4, 4, 4, MODE>(JB, filtered, p, grid, st);
    case 8: return launch_group_sweep_jf<8, 8, 4, MODE>(JB, filtered, p, grid, st);
    case 16: return launch_group_sweep_jf<16, 16, 4, MODE>(JB, filtered, p, grid, st);
    case 24: return launch_group_sweep_jf<24, 8, 4, MODE>(JB, filtered, p, grid, st);
    case 32: return launch_group_sweep_jf<32, 8, 4, MODE>(JB, filtered, p, grid, st);
    case 48: return launch_group_sweep_jf<48, 8, 8, MODE>(JB, filtered, p, grid, st);
    case 64: return launch_group_sweep_jf<64, 8, 8, MODE>(JB, filtered, p, grid, st);
    default: break;
  }
  rf_set_error("no grouped scan kernel for dim %d", KS * 16);
  return RF_ERR_UNSUPPORTED;
}

static GroupParams group_params(const rf_index* ix, const void* q, int B, const rf_group& g,
                                const rf_workspace& ws, const rf_grouped_ws& gws, const rf_filter_view* filt) {
  GroupParams p{};
  p.corpus = ix->tiles;
  p.q = (const _Float16*)q;
  p.B = B;
  p.n_rows = (uint32_t)ix->size;
  p.n_work = (uint32_t)((ix->size + 31) / 32);
  p.codes = g.codes;
  p.n_codes = g.n_codes;
  p.gpmax = gws.gpmax;
  p.gthr = gws.gthr;
  p.cand_cnt = ws.cand_cnt;
  p.cand = ws.cand;
  p.cap = RF_SHARD_CAP;
  if (filt) {
    p.hdr = filt->hdr;
    p.mask = filt->mask;
    p.blocks = filt->blocks;
    p.n_blocks = p.n_work;
  }
  return p;
}

int rf_launch_group_max(const rf_index* ix, const void* q, int B, int JB, const rf_group& g,
                        const rf_workspace& ws, const rf_grouped_ws& gws, int* P_out, hipStream_t st,
                        const rf_filter_view* filt) {
  // one partition per workgroup: the emit grid of the dim (no knob), at most RF_GROUP_PARTS
  const int grid = std::min(rf_emit_grid(ix, 0), RF_GROUP_PARTS);
  *P_out = grid;
  return dispatch_group_sweep<GMODE_MAX>(ix->KS, JB, filt != nullptr, group_params(ix, q, B, g, ws, gws, filt), grid, st);
}

int rf_launch_group_threshold(int B, const rf_group& g, int P, const rf_workspace& ws,
                              const rf_grouped_ws& gws, hipStream_t st) {
  hipLaunchKernelGGL(k_group_threshold, dim3(RF_QCHUNK), dim3(256), 0, st, B, g.n_codes, g.n_groups, g.group_size,
                     gws.gpmax, P, ws.eps, gws.gthr, ws.cand_cnt);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_group_emit(const rf_index* ix, const void* q, int B, int JB, const rf_group& g,
                         const rf_workspace& ws, const rf_grouped_ws& gws, hipStream_t st,
                         const rf_filter_view* filt) {
  return dispatch_group_sweep<GMODE_EMIT>(ix->KS, JB, filt != nullptr, group_params(ix, q, B, g, ws, gws, filt),
                                          std::min(rf_emit_grid(ix, 0), RF_GROUP_PARTS), st);
}

int rf_launch_merge_grouped(const rf_index* ix, const void* q, int B, const rf_group& g, int64_t id_base,
                            const rf_workspace& ws, float* scores, int64_t* ids, double* exact,
                            uint32_t* flags, hipStream_t st) {
  const size_t lds = gmerge_lds_bytes(ix->dim);
  static rf_lds_attr attr;
  RF_HIP(rf_ensure_lds(attr, (const void*)k_merge_grouped, lds));
  hipLaunchKernelGGL(k_merge_grouped, dim3(B), dim3(MERGE_THREADS), lds, st, (const _Float16*)q, ix->dim, ix->KS,
                     ix->tiles, g.codes, g.n_codes, g.n_groups, g.group_size, id_base, ws.cand_cnt, ws.cand,
                     (uint32_t)RF_SHARD_CAP, ws.eps, scores, ids, exact, flags, (uint32_t)ix->size);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
