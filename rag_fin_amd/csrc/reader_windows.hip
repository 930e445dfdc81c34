// Extractive reader over sliding windows: ONE decode per context from the logits of its overlapping windows
// (include/ragfin.h, rf_stitch_spans).  The windows are pair rows of rf_answer_spans, which wrote their logits;
// here every context token takes its logits from the window in which it has the most context, and the spans,
// the null slot and the two log-sum-exps are taken over the stitched sequence.  k_qa_spans holds one pair of
// <= 512 positions in one workgroup; a stitched context has up to 65 536 tokens, so the work is cut into tiles
// of 512 tokens (= candidate starts), one workgroup each, over three launches:
//   k_stitch_gather   tile: owner of each token (max context), S / E into the workspace, the tile's two maxima
//   k_stitch_tiles    tile: one start per thread, 512 + 63 ends in LDS; k_qa_spans' selection rounds write the
//                     tile's best n_best; the tile's fp64 sums of exp(S - max of the context), exp(E - max)
//   k_stitch_merge    context: the best n_best of the tiles' lists (each list is sorted and holds every member of
//                     the context's best n_best that starts in its tile), the sums added in ascending tile order
// A tile is addressed by a SLOT g in [0, W): context c owns the slots ctx_win[c] .. ctx_win[c + 1], one per
// window, and uses the first ceil(L / 512) of them -- a window holds at most T <= 512 tokens, so a context never
// has more tiles than windows.  The same bound places S / E: context c's tokens start at 512 * ctx_win[c].  The
// grids are W, W and C workgroups whatever the contexts' lengths, which the host does not know.
// No atomics.  Every reduction is either the maximum of a strict total order or an fp64 sum in a written order,
// and every number is a function of the context's own windows: the same context gives the same bits anywhere.
#include "reader_internal.h"

#define RW_THREADS RD_THREADS
#define RW_WAVES RD_WAVES
#define RW_TILE 512                                   // tokens (candidate starts) per tile
#define RW_HALO (RF_READER_MAX_SPAN - 1)              // ends beyond the tile a span starting in it can reach
#define RW_MAX_TILES (RF_READER_MAX_CONTEXT / RW_TILE)
static_assert(RW_TILE == RW_THREADS && RW_MAX_TILES <= RW_THREADS && RF_READER_MAX_SPAN == 64,
              "one thread per start, one thread per tile in the merge, 6 key bits for the span length");

struct rw_ctx {
  int w0, nwin;     // the context's rows of win / logits, clamped to [0, W]
  int L;            // its tokens, clamped to 512 * nwin and RF_READER_MAX_CONTEXT
  int null_w;       // the null slot's window, or RD_NONE
  float s0, e0;     // that window's logits at position 0
};

// A window with every field in range: first in [0, MAX_CONTEXT], count and seg in [0, T].
__device__ __forceinline__ rf_window rw_window(const rf_window* __restrict__ win, int w, int T) {
  rf_window v = win[w];
  v.first = min(max(v.first, 0), RF_READER_MAX_CONTEXT);
  v.count = min(max(v.count, 0), T);
  v.seg = min(max(v.seg, 0), T);
  return v;
}

// The context of slot g: the largest c in [0, C) with ctx_win[c] <= g (ctx_win[0] = 0).
__device__ __forceinline__ int rw_slot_context(const int32_t* __restrict__ ctx_win, int C, int g) {
  int lo = 0, hi = C;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ctx_win[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// What every launch needs of context c, by the whole workgroup: L = max(first + count) and the null slot, the
// minimum of the strict total order (s_w[0] + e_w[0], w).  Every thread returns the same values.
__device__ __forceinline__ rw_ctx rw_context(const float* __restrict__ logits, int W, int T,
                                             const rf_window* __restrict__ win, const int32_t* __restrict__ ctx_win,
                                             int c) {
  __shared__ int red_l[RW_WAVES], red_w[RW_WAVES];
  __shared__ float red_z[RW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  rw_ctx x;
  x.w0 = min(max(ctx_win[c], 0), W);
  const int w1 = min(max(ctx_win[c + 1], x.w0), W);
  x.nwin = w1 - x.w0;
  int l = 0, bw = RD_NONE;
  float bz = INFINITY;
  for (int w = x.w0 + tid; w < w1; w += RW_THREADS) {
    const rf_window v = rw_window(win, w, T);
    l = max(l, v.first + v.count);
    const float z = logits[(size_t)w * T * 2] + logits[(size_t)w * T * 2 + 1];
    if (z < bz || (z == bz && w < bw)) {
      bz = z;
      bw = w;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    l = max(l, __shfl_xor(l, o));
    const float zo = __shfl_xor(bz, o);
    const int wo = __shfl_xor(bw, o);
    if (zo < bz || (zo == bz && wo < bw)) {
      bz = zo;
      bw = wo;
    }
  }
  if (lane == 0) {
    red_l[wave] = l;
    red_z[wave] = bz;
    red_w[wave] = bw;
  }
  __syncthreads();
  l = red_l[0];
  bz = red_z[0];
  bw = red_w[0];
#pragma unroll
  for (int w = 1; w < RW_WAVES; ++w) {
    l = max(l, red_l[w]);
    if (red_z[w] < bz || (red_z[w] == bz && red_w[w] < bw)) {
      bz = red_z[w];
      bw = red_w[w];
    }
  }
  x.L = min(l, min(x.nwin, RW_MAX_TILES) * RW_TILE);
  x.null_w = bw;
  x.s0 = bw != RD_NONE ? logits[(size_t)bw * T * 2] : -INFINITY;
  x.e0 = bw != RD_NONE ? logits[(size_t)bw * T * 2 + 1] : -INFINITY;
  return x;
}

// max of (a, b) over the workgroup, in every thread; red: [2][RW_WAVES]
__device__ __forceinline__ void rw_block_max(float& a, float& b, float (*red)[RW_WAVES]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    a = fmaxf(a, __shfl_xor(a, o));
    b = fmaxf(b, __shfl_xor(b, o));
  }
  if (lane == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
  }
  __syncthreads();
  a = red[0][0];
  b = red[1][0];
#pragma unroll
  for (int w = 1; w < RW_WAVES; ++w) {
    a = fmaxf(a, red[0][w]);
    b = fmaxf(b, red[1][w]);
  }
}

// One selection round's maximum of (z, k) by rd_better over the workgroup, in every thread: k_qa_spans' round.
// Two buffers by the round's parity: a round's writes cannot meet the reads of the round before last, which
// every thread left before the barrier of the round between.
__device__ __forceinline__ void rw_block_best(float& z, int& k, int r, float (*red_z)[RW_WAVES], int (*red_k)[RW_WAVES]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const float zo = __shfl_xor(z, o);
    const int ko = __shfl_xor(k, o);
    if (rd_better(zo, ko, z, k)) {
      z = zo;
      k = ko;
    }
  }
  if (lane == 0) {
    red_z[r & 1][wave] = z;
    red_k[r & 1][wave] = k;
  }
  __syncthreads();
  z = red_z[r & 1][0];
  k = red_k[r & 1][0];
#pragma unroll
  for (int w = 1; w < RW_WAVES; ++w) {
    const float zo = red_z[r & 1][w];
    const int ko = red_k[r & 1][w];
    if (rd_better(zo, ko, z, k)) {
      z = zo;
      k = ko;
    }
  }
}

// The first w in [lo, hi) whose window starts at `first` or later (the windows ascend in first), or hi.
__device__ __forceinline__ int rw_lower_bound(const rf_window* __restrict__ win, int lo, int hi, int first) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (win[mid].first < first) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(RW_THREADS) k_stitch_gather(
    const float* __restrict__ logits, int W, int T, const rf_window* __restrict__ win,
    const int32_t* __restrict__ ctx_win, int C, float* __restrict__ S, float* __restrict__ E,
    float* __restrict__ tmax) {
  __shared__ float red[2][RW_WAVES];
  const int tid = threadIdx.x, g = blockIdx.x;
  const int c = rw_slot_context(ctx_win, C, g);
  const rw_ctx x = rw_context(logits, W, T, win, ctx_win, c);
  const int t = g - x.w0;
  if (t < 0 || (long long)t * RW_TILE >= x.L) return;        // workgroup-uniform: not a tile of this context
  const int tile0 = t * RW_TILE, tk = tile0 + tid;
  // a window holding a token of this tile starts in (tile0 - T, tile0 + 512): one range for the workgroup
  const int wa = rw_lower_bound(win, x.w0, x.w0 + x.nwin, tile0 - T + 1);
  const int wb = rw_lower_bound(win, wa, x.w0 + x.nwin, tile0 + RW_TILE);
  float sv = -INFINITY, ev = -INFINITY;
  if (tk < x.L) {
    int best = -1, own = -1;
    for (int w = wa; w < wb; ++w) {                          // (every lane reads the same window: broadcast loads)
      const rf_window v = rw_window(win, w, T);
      const int d = tk - v.first;
      if (d >= 0 && d < v.count) {
        const int m = min(d, v.count - 1 - d);
        if (m > best) {                                      // w ascends: among equal margins the smallest w stays
          best = m;
          own = w;
        }
      }
    }
    if (own >= 0) {                                          // (a token in no window -- malformed -- stays -inf)
      const rf_window v = rw_window(win, own, T);
      const int p = min(v.seg + (tk - v.first), T - 1);
      const float* l = logits + ((size_t)own * T + p) * 2;
      sv = l[0];
      ev = l[1];
    }
    S[(size_t)x.w0 * RW_TILE + tk] = sv;                     // tk < L <= 512 * nwin: inside the context's slots
    E[(size_t)x.w0 * RW_TILE + tk] = ev;
  }
  rw_block_max(sv, ev, red);
  if (tid == 0) {
    tmax[(size_t)g * 2] = sv;
    tmax[(size_t)g * 2 + 1] = ev;
  }
}

// The exact maxima of the context's S and E together with the null slot's s[0], e[0], in every thread.
__device__ __forceinline__ void rw_context_max(const rw_ctx& x, const float* __restrict__ tmax, float (*red)[RW_WAVES],
                                               float* ms, float* me) {
  const int tid = threadIdx.x, live = (x.L + RW_TILE - 1) / RW_TILE;   // <= RW_MAX_TILES <= RW_THREADS
  float a = tid < live ? tmax[(size_t)(x.w0 + tid) * 2] : -INFINITY;
  float b = tid < live ? tmax[(size_t)(x.w0 + tid) * 2 + 1] : -INFINITY;
  if (tid == 0) {
    a = fmaxf(a, x.s0);
    b = fmaxf(b, x.e0);
  }
  rw_block_max(a, b, red);
  *ms = a;
  *me = b;
}

__global__ void __launch_bounds__(RW_THREADS) k_stitch_tiles(
    const float* __restrict__ logits, int W, int T, const rf_window* __restrict__ win,
    const int32_t* __restrict__ ctx_win, int C, const float* __restrict__ S, const float* __restrict__ E,
    const float* __restrict__ tmax, int max_len, int n_best, rf_span* __restrict__ tbest, double* __restrict__ tsum) {
  __shared__ float el[RW_TILE + RW_HALO + 1];
  __shared__ float red_m[2][RW_WAVES], red_z[2][RW_WAVES];
  __shared__ double red_d[2][RW_WAVES];
  __shared__ int red_k[2][RW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = blockIdx.x;
  const int c = rw_slot_context(ctx_win, C, g);
  const rw_ctx x = rw_context(logits, W, T, win, ctx_win, c);
  const int t = g - x.w0;
  // tile 0 of a context with windows runs even when L == 0: the merge reads its (empty) list and (zero) sums
  if (t < 0 || t >= x.nwin || (t > 0 && (long long)t * RW_TILE >= x.L)) return;   // workgroup-uniform
  const int tile0 = t * RW_TILE, tk = tile0 + tid;
  S += (size_t)x.w0 * RW_TILE;
  E += (size_t)x.w0 * RW_TILE;
  const float sv = tk < x.L ? S[tk] : -INFINITY, ev = tk < x.L ? E[tk] : -INFINITY;
  el[tid] = ev;
  if (tid <= RW_HALO) el[RW_TILE + tid] = tk + RW_TILE < x.L ? E[tk + RW_TILE] : -INFINITY;

  // ---- the tile's share of the two sums: exp(v - the CONTEXT's maximum) in fp64, the xor-shuffle tree of a
  // wave, the 8 wave sums ascending ----
  float ms, me;
  rw_context_max(x, tmax, red_m, &ms, &me);                  // (its barrier also completes el)
  double ds = tk < x.L ? exp((double)sv - (double)ms) : 0.0;
  double de = tk < x.L ? exp((double)ev - (double)me) : 0.0;
  for (int o = 32; o > 0; o >>= 1) {
    ds += __shfl_xor(ds, o);
    de += __shfl_xor(de, o);
  }
  if (lane == 0) {
    red_d[0][wave] = ds;
    red_d[1][wave] = de;
  }
  __syncthreads();
  if (tid == 0) {
    double ts = red_d[0][0], te = red_d[1][0];
#pragma unroll
    for (int w = 1; w < RW_WAVES; ++w) {
      ts += red_d[0][w];
      te += red_d[1][w];
    }
    tsum[(size_t)g * 2] = ts;
    tsum[(size_t)g * 2 + 1] = te;
  }

  // ---- the tile's best n_best: thread = candidate start tile0 + tid, holding the best span it has not given
  // yet.  Positions and keys are local to the tile (start tid, ends up to 512 + 62 in el); within one tile the
  // local key orders candidates as the context-wide key (i << 6) | (j - i) does ----
  rf_span* out = tbest + (size_t)g * RF_READER_MAX_BEST;
  const bool starts = tk < x.L;
  const int jmax = min(tid + max_len - 1, x.L - 1 - tile0);
  const float si = starts ? sv : 0.f;
  float bz = -INFINITY;
  int bk = starts ? rd_next(el, si, tid, jmax, INFINITY, -1, &bz) : RD_NONE;
  int r = 0;
  for (; r < n_best; ++r) {
    float z = bz;
    int k = bk;
    rw_block_best(z, k, r, red_z, red_k);
    if (k == RD_NONE) break;                                 // workgroup-uniform
    const int wi = k >> 6, wj = wi + (k & 63);
    if (tid == 0) out[r] = rf_span{tile0 + wi, tile0 + wj, z};
    if (wi == tid) bk = rd_next(el, si, tid, jmax, z, wj, &bz);   // the winner's owner moves on
  }
  if (tid >= r && tid < n_best) out[tid] = rf_span{-1, -1, -INFINITY};
}

__global__ void __launch_bounds__(RW_THREADS) k_stitch_merge(
    const float* __restrict__ logits, int W, int T, const rf_window* __restrict__ win,
    const int32_t* __restrict__ ctx_win, const float* __restrict__ tmax, const rf_span* __restrict__ tbest,
    const double* __restrict__ tsum, int n_best, rf_span* __restrict__ spans, float* __restrict__ norm) {
  __shared__ float red_m[2][RW_WAVES], red_z[2][RW_WAVES];
  __shared__ int red_k[2][RW_WAVES];
  const int tid = threadIdx.x, c = blockIdx.x;
  const rw_ctx x = rw_context(logits, W, T, win, ctx_win, c);
  const int live = x.nwin == 0 ? 0 : max(1, (x.L + RW_TILE - 1) / RW_TILE);   // the lists k_stitch_tiles wrote
  float ms, me;
  rw_context_max(x, tmax, red_m, &ms, &me);

  // ---- the normalisers: the null term, then the tiles' sums in ascending tile order (a context without
  // windows has neither: log(0) = -inf) ----
  if (tid == 0) {
    const bool has_null = x.null_w != RD_NONE;
    double ts = has_null ? exp((double)x.s0 - (double)ms) : 0.0;
    double te = has_null ? exp((double)x.e0 - (double)me) : 0.0;
    for (int t = 0; t < live; ++t) {
      ts += tsum[(size_t)(x.w0 + t) * 2];
      te += tsum[(size_t)(x.w0 + t) * 2 + 1];
    }
    norm[(size_t)c * 3 + 0] = has_null ? x.s0 + x.e0 : -INFINITY;
    norm[(size_t)c * 3 + 1] = (float)((double)ms + log(ts));
    norm[(size_t)c * 3 + 2] = (float)((double)me + log(te));
  }

  // ---- the best n_best of the union of the tiles' lists: thread = tile, holding the head of its sorted list ----
  rf_span* out = spans + (size_t)c * n_best;
  const rf_span* mine = tbest + (size_t)(x.w0 + tid) * RF_READER_MAX_BEST;
  int pos = 0;
  float bz = -INFINITY;
  int bk = RD_NONE;
  if (tid < live) {
    const rf_span h = mine[0];
    if (h.start >= 0) {
      bz = h.z;
      bk = (h.start << 6) | (h.end - h.start);
    }
  }
  int r = 0;
  for (; r < n_best; ++r) {
    float z = bz;
    int k = bk;
    rw_block_best(z, k, r, red_z, red_k);
    if (k == RD_NONE) break;                                 // workgroup-uniform
    const int wi = k >> 6;
    if (tid == 0) out[r] = rf_span{wi, wi + (k & 63), z};
    if (wi / RW_TILE == tid && bk == k) {                    // the winner's tile moves on
      bz = -INFINITY;
      bk = RD_NONE;
      if (++pos < n_best) {
        const rf_span h = mine[pos];
        if (h.start >= 0) {
          bz = h.z;
          bk = (h.start << 6) | (h.end - h.start);
        }
      }
    }
  }
  if (tid >= r && tid < n_best) out[tid] = rf_span{-1, -1, -INFINITY};
}

// ---- host --------------------------------------------------------------------------------------------------------
struct rw_layout {
  size_t S, E, tmax, tsum, tbest, total;
};

static rw_layout rw_plan(int W) {
  auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
  const size_t slots = (size_t)(W > 0 ? W : 1);
  rw_layout p;
  p.S = 0;
  p.E = p.S + up(slots * RW_TILE * sizeof(float));
  p.tsum = p.E + up(slots * RW_TILE * sizeof(float));
  p.tmax = p.tsum + up(slots * 2 * sizeof(double));
  p.tbest = p.tmax + up(slots * 2 * sizeof(float));
  p.total = p.tbest + up(slots * RF_READER_MAX_BEST * sizeof(rf_span));
  return p;
}

extern "C" size_t rf_stitch_workspace_bytes(int W, int C, int max_context_tokens) {
  if (W < 0 || C < 1 || max_context_tokens < 0 || max_context_tokens > RF_READER_MAX_CONTEXT) return 0;
  return rw_plan(W).total;
}

extern "C" int rf_stitch_spans(const float* logits_dev, int W, int T, const rf_window* win_dev,
                               const int32_t* ctx_win_dev, int C, int max_answer_len, int n_best, rf_span* spans_dev,
                               float* norm_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!logits_dev || !win_dev || !ctx_win_dev || !spans_dev || !norm_dev || !workspace_dev) {
    rf_set_error("rf_stitch_spans: null argument");
    return RF_ERR_INVALID;
  }
  if (n_best < 1 || n_best > RF_READER_MAX_BEST || max_answer_len < 1 || max_answer_len > RF_READER_MAX_SPAN) {
    rf_set_error("rf_stitch_spans: n_best=%d (1..%d) or max_answer_len=%d (1..%d) out of range", n_best,
                 RF_READER_MAX_BEST, max_answer_len, RF_READER_MAX_SPAN);
    return RF_ERR_INVALID;
  }
  if (W < 0 || C < 1 || T < 1) {
    rf_set_error("rf_stitch_spans: W=%d (>= 0), C=%d (>= 1) or T=%d (>= 1) out of range", W, C, T);
    return RF_ERR_INVALID;
  }
  if (T > RD_THREADS) {
    rf_set_error("rf_stitch_spans: T=%d exceeds the %d positions of a pair row", T, RD_THREADS);
    return RF_ERR_UNSUPPORTED;
  }
  const rw_layout p = rw_plan(W);
  if (workspace_bytes < p.total || ((uintptr_t)workspace_dev & 15)) {
    rf_set_error("rf_stitch_spans: workspace of %zu bytes at %p, %zu bytes aligned to 16 needed", workspace_bytes,
                 workspace_dev, p.total);
    return RF_ERR_CAPACITY;
  }
  char* ws = (char*)workspace_dev;
  float *S = (float*)(ws + p.S), *E = (float*)(ws + p.E), *tmax = (float*)(ws + p.tmax);
  double* tsum = (double*)(ws + p.tsum);
  rf_span* tbest = (rf_span*)(ws + p.tbest);
  hipStream_t st = (hipStream_t)stream;
  if (W > 0) {
    hipLaunchKernelGGL(k_stitch_gather, dim3(W), dim3(RW_THREADS), 0, st, logits_dev, W, T, win_dev, ctx_win_dev, C, S,
                       E, tmax);
    hipLaunchKernelGGL(k_stitch_tiles, dim3(W), dim3(RW_THREADS), 0, st, logits_dev, W, T, win_dev, ctx_win_dev, C, S,
                       E, tmax, max_answer_len, n_best, tbest, tsum);
  }
  hipLaunchKernelGGL(k_stitch_merge, dim3(C), dim3(RW_THREADS), 0, st, logits_dev, W, T, win_dev, ctx_win_dev, tmax,
                     tbest, tsum, n_best, spans_dev, norm_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
