// SQ8 index type: an int8 shadow of the fp16 corpus and the int8 emit sweep of rf_search_sq8.
// Reference: Collection.create_index("embedding", {"index_type": ...}) -- "chunking_storing (1).py":29;
// the pymilvus index type SQ8 trades bytes per row against speed.  Here the answer stays exact:
// the int8 sweep only nominates candidates, with a per-row error bound, and the
// merge rescores them in fp64 from the fp16 tiles.
//
// Shadow layout (caller-owned, rf_sq8_storage_bytes):
//   tiles8  the same 32-row blocks as the fp16 tiles; a block holds KS8 = dim / 32 fragments of
//           1 KiB, fragment kk being the A operand of one v_mfma_i32_32x32x32_i8: lane l
//           (r = l & 31, h = l >> 5) owns the 16 bytes row[32 b + r][32 kk + 16 h .. +16).  The
//           query B fragment takes the same (lane -> k) map, so any k order inside the
//           instruction cancels in the dot product.
//   scale   fp32 [blocks][32] s_r, in accumulator order (rf_sq8_slot): lane half h of a wave
//           finds the 16 values of its accumulator rows at [32 b + 16 h .. +16)
//   err     fp32 [blocks][32] e_r, same order
//   max     {bits of N' = max_r ||s_r c^_r||, bits of E = max_r e_r}, both rounded up
// Quantization is a pure function of the fp16 row (so the shadow after any adds and compactions
// equals a fresh attach over the same rows, byte for byte):
//   s_r = max_i |c_i| / 127 (fp32), c^_i = clamp(rint(c_i / s_r), -127, 127) (fp32 division),
//   e_r >= ||c - s_r c^||_2 (fp64, rounded up into fp32); a zero row gives s_r = 0, c^ = 0, e_r = 0.
#include "rf_internal.h"
#include "scan_common.h"
#include "sq8.h"

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x16 __attribute__((ext_vector_type(16)));

static inline int64_t sq8_blocks(int64_t rows) { return (rows + RF_BLOCK_ROWS - 1) / RF_BLOCK_ROWS; }

// ---- quantization ---------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_xor(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float sq8_code(float x, float s) {
  return s > 0.f ? fminf(fmaxf(rintf(x / s), -127.f), 127.f) : 0.f;
}

// One wave per row: rows [row0, row1) of the fp16 tiles -> int8 fragments, s_r, e_r, and the
// N' / E trackers.  Lane l takes the fp16 chunks l and l + 64 (8 dims each, dim <= 1024); the
// wave reductions run in a fixed order, so a row's values never depend on the launch.
__global__ void __launch_bounds__(256) k_sq8_rows(const uint4* __restrict__ tiles, int KS, int64_t row0,
                                                  int64_t row1, uint2* __restrict__ t8,
                                                  float* __restrict__ scale, float* __restrict__ err,
                                                  uint32_t* __restrict__ mx) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int chunks = 2 * KS;
  const int KS8 = KS / 2;
  float nbest = 0.f, ebest = 0.f;
  for (int64_t row = row0 + wave; row < row1; row += nwaves) {
    half8 v[2];
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = lane + 64 * j;
      v[j] = __builtin_bit_cast(half8, c < chunks ? tiles[rf_chunk_index(row, c, KS)] : make_uint4(0, 0, 0, 0));
#pragma unroll
      for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)v[j][e]));
    }
    m = wave_max_xor(m);
    const float s = m / 127.f;
    double r2 = 0.0, n2 = 0.0;
    const int64_t b = row >> 5;
    const int r = (int)(row & 31);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = lane + 64 * j;
      uint32_t w[2] = {0u, 0u};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = (float)v[j][e];
        const float cq = sq8_code(x, s);
        w[e >> 2] |= ((uint32_t)(int32_t)cq & 0xFFu) << (8 * (e & 3));
        const double y = (double)s * (double)cq;   // exact: 24-bit x 8-bit
        const double d = (double)x - y;
        r2 = fma(d, d, r2);
        n2 = fma(y, y, n2);
      }
      if (c < chunks) {
        const int u = c >> 1;   // 16-byte int8 unit of the row: dims 16 u .. +16
        const size_t idx = ((size_t)b * KS8 + (u >> 1)) * 64 + (size_t)((u & 1) * 32 + r);
        t8[idx * 2 + (c & 1)] = make_uint2(w[0], w[1]);
      }
    }
    r2 = wave_sum_xor(r2);
    n2 = wave_sum_xor(n2);
    const float e = rf_sqrt_up(r2);
    if (lane == 0) {
      const size_t slot = (size_t)b * 32 + rf_sq8_slot(r);
      scale[slot] = s;
      err[slot] = e;
    }
    nbest = fmaxf(nbest, rf_sqrt_up(n2));
    ebest = fmaxf(ebest, e);
  }
  if (lane == 0) {
    if (nbest > 0.f) atomicMax(&mx[0], __builtin_bit_cast(uint32_t, nbest));
    if (ebest > 0.f) atomicMax(&mx[1], __builtin_bit_cast(uint32_t, ebest));
  }
}

// One wave per query slot of a 64-query sweep: q^ (int8 [64][dim]), t_q, n_q = ||q|| and
// f_q = ||q - t_q q^|| (both rounded up).  Slots past B get zeros.
__global__ void __launch_bounds__(64) k_sq8_queries(const _Float16* __restrict__ q, int B, int dim,
                                                    int8_t* __restrict__ q8, float* __restrict__ tq,
                                                    float* __restrict__ nq, float* __restrict__ fq) {
  const int qi = blockIdx.x;
  const int lane = threadIdx.x;
  if (qi >= B) {
    if (lane == 0) tq[qi] = nq[qi] = fq[qi] = 0.f;
    return;
  }
  const _Float16* row = q + (size_t)qi * dim;
  float m = 0.f;
  for (int d = lane; d < dim; d += 64) m = fmaxf(m, fabsf((float)row[d]));
  m = wave_max_xor(m);
  const float t = m / 127.f;
  double n2 = 0.0, f2 = 0.0;
  for (int d = lane; d < dim; d += 64) {
    const float x = (float)row[d];
    const float cq = sq8_code(x, t);
    q8[(size_t)qi * dim + d] = (int8_t)(int32_t)cq;
    const double dd = (double)x - (double)t * (double)cq;
    n2 = fma((double)x, (double)x, n2);
    f2 = fma(dd, dd, f2);
  }
  n2 = wave_sum_xor(n2);
  f2 = wave_sum_xor(f2);
  if (lane == 0) {
    tq[qi] = t;
    nq[qi] = rf_sqrt_up(n2);
    fq[qi] = rf_sqrt_up(f2);
  }
}

// ---- the int8 emit sweep ------------------------------------------------------------------------
struct Sq8Params {
  const uint4* corpus;   // int8 tiles
  const float* scale;    // [blocks][32], accumulator order
  const float* err;
  const int8_t* q8;      // [64][dim]
  const float* tq;       // [64]
  const float* nq;       // [64]
  int B, dim;
  uint32_t n_rows, n_work;
  const float* thr;      // [64] in a~ units (k_threshold with its SQ8 argument)
  uint32_t* cand_cnt;
  uint2* cand;
  uint32_t cap;
};

// emit_flush's hook: an append past the capacity means the merge flags the query
// (RF_FLAG_CAND_OVERFLOW) whatever else is appended, so the workgroup stops testing it (`sat`, LDS).
struct Sq8ListFull {
  unsigned long long* sat;
  __device__ __forceinline__ void operator()(uint32_t q) const { atomicOr(sat, 1ull << q); }
};

struct Sq8Meta {
  float4 s[4], e[4];   // s_r / e_r of the 16 accumulator rows of this lane half
};
__device__ __forceinline__ void load_meta(Sq8Meta& m, const Sq8Params& p, uint32_t b, int h) {
  const float4* sp = (const float4*)(p.scale + (size_t)b * 32 + h * 16);
  const float4* ep = (const float4*)(p.err + (size_t)b * 32 + h * 16);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m.s[j] = sp[j];
    m.e[j] = ep[j];
  }
}
__device__ __forceinline__ float f4_at(const float4 (&v)[4], int i) {
  const float4 x = v[i >> 2];
  return (i & 3) == 0 ? x.x : (i & 3) == 1 ? x.y : (i & 3) == 2 ? x.z : x.w;
}

// One block: KS8 int8 MFMAs per query group from the register ring, then a~ = fl(fl(t_q s_r) D)
// and the lane-local test a~ + n_q e_r >= thr_q, one ballot per block.  The metadata of the NEXT
// block is requested at the top of the step, so its round trip runs under this block's work.
template <int KS8, int R, int JB, bool LAST>
__device__ __forceinline__ void sq8_step(u32x4 (&ring)[R], Sq8Meta& meta, uint32_t b, uint32_t bn,
                                         const u32x4* smemQ, int lane, const float (&th)[JB],
                                         const float (&tq)[JB], const float (&nq)[JB], EmitState& es,
                                         const Sq8Params& p, unsigned long long* sat) {
  static_assert(KS8 % R == 0, "ring must divide the block");
  asm volatile("" ::: "memory");
  const int h = lane >> 5;
  const uint4* cur = p.corpus + (size_t)b * (KS8 * 64) + lane;
  const uint4* nxt = p.corpus + (size_t)bn * (KS8 * 64) + lane;
  Sq8Meta next;
  if (!LAST) load_meta(next, p, bn, h);
  i32x16 acc[JB];
#pragma unroll
  for (int jb = 0; jb < JB; ++jb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[jb][i] = 0;
#pragma unroll
  for (int kk = 0; kk < KS8; ++kk) {
    const i32x4 a = __builtin_bit_cast(i32x4, ring[kk % R]);
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
      const i32x4 bq = __builtin_bit_cast(i32x4, smemQ[(jb * KS8 + kk) * 64 + lane]);
      acc[jb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq, acc[jb], 0, 0, 0);
    }
    if (kk + R < KS8) {
      ring[kk % R] = ld_frag(cur + (kk + R) * 64);
    } else if (!LAST) {
      ring[kk % R] = ld_frag(nxt + (kk + R - KS8) * 64);
    }
  }
  const uint32_t row0 = b * 32u;
  const uint32_t lim = p.n_rows - row0;
  const unsigned long long full = *(volatile unsigned long long*)sat;   // queries whose list is full
  f32x16 sc[JB];
  uint32_t bits = 0u;
#pragma unroll
  for (int jb = 0; jb < JB; ++jb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float a = __fmul_rn(__fmul_rn(tq[jb], f4_at(meta.s, i)), (float)acc[jb][i]);
      sc[jb][i] = a;
      const bool ok = (a + nq[jb] * f4_at(meta.e, i) >= th[jb]) && (acc_row(i, h) < lim) &&
                      ((full >> (jb * 32 + (lane & 31))) & 1ull) == 0ull;
      bits |= ok ? (1u << (jb * 16 + i)) : 0u;
    }
  // the test of a row depends on its own e_r, so the mask is built here; the a~ are what is appended
  if (__ballot(bits != 0u) != 0ull) emit_append<JB>(sc, bits, row0, lane, es, [&] { emit_flush(es, p, lane, Sq8ListFull{sat}); });
  if (!LAST) meta = next;
}

template <int KS8, int R, int JB>
__global__ void __launch_bounds__(256, 2) k_sq8_emit(Sq8Params p) {
  constexpr int WAVES = 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ unsigned long long sat;                                  // queries whose list is full
  u32x4* smemQ = (u32x4*)smem_raw;                                    // JB*KS8*64 uint4
  unsigned char* tail = smem_raw + (size_t)JB * KS8 * RF_FRAG_BYTES;  // emit staging
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5;

  float th[JB], tq[JB], nq[JB];
#pragma unroll
  for (int jb = 0; jb < JB; ++jb) {
    const int qi = jb * 32 + (lane & 31);
    th[jb] = p.thr[qi];
    tq[jb] = p.tq[qi];
    nq[jb] = p.nq[qi];
  }
  EmitState es = emit_state((uint32_t*)tail, wave, WAVES, SCAP);
  const uint32_t W = gridDim.x * WAVES;
  const uint32_t gw = blockIdx.x * WAVES + wave;
  u32x4 ring[R];
  Sq8Meta meta;
  if (gw < p.n_work) {
    const uint4* src = p.corpus + (size_t)gw * (KS8 * 64) + lane;
#pragma unroll
    for (int s = 0; s < R; ++s) ring[s] = ld_frag(src + s * 64);
    load_meta(meta, p, gw, h);
  }
  if (tid == 0) sat = 0ull;
  stage_queries<KS8, JB, WAVES>(smemQ, p.q8, p.B);   // q^[32 jb + j][32 kk + 16 h .. +16)
  __syncthreads();
  const uint32_t cnt = (p.n_work > gw) ? (p.n_work - gw + W - 1) / W : 0u;
  if (cnt > 0) {
    uint32_t b = gw;
    for (uint32_t i = 0; i + 1 < cnt; ++i, b += W)
      sq8_step<KS8, R, JB, false>(ring, meta, b, b + W, smemQ, lane, th, tq, nq, es, p, &sat);
    sq8_step<KS8, R, JB, true>(ring, meta, b, b, smemQ, lane, th, tq, nq, es, p, &sat);
  }
  if (es.cnt > 0) emit_flush(es, p, lane, Sq8ListFull{&sat});
}

// ---- test hooks -------------------------------------------------------------------------------
// a~ for the first n rows (one wave per (block, 32-query group), plain loads) and delta_q
__global__ void __launch_bounds__(64) k_sq8_debug(const uint4* __restrict__ t8, const float* __restrict__ scale,
                                                  int KS8, const int8_t* __restrict__ q8, const float* __restrict__ tq,
                                                  const float* __restrict__ nq, const float* __restrict__ fq,
                                                  const uint32_t* __restrict__ mx, int B, int dim, uint32_t n,
                                                  float* __restrict__ out, float* __restrict__ delta) {
  const int lane = threadIdx.x;
  const int h = lane >> 5;
  const uint32_t b = blockIdx.x;
  const int qi = blockIdx.y * 32 + (lane & 31);
  i32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0;
  for (int kk = 0; kk < KS8; ++kk) {
    const uint4 av = t8[((size_t)b * KS8 + kk) * 64 + lane];
    uint4 bv = make_uint4(0, 0, 0, 0);
    if (qi < B) bv = *(const uint4*)(q8 + (size_t)qi * dim + kk * 32 + h * 16);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, av), __builtin_bit_cast(i32x4, bv), acc,
                                                0, 0, 0);
  }
  if (qi >= B) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t row = b * 32u + acc_row(i, h);
    if (row < n)
      out[(size_t)qi * n + row] = __fmul_rn(__fmul_rn(tq[qi], scale[(size_t)b * 32 + h * 16 + i]), (float)acc[i]);
  }
  if (b == 0 && h == 0 && delta)
    delta[qi] = rf_sq8_delta(nq[qi], fq[qi], __builtin_bit_cast(float, mx[0]), __builtin_bit_cast(float, mx[1]));
}

// un-tiled int8 rows [n, dim], s_r [n], e_r [n] of rows rows[0..n) (rows outside [0, size): zeros)
__global__ void k_sq8_get_rows(const uint4* __restrict__ t8, const float* __restrict__ scale,
                               const float* __restrict__ err, const int64_t* __restrict__ rows, int64_t n, int KS8,
                               int64_t size, uint4* __restrict__ out, float* __restrict__ s_out,
                               float* __restrict__ e_out) {
  const int units = 2 * KS8;
  const int64_t total = n * units;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int64_t j = i / units;
    const int u = (int)(i % units);
    const int64_t row = rows[j];
    const bool ok = row >= 0 && row < size;
    const int64_t b = ok ? row >> 5 : 0;
    const int r = ok ? (int)(row & 31) : 0;
    out[i] = ok ? t8[((size_t)b * KS8 + (u >> 1)) * 64 + (u & 1) * 32 + r] : make_uint4(0, 0, 0, 0);
    if (u == 0) {
      s_out[j] = ok ? scale[(size_t)b * 32 + rf_sq8_slot(r)] : 0.f;
      e_out[j] = ok ? err[(size_t)b * 32 + rf_sq8_slot(r)] : 0.f;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
static inline int grid_for(int64_t work_items, int block) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return (int)g;
}

extern "C" size_t rf_sq8_storage_bytes(int dim, int64_t capacity_rows) {
  if (dim <= 0 || dim % 32 != 0 || !rf_scan_supported_dim(dim) || capacity_rows <= 0) return 0;
  const size_t blocks = (size_t)sq8_blocks(capacity_rows);
  return blocks * ((size_t)(dim / 32) * RF_FRAG_BYTES + 2 * 32 * sizeof(float)) + 256;
}

int rf_sq8_quantize_rows(rf_index* ix, int64_t row0, int64_t row1, hipStream_t st) {
  const int64_t end = sq8_blocks(row1) * RF_BLOCK_ROWS;   // whole blocks: pad rows read as zero
  if (end <= row0) return RF_OK;
  hipLaunchKernelGGL(k_sq8_rows, dim3(grid_for((end - row0) * 64, 256)), dim3(256), 0, st, ix->tiles, ix->KS,
                     row0, end, (uint2*)ix->sq8_tiles, ix->sq8_scale, ix->sq8_err, ix->sq8_max);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

extern "C" int rf_index_attach_sq8(rf_index_t* ix, void* storage_dev, size_t storage_bytes, void* stream) {
  if (!ix || !storage_dev) {
    rf_set_error("rf_index_attach_sq8: null argument");
    return RF_ERR_INVALID;
  }
  if (ix->dim % 32 != 0) {
    rf_set_error("rf_index_attach_sq8: SQ8 needs dim %% 32 == 0 (dim %d)", ix->dim);
    return RF_ERR_UNSUPPORTED;
  }
  const size_t need = rf_sq8_storage_bytes(ix->dim, ix->capacity);
  if (storage_bytes < need) {
    rf_set_error("rf_index_attach_sq8: storage %zu B < required %zu B", storage_bytes, need);
    return RF_ERR_CAPACITY;
  }
  if (((uintptr_t)storage_dev & 15) != 0) {
    rf_set_error("rf_index_attach_sq8: storage not 16-byte aligned");
    return RF_ERR_INVALID;
  }
  const size_t blocks = (size_t)sq8_blocks(ix->capacity);
  unsigned char* base = (unsigned char*)storage_dev;
  ix->sq8_tiles = (uint4*)base;
  ix->sq8_scale = (float*)(base + blocks * (ix->dim / 32) * RF_FRAG_BYTES);
  ix->sq8_err = ix->sq8_scale + blocks * 32;
  ix->sq8_max = (uint32_t*)(ix->sq8_err + blocks * 32);
  hipStream_t st = (hipStream_t)stream;
  RF_HIP(hipMemsetAsync(ix->sq8_max, 0, 256, st));
  if (ix->size > 0) return rf_sq8_quantize_rows(ix, 0, ix->size, st);
  return RF_OK;
}

extern "C" int rf_index_detach_sq8(rf_index_t* ix) {
  if (!ix) {
    rf_set_error("rf_index_detach_sq8: null index");
    return RF_ERR_INVALID;
  }
  ix->sq8_tiles = nullptr;
  ix->sq8_scale = nullptr;
  ix->sq8_err = nullptr;
  ix->sq8_max = nullptr;
  return RF_OK;
}

extern "C" int rf_index_get_rows_sq8(const rf_index_t* ix, const int64_t* rows_dev, int64_t n, void* out_dev,
                                     float* scales_dev, float* err_dev, void* stream) {
  if (!ix || !rows_dev || !out_dev || !scales_dev || !err_dev || n < 0) {
    rf_set_error("rf_index_get_rows_sq8: bad argument");
    return RF_ERR_INVALID;
  }
  if (!ix->sq8_tiles) {
    rf_set_error("rf_index_get_rows_sq8: no SQ8 shadow attached");
    return RF_ERR_INVALID;
  }
  if (((uintptr_t)out_dev & 15) != 0) {
    rf_set_error("rf_index_get_rows_sq8: out not 16-byte aligned");
    return RF_ERR_INVALID;
  }
  if (n == 0) return RF_OK;
  const int KS8 = ix->dim / 32;
  hipLaunchKernelGGL(k_sq8_get_rows, dim3(grid_for(n * KS8 * 2, 256)), dim3(256), 0, (hipStream_t)stream,
                     ix->sq8_tiles, ix->sq8_scale, ix->sq8_err, rows_dev, n, KS8, ix->size, (uint4*)out_dev,
                     scales_dev, err_dev);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_sq8_queries(const rf_index* ix, const void* q, int B, const rf_sq8_ws& sw, hipStream_t st) {
  hipLaunchKernelGGL(k_sq8_queries, dim3(RF_QCHUNK), dim3(64), 0, st, (const _Float16*)q, B, ix->dim, sw.q8, sw.tq,
                     sw.nq, sw.fq);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_sq8_debug(const rf_index* ix, int B, int64_t n, const rf_sq8_ws& sw, float* out, float* delta,
                        hipStream_t st) {
  const dim3 grid((unsigned)((n + 31) / 32), (B + 31) / 32);
  hipLaunchKernelGGL(k_sq8_debug, grid, dim3(64), 0, st, ix->sq8_tiles, ix->sq8_scale, ix->dim / 32, sw.q8, sw.tq,
                     sw.nq, sw.fq, ix->sq8_max, B, ix->dim, (uint32_t)n, out, delta);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

template <int KS8, int R, int JB>
static int launch_sq8(const Sq8Params& p, int grid, hipStream_t st) {
  const size_t lds = (size_t)JB * KS8 * RF_FRAG_BYTES + (size_t)3 * 4 * SCAP * 4;
  static rf_lds_attr attr;  // per instantiation, per device
  RF_HIP(rf_ensure_lds(attr, (const void*)k_sq8_emit<KS8, R, JB>, lds));
  hipLaunchKernelGGL((k_sq8_emit<KS8, R, JB>), dim3(grid), dim3(256), lds, st, p);
  RF_HIP(hipGetLastError());
  return RF_OK;
}

int rf_launch_sq8_emit(const rf_index* ix, int B, int JB, const rf_workspace& ws, const rf_sq8_ws& sw,
                       hipStream_t st) {
  const uint32_t nblk = (uint32_t)((ix->size + 31) / 32);
  int grid = ix->num_cus * 2;
  const uint32_t need = (nblk + 3) / 4;
  if ((uint32_t)grid > need) grid = (int)need;
  if (grid < 1) grid = 1;
  Sq8Params p{};
  p.corpus = ix->sq8_tiles;
  p.scale = ix->sq8_scale;
  p.err = ix->sq8_err;
  p.q8 = sw.q8;
  p.tq = sw.tq;
  p.nq = sw.nq;
  p.B = B;
  p.dim = ix->dim;
  p.n_rows = (uint32_t)ix->size;
  p.n_work = nblk;
  p.thr = ws.thr;
  p.cand_cnt = ws.cand_cnt;
  p.cand = ws.cand;
  p.cap = RF_SHARD_CAP;
  // ring: a whole block up to 8 KiB, otherwise 6, 8 or 12 fragments (must divide KS8); dim 384 takes half a
  // block: 6 beat 12 by 2.4 us per sweep in the interleaved A/B, 4 did not beat 6
#define RF_SQ8(ks8, r) \
  case ks8:            \
    return JB == 1 ? launch_sq8<ks8, r, 1>(p, grid, st) : launch_sq8<ks8, r, 2>(p, grid, st);
#ifdef RF_EXPERIMENTS
  // A/B of the ring depth at dim 384 (tools/bench_sq8_ring.py, profiles/flat_shadow_emit_ab.txt); the product
  // below dispatches the ring of 6 that won it
  if (ix->dim / 32 == 12 && rf_knob_sq8_ring12 == 12)
    return JB == 1 ? launch_sq8<12, 12, 1>(p, grid, st) : launch_sq8<12, 12, 2>(p, grid, st);
  if (ix->dim / 32 == 12 && rf_knob_sq8_ring12 == 4)
    return JB == 1 ? launch_sq8<12, 4, 1>(p, grid, st) : launch_sq8<12, 4, 2>(p, grid, st);
#endif
  switch (ix->dim / 32) {
    RF_SQ8(2, 2) RF_SQ8(4, 4) RF_SQ8(8, 8) RF_SQ8(12, 6) RF_SQ8(16, 8) RF_SQ8(24, 12) RF_SQ8(32, 8)
    default:
      break;
  }
#undef RF_SQ8
  rf_set_error("no SQ8 emit kernel for dim %d", ix->dim);
  return RF_ERR_UNSUPPORTED;
}
