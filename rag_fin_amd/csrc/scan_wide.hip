// Wide sweep: up to 256 queries against the corpus in ONE pass (dim 384), one kernel: k_scan_w16.
//
// The 64-query kernel (scan.hip) keeps the queries in LDS and streams corpus fragments straight
// into registers; at 256 queries the roles flip:
//   * each of the 8 waves of a workgroup owns 32 queries and keeps them as B-operand fragments in
//     REGISTERS for the whole sweep (96 VGPRs, loaded once);
//   * a corpus block (32 rows, 24 KiB) is brought from HBM ONCE per workgroup by LDS-DMA into a
//     3-slot ring of 2-block phases and shared by the 8 waves through LDS.
// Arithmetic intensity is 256 flop per corpus byte: HBM and the matrix pipe are both near their
// roofs (BASELINE.json configs[2], "HBM-roofline run").  DESIGN.md 4.1b has the measurements and
// the forms that were tried and dropped; their source is in the git history (the round-1 kernel
// with 32x32x16 MFMAs and waves in lockstep, a register-staged ring, 4 waves x 64 queries, every
// wave streaming the corpus itself: 447 us per step -- 8x the load instructions saturate the TA
// path).
#include "scan_common.h"
#include "lds_ring.h"
#include <stdlib.h>
#include <type_traits>

#define WIDE_KS 24

struct WideParams {
  const uint4* corpus;
  const _Float16* q;
  int B;
  uint32_t n_rows;
  uint32_t n_work;
  uint32_t bstride;
  const float* thr;
  uint32_t* cand_cnt;
  uint2* cand;
  uint32_t cap;
  float* pmax;
  int P;
};

int rf_wide_supported(const rf_index* ix) { return ix->KS == WIDE_KS; }

// The corpus arrives by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave-instruction, the
// fragment image is lane-linear so HBM order == LDS order): no staging registers, no ds_write
// pass.  A phase = 2 blocks (64 rows, 48 KiB contiguous in HBM); 3 LDS slots; loads run two
// phases (96 KiB per CU) ahead behind a counted vmcnt and one raw s_barrier per phase, the pieces
// spread over the phase's groups of MFMAs (an LDS-DMA issue holds its wave for tens of cycles).
// The A-operand reads are inline-asm ds_read_b128 with hand-counted lgkmcnt waits (as
// compiler-visible LDS loads each would get an s_waitcnt vmcnt(0): hipcc cannot tell them from the
// DMA writes in flight).  Two waves per SIMD with 32 queries each: the partner wave's MFMAs cover
// the other's non-matrix work.
#define WL_SLOTS 3
#define WL_PB 2                               // corpus blocks per phase
#define WL_FRAGS (WIDE_KS * WL_PB)            // 1-KiB fragments per phase (48)
#define WL_STAGE_WORDS 3072                   // emit staging, all waves: 8 x 32 entries x W16_ENTRY_WORDS

__device__ __forceinline__ float vmax3(float a, float b, float c) {
  // v_max3_f32 straight on the MFMA results (fmaxf adds a canonicalising v_max per element)
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// The kernel: v_mfma_f32_16x16x32_f16, staggered wave halves.  Three choices that the counters of
// its lockstep 32x32x16 predecessor asked for (profiles/r01q_pmc_wide.json: matrix pipe busy 47 %,
// 2.4 VALU instructions per MFMA):
//   * 16x16x32 MFMAs.  Same FLOP per cycle as 32x32x16, but the chip -- which is power-bound
//     in this kernel (1.4-1.5 GHz under a 32x32x16 loop) -- holds a higher clock under them
//     (MI355X_MICROARCH.md "DVFS give-back" item 7: 1.12-1.15x the FLOP/s; own microbench
//     tools/micro/mfma_operand_bench.hip: 5-10 %).  The corpus image is unchanged: lane l of a
//     16-row x 32-k A operand reads 16 bytes of fragment 2 ks + (g >> 1), g = l >> 4, at source
//     lane 32 (g & 1) + 16 rg + (l & 15) -- within each 16-lane service group of ds_read_b128
//     the sixteen 16-byte slots are distinct mod 256 B, i.e. the permuted read is conflict-free.
//     A wave's tile per block is 2 row groups x 2 query groups; every A read feeds two MFMAs,
//     and the four accumulators rotate, so no MFMA waits on its predecessor.
//   * The two waves of a SIMD (w and w + 4) do not run the phase in lockstep.  Waves 0-3
//     issue their six LDS-DMA pieces (60-185 cycles of issue stall each) in the first half of
//     the phase and filter at MFMA groups 0 and 6; waves 4-7 issue in the second half and filter
//     at groups 3 and 9: one wave's non-matrix work falls under its partner's MFMAs.
//   * Filter without copies: v_max3 reads the accumulators in place (the hazard nops take the
//     accumulator itself as in/out operand), 3 max3 + 1 max + 1 compare per query group and
//     block; the slow path is one v_cmp per accumulator register whose SGPR result IS the
//     ballot, and runs only for the query group that hit.
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define W16_KS 12   // k-steps of 32 per row (dim 384)
#ifndef W16_AHEAD
#define W16_AHEAD 2   // groups of A-operand reads in flight ahead of their MFMAs (1 | 2)
#endif

// four A-operand reads at immediate offsets O0..O3 from the lane's slot address
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ void w16_read4(rf_u32x4 (&d)[4], uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d[0]) : "v"(addr), "n"(O0));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d[1]) : "v"(addr), "n"(O1));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d[2]) : "v"(addr), "n"(O2));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d[3]) : "v"(addr), "n"(O3));
}
// group gi (0..11) of a phase: block gi / 6, k-steps 2 (gi % 6) and + 1, row groups 0 and 1
template <int GI>
__device__ __forceinline__ void w16_read_group(rf_u32x4 (&d)[4], uint32_t addr) {
  constexpr int base = (GI / 6) * (WIDE_KS * RF_FRAG_BYTES) + (2 * (GI % 6)) * 2048;
  w16_read4<base, base + 256, base + 2048, base + 2048 + 256>(d, addr);
}

struct W16Acc {
  f32x4 t[2][2];   // [row group][query group]: lane l = query 16 qg + (l & 15), rows 16 rg + 4 (l >> 4) + j
};

__device__ __forceinline__ float w16_max8(W16Acc& a, int qg) {
  // MFMA write -> VALU read wait states, by hand (the v_max3 are inline asm, invisible to the
  // hazard recognizer): the nops take the accumulator registers they guard as in/out
  asm volatile("s_nop 7\n\ts_nop 3" : "+v"(a.t[0][qg]), "+v"(a.t[1][qg]));
  const float m0 = vmax3(a.t[0][qg][0], a.t[0][qg][1], a.t[0][qg][2]);
  const float m1 = vmax3(a.t[0][qg][3], a.t[1][qg][0], a.t[1][qg][1]);
  const float m2 = vmax3(a.t[1][qg][2], a.t[1][qg][3], m0);
  return vmax3(m1, m2, m2);
}

// Emit staging (LDS, per wave): entries of 12 words = { row of score 0, query, the query's
// threshold, pad, 8 scores }: a lane whose 8-row column of a block holds a score >= threshold
// appends the WHOLE column (rows base + j and base + 16 + j, j = 0..3) with two ds_write_b128 and
// one ds_write_b96 -- a handful of instructions, the same for every hit, so a hit does not make
// its wave late at the phase barrier (the round-1 form scanned the sixteen accumulator registers
// with a ballot each: ~200 cycles per hit, and with ~3 hits per phase and workgroup nearly every
// phase waited for somebody's slow path).  The threshold test per score and the row bound are
// applied when the staging area is flushed, 64 scores at a time.
#define W16_ENTRY_WORDS 12
struct W16Stage {
  uint32_t* base;       // this wave's entries
  uint32_t base_addr;   // ... as an LDS byte address
  uint32_t cnt;         // wave-uniform
};

template <int CAP_E, class P>
__device__ __forceinline__ void w16_append(const W16Acc& a, int qg, unsigned long long mask, float th, uint32_t row0,
                                           uint32_t q, int lane, W16Stage& st, const P& p) {
  const uint32_t n = (uint32_t)__popcll(mask);
  const bool ok = (mask >> lane) & 1ull;
  if (st.cnt + n <= (uint32_t)CAP_E) {
    if (ok) {
      // inline-asm stores: a compiler-visible LDS store gets an s_waitcnt vmcnt(0) in front of it (hipcc
      // cannot tell it from the LDS-DMA writes in flight), i.e. every hit would drain the corpus ring
      const uint32_t e = st.base_addr + (st.cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))) * (W16_ENTRY_WORDS * 4);
      const u32x4 hdr = {row0 + 4u * (uint32_t)(lane >> 4), q, __builtin_bit_cast(uint32_t, th), 0u};
      asm volatile("ds_write_b128 %0, %1\n\tds_write_b128 %0, %2 offset:16\n\tds_write_b128 %0, %3 offset:32"
                   :: "v"(e), "v"(hdr), "v"(a.t[0][qg]), "v"(a.t[1][qg]) : "memory");
    }
    st.cnt += n;
  } else if (ok) {   // staging full within one phase (adversarial duplicates): flag the query
    atomicAdd(&p.cand_cnt[q * RF_CAND_SHARDS + (blockIdx.x & (RF_CAND_SHARDS - 1))], p.cap + 1u);
  }
}

template <class P>
__device__ __forceinline__ void w16_flush(W16Stage& st, const P& p, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  for (uint32_t i = lane; i < st.cnt * 8u; i += 64) {
    const uint32_t* e = st.base + (i >> 3) * W16_ENTRY_WORDS;
    const uint32_t s = i & 7u;
    const float score = __builtin_bit_cast(float, e[4 + s]);
    const uint32_t row = e[0] + 16u * (s >> 2) + (s & 3u);
    if (score >= __builtin_bit_cast(float, e[2]) && row < p.n_rows) {
      const uint32_t list = e[1] * RF_CAND_SHARDS + (blockIdx.x & (RF_CAND_SHARDS - 1));
      const uint32_t slot = atomicAdd(&p.cand_cnt[list], 1u);
      if (slot < p.cap) p.cand[(size_t)list * p.cap + slot] = make_uint2(row, __builtin_bit_cast(uint32_t, score));
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  st.cnt = 0;
}

// NE: LDS-DMA pieces per phase issued by each of waves 0-3 (waves 4-7 issue 12 - NE each).  The two
// waves of a SIMD are NOT treated alike by the hardware: at equal priority the older one wins every
// arbitration, the younger runs in what is left.  With the stall-prone work (LDS-DMA issue: 60-185
// cycles each) split evenly, the winner finished its phase after ~3 000 cycles and then waited
// ~1 650 cycles at the barrier, while the loser ran its own MFMAs AND its own stalls in the time
// that was left (in-kernel stamps, profiles/r02e_wide_stamps.txt: 4 684 cycles per phase against
// 3 072 of matrix work).  So the roles are made unequal on purpose: waves 0-3 run at s_setprio 1
// and carry (nearly) all the LDS-DMA issues -- their stalls are the slots in which waves 4-7, which
// do almost nothing but MFMAs, get the matrix pipe.
template <int MODE, int DBG, int NE>
__global__ void __launch_bounds__(512, 1) k_scan_w16(WideParams p) {
  constexpr int NW = 8;
  constexpr int NL = WL_FRAGS / 4 - NE;          // pieces per phase of each of waves 4-7
  static_assert(NE >= 6 && NE <= 12, "pieces per early wave");
  constexpr int CAP_E = WL_STAGE_WORDS / NW / W16_ENTRY_WORDS;   // emit staging entries per wave: 32
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  // ONE shared array: [WL_SLOTS][48 fragments][64 lanes] uint4, the emit staging words, and a
  // 1-KiB dump area for the pieces issued past the end of the stream
  u32x4* slots = (u32x4*)smem_raw;
  uint32_t* stage = (uint32_t*)(slots + WL_SLOTS * WL_FRAGS * 64);
  u32x4* const dump = (u32x4*)(stage + WL_STAGE_WORDS);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g = lane >> 4;

  // work items (block PAIRS) of this workgroup: u = blockIdx.x, + gridDim.x, ...
  const uint32_t G = gridDim.x;
  const uint32_t cnt = (p.n_work > blockIdx.x) ? (p.n_work - blockIdx.x + G - 1) / G : 0u;
  if (cnt == 0) return;  // workgroup-uniform
  const uint32_t nblk = (p.n_rows + 31u) >> 5;

  // A phase is 48 fragments (two blocks, contiguous in HBM).  Wave w < 4 brings fragments
  // NE w .. NE w + NE - 1, wave w >= 4 fragments 4 NE + NL (w - 4) .. + NL - 1.  Every phase issues
  // exactly the same number of pieces per wave, so the vmcnt arithmetic is the same in the last
  // phases: past the end the pieces re-read the corpus' last block into the dump area (an L2 hit,
  // no HBM traffic), and so does the second block of an odd tail (its rows are masked by row1).
  const bool early = wave < NW / 2;
  const uint32_t f0 = early ? (uint32_t)(wave * NE) : (uint32_t)(4 * NE + (wave - 4) * NL);
  struct Pieces {
    const uint4* src;   // lane's address of fragment 0 of the phase
    u32x4* dst;         // fragment 0 of the slot (or the dump area)
    int dstep;
    uint32_t cut;       // fragments >= cut come from 24 fragments further back (odd tail: the pair's second block does not exist)
  };
  auto pieces_of = [&](uint32_t ph) {
    const bool live = ph < cnt;
    uint32_t b = (blockIdx.x + ph * G) * p.bstride * WL_PB;
    Pieces pc;
    pc.cut = (live && b + 1u < nblk) ? 2u * WIDE_KS : (uint32_t)WIDE_KS;
    b = (live && b < nblk) ? b : nblk - 1u;
    pc.src = p.corpus + (size_t)b * WIDE_KS * 64 + lane;
    pc.dst = live ? slots + (ph % WL_SLOTS) * WL_FRAGS * 64 : dump;
    pc.dstep = live ? 64 : 0;
    return pc;
  };
  auto issue_piece = [&](const Pieces& pc, int j) {
    const uint32_t f = f0 + (uint32_t)j;
    const uint32_t fs = (DBG & 1) ? 0u : (f >= pc.cut ? f - (uint32_t)WIDE_KS : f);   // DBG 1: every piece re-reads one cached KiB
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pc.src + (size_t)fs * 64),
                                     (__attribute__((address_space(3))) void*)(pc.dst + f * pc.dstep), 16, 0, 2 /* nt */);
  };

  // the first two phases of the corpus stream start before anything else
  {
    const Pieces p0 = pieces_of(0), p1 = pieces_of(1);
    if (early) {
#pragma unroll
      for (int j = 0; j < NE; ++j) issue_piece(p0, j);
#pragma unroll
      for (int j = 0; j < NE; ++j) issue_piece(p1, j);
    } else {
#pragma unroll
      for (int j = 0; j < NL; ++j) issue_piece(p0, j);
#pragma unroll
      for (int j = 0; j < NL; ++j) issue_piece(p1, j);
    }
  }

  // this wave's 32 queries as B operands of the 16x16x32 MFMA, resident for the whole sweep:
  // qf[qg][ks], lane l = query 32 wave + 16 qg + (l & 15), dims 32 ks + 8 (l >> 4) .. + 8
  u32x4 qf[2][W16_KS];
  float th[2];
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) {
    const int qi = wave * 32 + qg * 16 + c16;
    const int qc = qi < p.B ? qi : p.B - 1;   // unconditional loads (no branch per fragment)
#pragma unroll
    for (int ks = 0; ks < W16_KS; ++ks)
      qf[qg][ks] = *(const u32x4*)(p.q + (size_t)qc * (WIDE_KS * 16) + ks * 32 + g * 8);
    th[qg] = (MODE == MODE_EMIT) ? p.thr[qc] : 0.f;
    if (qi >= p.B || (DBG & 1)) th[qg] = INFINITY;
  }
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) {
    const int qi = wave * 32 + qg * 16 + c16;
#pragma unroll
    for (int ks = 0; ks < W16_KS; ++ks) {
      u32x4 v = qf[qg][ks];
      if (qi >= p.B) v = u32x4{0u, 0u, 0u, 0u};
      asm volatile("" : "+v"(v));   // resident: not to be re-materialised inside the loop
      qf[qg][ks] = v;
    }
  }
  float pm[2] = {-INFINITY, -INFINITY};
  W16Stage st;
  st.cnt = 0;
  st.base = stage + wave * (WL_STAGE_WORDS / NW);
  st.base_addr = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)st.base;

  // score filter of one 32-row block.  Sample: running maximum per lane and query group;
  // emit: any score >= the query's threshold sends the wave down the append path.
  auto filter = [&](W16Acc& a, uint32_t row0) __attribute__((always_inline)) {
    if (MODE == MODE_SAMPLE) {
      if (row0 + 32u > p.n_rows) {   // wave-uniform: the corpus' last block / a block past the end
#pragma unroll
        for (int rg = 0; rg < 2; ++rg)
#pragma unroll
          for (int qg = 0; qg < 2; ++qg)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (row0 + (uint32_t)(16 * rg + 4 * g + j) >= p.n_rows) a.t[rg][qg][j] = -INFINITY;
      }
#pragma unroll
      for (int qg = 0; qg < 2; ++qg) pm[qg] = vmax3(pm[qg], w16_max8(a, qg), pm[qg]);
    } else {
      const float m0 = w16_max8(a, 0), m1 = w16_max8(a, 1);
      const unsigned long long h0 = __builtin_amdgcn_fcmpf(m0, th[0], 3 /* FCMP_OGE */),
                               h1 = __builtin_amdgcn_fcmpf(m1, th[1], 3);
      if ((h0 | h1) != 0ull) {
        const uint32_t q0 = (uint32_t)(wave * 32 + c16);
        if (h0 != 0ull) w16_append<CAP_E>(a, 0, h0, th[0], row0, q0, lane, st, p);
        if (h1 != 0ull) w16_append<CAP_E>(a, 1, h1, th[1], row0, q0 + 16u, lane, st, p);
      }
    }
  };

  // lane's byte address of A-operand (block 0, k-step 0, row group 0) inside a slot
  const uint32_t lane_a = (uint32_t)(((g >> 1) * 64 + (g & 1) * 32 + c16) * 16);
  W16Acc acc0, acc1;   // acc1 outlives its phase: it is filtered inside the next one
#pragma unroll
  for (int rg = 0; rg < 2; ++rg)
#pragma unroll
    for (int qg = 0; qg < 2; ++qg)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc0.t[rg][qg][j] = acc1.t[rg][qg][j] = -INFINITY;
  uint32_t row1_prev = p.n_rows;
  uint64_t t_wait = 0, t_bar = 0, t_c0 = 0, t_r0 = 0, t_flush = 0;
  float n_flush = 0.f;
  if (DBG & 4) {
    t_c0 = __builtin_amdgcn_s_memtime();
    t_r0 = __builtin_amdgcn_s_memrealtime();
  }
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // one phase for the EARLY (waves 0-3) or LATE (waves 4-7) half of the workgroup
  auto phase = [&](uint32_t ph, auto late_tag) __attribute__((always_inline)) {
    constexpr bool LATE = decltype(late_tag)::value;
    constexpr int F1_AT = LATE ? 4 : 1;    // MFMA group in front of which the PREVIOUS phase's second block is filtered
    constexpr int F0_AT = LATE ? 10 : 7;   // ... and this phase's first block
    constexpr int NP = LATE ? NL : NE;     // my LDS-DMA pieces per phase, spread evenly over the 12 MFMA groups
    // my pieces of phase ph have landed (my NP pieces of phase ph+1 may stay in flight) ...
    uint64_t ts0 = 0, ts1 = 0;
    if (DBG & 4) ts0 = __builtin_amdgcn_s_memtime();
    if (DBG & 8) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP) : "memory");
    if (DBG & 4) {
      ts1 = __builtin_amdgcn_s_memtime();
      t_wait += ts1 - ts0;
    }
    // ... and after the barrier everybody's have, and everybody has consumed phase ph-1
    __builtin_amdgcn_s_barrier();
    if (DBG & 4) t_bar += __builtin_amdgcn_s_memtime() - ts1;
    const Pieces nxt = pieces_of(ph + 2);  // goes into the slot phase ph - 1 has just vacated
    const u32x4* slot = slots + (ph % WL_SLOTS) * (WL_FRAGS * 64);
    const uint32_t sa = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)slot + lane_a;
    const uint32_t b0 = (blockIdx.x + ph * G) * p.bstride * WL_PB;
    const uint32_t row0 = (b0 < nblk) ? b0 * 32u : p.n_rows;
    const uint32_t row1 = (b0 + 1u < nblk) ? (b0 + 1u) * 32u : p.n_rows;
    // A operands: groups of 4 reads, W16_AHEAD groups in flight ahead of the MFMAs that consume them
    rf_u32x4 fa[W16_AHEAD + 1][4];
    if (DBG & 64) {   // ablation: no A-operand reads at all (stale registers: wrong results)
#pragma unroll
      for (int i = 0; i < W16_AHEAD + 1; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "=v"(fa[i][j]));
    } else {
      w16_read_group<0>(fa[0], sa);
      if (W16_AHEAD > 1) w16_read_group<1>(fa[1], sa);
    }
    __builtin_amdgcn_sched_barrier(0);
    // the one flush site of the loop (the append path never flushes)
    if (MODE == MODE_EMIT && st.cnt >= (uint32_t)CAP_E / 4) {   // (3/4 instead: no flush left in the loop, the sweep no faster: 165.4 against 165.0 us)
      uint64_t tf0 = 0;
      if (DBG & 4) tf0 = __builtin_amdgcn_s_memtime();
      w16_flush(st, p, lane);
      if (DBG & 4) {
        t_flush += __builtin_amdgcn_s_memtime() - tf0;
        n_flush += 1.f;
      }
    }
#define W16_GROUP(GI)                                                                                          \
    {                                                                                                          \
      constexpr int SLOT = GI % (W16_AHEAD + 1);                                                               \
      if (GI % 3 == 0 && !(DBG & 16)) __builtin_amdgcn_s_setprio(3 - GI / 3);   /* the wave that is behind wins */ \
      if (DBG & 64) {                                                                                          \
      } else if (GI + W16_AHEAD < 12) {                                                                        \
        w16_read_group<(GI + W16_AHEAD < 12 ? GI + W16_AHEAD : 0)>(fa[(GI + W16_AHEAD) % (W16_AHEAD + 1)], sa); \
        if (!(DBG & 32)) lds_wait_group<4 * W16_AHEAD>(fa[SLOT]);   /* DBG 32: no wait for the operands (wrong results) */ \
      } else {                                                                                                 \
        if (!(DBG & 32)) lds_wait_group<4 * (11 - GI)>(fa[SLOT]);                                              \
      }                                                                                                        \
      if (GI == F1_AT && !(DBG & 2)) filter(acc1, row1_prev);                                                  \
      if (GI == F0_AT && !(DBG & 2)) filter(acc0, row0);                                                       \
      if (!(DBG & 8)) {                                                                                        \
        _Pragma("unroll") for (int j = (GI * NP) / 12; j < ((GI + 1) * NP) / 12; ++j) issue_piece(nxt, j);     \
      }                                                                                                        \
      W16Acc& dst = (GI < 6) ? acc0 : acc1;                                                                    \
      _Pragma("unroll") for (int u = 0; u < 2; ++u) {         /* k-step 2 (GI % 6) + u */                      \
        const int ks = 2 * (GI % 6) + u;                                                                       \
        _Pragma("unroll") for (int rg = 0; rg < 2; ++rg) {                                                     \
          const half8 a = __builtin_bit_cast(half8, fa[SLOT][2 * u + rg]);                                     \
          _Pragma("unroll") for (int qg = 0; qg < 2; ++qg)                                                     \
            dst.t[rg][qg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(half8, qf[qg][ks]),   \
                                                                   ks ? dst.t[rg][qg] : zero4, 0, 0, 0);       \
        }                                                                                                      \
      }                                                                                                        \
    }
    W16_GROUP(0) W16_GROUP(1) W16_GROUP(2) W16_GROUP(3) W16_GROUP(4) W16_GROUP(5)
    W16_GROUP(6) W16_GROUP(7) W16_GROUP(8) W16_GROUP(9) W16_GROUP(10) W16_GROUP(11)
#undef W16_GROUP
    row1_prev = row1;
  };

  for (uint32_t ph = 0; ph < cnt; ++ph) {
    if (early) phase(ph, std::false_type{});
    else phase(ph, std::true_type{});
  }
  if (!(DBG & 2)) filter(acc1, row1_prev);   // the last phase's second block
  if (DBG & 2) asm volatile("" : "+v"(acc0.t[0][0]), "+v"(acc0.t[1][1]), "+v"(acc1.t[0][0]), "+v"(acc1.t[1][1]));

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the dump pieces must land before the LDS is handed on
  if ((DBG & 4) && p.pmax && lane == 0) {   // diagnostic run only (tools/bench_wide.py --dbg 4)
    float* o = p.pmax + ((size_t)blockIdx.x * NW + wave) * 8;
    o[0] = (float)(__builtin_amdgcn_s_memtime() - t_c0);
    o[1] = (float)(__builtin_amdgcn_s_memrealtime() - t_r0);
    o[2] = (float)t_wait;   // cycles in the vmcnt wait (my LDS-DMA pieces of the phase not landed yet)
    o[3] = (float)cnt;
    o[4] = (float)t_bar;    // cycles in s_barrier (waiting for the slowest wave)
    o[5] = (float)t_flush;  // cycles in the staging flushes of the loop (global atomics)
    o[6] = n_flush;
  }
  if (MODE == MODE_EMIT) {
    if (st.cnt > 0) w16_flush(st, p, lane);
  } else {
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
      const int qi = wave * 32 + qg * 16 + c16;
      float m = fmaxf(pm[qg], __shfl_xor(pm[qg], 16));
      m = fmaxf(m, __shfl_xor(m, 32));
      if (g == 0 && qi < p.B) p.pmax[(size_t)qi * p.P + blockIdx.x] = m;
    }
  }
}

// ---- host side ---------------------------------------------------------------------------
static size_t wide_lds_bytes() {
  return (size_t)WL_SLOTS * WL_FRAGS * RF_FRAG_BYTES + (size_t)WL_STAGE_WORDS * 4 + (size_t)RF_FRAG_BYTES;   // slots, emit staging, dump area
}
#define W16_NE 12   // LDS-DMA pieces per phase of each of waves 0-3 (the product's choice; see k_scan_w16)
template <int MODE, int DBG, int NE = W16_NE>
static int launch_w16(const WideParams& p, int grid, hipStream_t st) {
  auto kern = k_scan_w16<MODE, DBG, NE>;
  static rf_lds_attr attr;   // per instantiation, per device
  RF_HIP(rf_ensure_lds(attr, (const void*)kern, wide_lds_bytes()));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), wide_lds_bytes(), st, p);
  RF_HIP(hipGetLastError());
  return RF_OK;
}
// the instantiation of k_scan_w16 for the call: the product's, or (experiments build) a diagnostic one
template <int MODE>
static int dispatch_w16(const WideParams& p, int grid, hipStream_t st) {
#ifdef RF_EXPERIMENTS
  // rf_set_tuning("wide_dbg", bits): 1 = every DMA piece re-reads one cached KiB, 2 = no filters, 4 = clock
  // stamps, 8 = no LDS-DMA in the loop (1 | 2 | 8: results wrong)
  if (MODE == MODE_EMIT) {
    switch (rf_knob_wide_dbg) {
      case 20: return launch_w16<MODE_EMIT, 20>(p, grid, st);   // stamps, static priorities (no progress-based s_setprio)
      case 16: return launch_w16<MODE_EMIT, 16>(p, grid, st);   // static priorities
      case 33: return launch_w16<MODE_EMIT, 33>(p, grid, st);   // no operand waits, cached-KiB DMA, no hits
      case 37: return launch_w16<MODE_EMIT, 37>(p, grid, st);   // the same with stamps
      case 62: return launch_w16<MODE_EMIT, 65>(p, grid, st);   // (wide_dbg 62) no operand reads at all, cached-KiB DMA, no hits
      case 63: return launch_w16<MODE_EMIT, 69>(p, grid, st);   // (wide_dbg 63) the same with stamps
      case 61: return launch_w16<MODE_EMIT, 77>(p, grid, st);   // (wide_dbg 61) no reads, no DMA, stamps: MFMAs + filters + barrier only
#define W16_DBG(x) case x: return launch_w16<MODE_EMIT, x>(p, grid, st);
      W16_DBG(1) W16_DBG(4) W16_DBG(8) W16_DBG(5)
#undef W16_DBG
      default: break;
    }
    switch (rf_knob_wide_ne) {   // rf_set_tuning("wide_ne", n): the DMA split between the wave halves; + 100: with clock stamps
#define W16_NEV(n) case n: return launch_w16<MODE_EMIT, 0, n>(p, grid, st); case 100 + n: return launch_w16<MODE_EMIT, 4, n>(p, grid, st);
      W16_NEV(6) W16_NEV(8) W16_NEV(9) W16_NEV(10) W16_NEV(11)
#undef W16_NEV
      default: break;
    }
  }
#endif
  return launch_w16<MODE, 0>(p, grid, st);
}

int rf_launch_wide_sample(const rf_index* ix, const void* q, int B, const rf_workspace& ws, int* P_out,
                          hipStream_t st) {
  const uint32_t nblk = (uint32_t)((ix->size + 31) / 32);
  const uint32_t npair = (nblk + 1) / 2;
  // ~1/16 of the corpus in block pairs, 64..RF_SAMPLE_WGS partitions of up to 4 pairs
  uint32_t n_work = npair / 16;
  if (n_work < 64u) n_work = 64u;
  if (n_work > (uint32_t)RF_SAMPLE_WGS * rf_knob_wide_sample_pairs) n_work = (uint32_t)RF_SAMPLE_WGS * rf_knob_wide_sample_pairs;
  if (n_work > npair) n_work = npair;
  const int grid = (int)(n_work < (uint32_t)RF_SAMPLE_WGS ? n_work : (uint32_t)RF_SAMPLE_WGS);
  WideParams p{};
  p.corpus = ix->tiles;
  p.q = (const _Float16*)q;
  p.B = B;
  p.n_rows = (uint32_t)ix->size;
  p.n_work = n_work;
  p.bstride = npair / n_work;
  p.pmax = ws.pmax;
  p.P = grid;
  *P_out = grid;
  return dispatch_w16<MODE_SAMPLE>(p, grid, st);
}

int rf_launch_wide_emit(const rf_index* ix, const void* q, int B, const rf_workspace& ws, hipStream_t st) {
  const uint32_t nblk = (uint32_t)((ix->size + 31) / 32);
  const uint32_t npair = (nblk + 1) / 2;
  int grid = ix->num_cus;   // one workgroup per CU (all of its LDS)
  if ((uint32_t)grid > npair) grid = (int)npair;
  if (grid < 1) grid = 1;
  WideParams p{};
  p.corpus = ix->tiles;
  p.q = (const _Float16*)q;
  p.B = B;
  p.n_rows = (uint32_t)ix->size;
  p.n_work = npair;
  p.bstride = 1;
  p.thr = ws.thr;
  p.cand_cnt = ws.cand_cnt;
  p.cand = ws.cand;
  p.cap = RF_SHARD_CAP;
  if (rf_knob_wide_dbg & 4) p.pmax = ws.pmax;   // stamp buffer of the diagnostic run
  return dispatch_w16<MODE_EMIT>(p, grid, st);
}
