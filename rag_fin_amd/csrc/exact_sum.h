// Exact sums of doubles in fixed point (include/ragfin.h, "metric aggregations").
//
// A finite double is a 53-bit integer times a power of two, so the exact sum of any number of doubles is an
// integer multiple of 2^-1074 below 2^(1024 + 31): it fits a fixed-point accumulator of 66 limbs of 32 bits.
// The limbs are kept in int64 words, so that adding a value is three integer adds without a carry -- they
// commute, and the accumulator does not depend on the order of the adds -- and the carries are propagated
// once, at the end, before ONE rounding to the nearest double (ties to even).  The device kernels
// (facet_stats.hip) and the host test (tests/native/exact_sum_main.cpp) compile this same text.
//
// A record of RF_STATS_WORDS int64 words:
//   [0, 66)  limb j holds the weight 2^(32 j - 1074)
//   66       count: the non-NaN values        67  nan: the NaN values
//   68       +inf values                      69  -inf values
//   70       min: the largest COMPLEMENT of an order-preserving key    71  max: the largest key
//            (unsigned compares; a zeroed record is the identity of both)
// A finite double with biased exponent E and significand M (53 bits, without the implicit bit when E == 0)
// is M * 2^(p - 1074) with p = max(E, 1) - 1: M << (p & 31) has at most 84 bits and is cut into three pieces
// below 2^32 that go, negated for a negative value, to limbs p >> 5, + 1, + 2 (p <= 2045: the last limb is
// 65).  An int64 value adds its low 32 bits (unsigned) to limb 0 and its high 32 bits (signed) to limb 1.
// Every piece is below 2^32 in magnitude and a limb takes one piece per value, so a limb stays inside an
// int64 for fewer than 2^31 values.
#ifndef RF_EXACT_SUM_H
#define RF_EXACT_SUM_H
#include <stdint.h>

#ifdef __HIPCC__
#define ES_FN __host__ __device__ inline
#else
#define ES_FN inline
#endif

#define ES_LIMBS 66
#define ES_COUNT 66
#define ES_NAN 67
#define ES_PINF 68
#define ES_NINF 69
#define ES_MIN 70
#define ES_MAX 71
#ifndef RF_STATS_WORDS
#define RF_STATS_WORDS 72   // (include/ragfin.h says the same)
#endif

#define ES_CLASS_FINITE 0
#define ES_CLASS_NAN 1
#define ES_CLASS_PINF 2
#define ES_CLASS_NINF 3

// The class of a double from its bits; for a finite one its first limb, its three pieces and its sign.
ES_FN int es_split_f64(uint64_t bits, int* limb, uint32_t piece[3], int* negative) {
  const uint32_t E = (uint32_t)(bits >> 52) & 0x7FFu;
  const uint64_t frac = bits & 0x000FFFFFFFFFFFFFull;
  *negative = (int)(bits >> 63);
  if (E == 0x7FFu) return frac ? ES_CLASS_NAN : (*negative ? ES_CLASS_NINF : ES_CLASS_PINF);
  const uint64_t M = E ? frac | (1ull << 52) : frac;
  const uint32_t p = (E ? E : 1u) - 1u;
  const uint32_t s = p & 31u;
  *limb = (int)(p >> 5);
  piece[0] = (uint32_t)(M << s);               // bits [0, 32) of M << s
  const uint64_t rest = (M >> 1) >> (31u - s);   // M >> (32 - s), also for s == 0
  piece[1] = (uint32_t)rest;
  piece[2] = (uint32_t)(rest >> 32);           // below 2^21
  return ES_CLASS_FINITE;
}

// order-preserving keys: a < b as values  <=>  key(a) < key(b) as unsigned (fp64: no NaN comes here)
ES_FN uint64_t es_key_i64(int64_t x) { return (uint64_t)x ^ (1ull << 63); }
ES_FN uint64_t es_key_f64_bits(uint64_t b) { return (b >> 63) ? ~b : b | (1ull << 63); }
ES_FN uint64_t es_unkey_i64(uint64_t k) { return k ^ (1ull << 63); }
ES_FN uint64_t es_unkey_f64_bits(uint64_t k) { return (k >> 63) ? k ^ (1ull << 63) : ~k; }

// Adds one value into a record through add(word, delta) and max(word, key): plain in a host test, atomics on
// the device.  Both take the word's index in the record.
template <typename Add, typename Max>
ES_FN void es_accumulate_f64(uint64_t bits, Add add, Max max) {
  int limb, negative;
  uint32_t piece[3];
  const int c = es_split_f64(bits, &limb, piece, &negative);
  if (c == ES_CLASS_NAN) {
    add(ES_NAN, (int64_t)1);
    return;
  }
  add(ES_COUNT, (int64_t)1);
  const uint64_t key = es_key_f64_bits(bits);
  max(ES_MIN, ~key);
  max(ES_MAX, key);
  if (c != ES_CLASS_FINITE) {
    add(c == ES_CLASS_PINF ? ES_PINF : ES_NINF, (int64_t)1);
    return;
  }
  for (int i = 0; i < 3; ++i)
    if (piece[i]) add(limb + i, negative ? -(int64_t)piece[i] : (int64_t)piece[i]);
}

template <typename Add, typename Max>
ES_FN void es_accumulate_i64(int64_t x, Add add, Max max) {
  add(ES_COUNT, (int64_t)1);
  const uint64_t key = es_key_i64(x);
  max(ES_MIN, ~key);
  max(ES_MAX, key);
  const int64_t lo = (int64_t)((uint64_t)x & 0xFFFFFFFFull), hi = x >> 32;   // x == lo + hi * 2^32
  if (lo) add(0, lo);
  if (hi) add(1, hi);
}

// bits [at, at + 64) of the magnitude held as one 32-bit digit per word w[0 .. n) (at >= 0)
ES_FN uint64_t es_window(const int64_t* w, int n, int at) {
  const int j = at >> 5, s = at & 31;
  const uint64_t d0 = j < n ? (uint64_t)w[j] : 0ull;
  const uint64_t d1 = j + 1 < n ? (uint64_t)w[j + 1] : 0ull;
  const uint64_t d2 = j + 2 < n ? (uint64_t)w[j + 2] : 0ull;
  uint64_t v = (d0 | (d1 << 32)) >> s;
  if (s) v |= d2 << (64 - s);
  return v;
}

// The limbs of a record -> the bits of the exact sum rounded once to the nearest double, ties to even;
// +-inf beyond the double range, +0.0 for an exact zero.  Works in place: afterwards w[0 .. 66) hold the
// magnitude's 32-bit digits (the top one up to 64 bits).  Below 2^-1022 nothing is rounded: every sum is a
// multiple of 2^-1074.
ES_FN uint64_t es_round_limbs(int64_t* w) {
  // carries: digit = (limb + carry) mod 2^32, carry = floor((limb + carry) / 2^32), without leaving int64
  int64_t carry = 0;
  for (int j = 0; j < ES_LIMBS - 1; ++j) {
    const int64_t lo = (int64_t)((uint64_t)w[j] & 0xFFFFFFFFull), hi = w[j] >> 32;
    const int64_t t = lo + carry;
    w[j] = (int64_t)((uint64_t)t & 0xFFFFFFFFull);
    carry = hi + (t >> 32);
  }
  int64_t top = w[ES_LIMBS - 1] + carry;   // (a piece of the last limb is below 2^18: no overflow)
  const int negative = top < 0;
  if (negative) {   // the magnitude: complement the digits, add one
    uint64_t c = 1ull;
    for (int j = 0; j < ES_LIMBS - 1; ++j) {
      const uint64_t d = (~(uint64_t)w[j] & 0xFFFFFFFFull) + c;
      w[j] = (int64_t)(d & 0xFFFFFFFFull);
      c = d >> 32;
    }
    top = (int64_t)(~(uint64_t)top + c);
  }
  // the top word may hold more than 32 bits: spread it over two digits (a 67th lives in `extra`)
  const uint64_t utop = (uint64_t)top;
  w[ES_LIMBS - 1] = (int64_t)(utop & 0xFFFFFFFFull);
  const uint64_t extra = utop >> 32;
  // the highest set bit B of the magnitude (digit 66 is `extra`)
  int B = -1;
  if (extra) {
    B = 32 * ES_LIMBS + 63 - __builtin_clzll(extra);
  } else {
    for (int j = ES_LIMBS - 1; j >= 0; --j) {
      const uint32_t d = (uint32_t)w[j];
      if (d) {
        B = 32 * j + 31 - __builtin_clz(d);
        break;
      }
    }
  }
  const uint64_t sign = negative ? (1ull << 63) : 0ull;
  if (B < 0) return 0ull;   // an exact zero is +0.0
  if (B <= 52) return sign | es_window(w, ES_LIMBS, 0);   // subnormal, or exponent 1: the magnitude is the bits
  if (B >= 32 * ES_LIMBS) return sign | 0x7FF0000000000000ull;   // (beyond 2^1038: far past the double range)
  uint64_t mant = es_window(w, ES_LIMBS, B - 52) & ((1ull << 53) - 1ull);
  const int g = B - 53;   // the guard bit; sticky: any bit below it
  const int guard = (int)((es_window(w, ES_LIMBS, g) & 1ull));
  int sticky = 0;
  for (int j = 0; j < (g >> 5) && !sticky; ++j) sticky = w[j] != 0;
  if (!sticky && (g & 31)) sticky = ((uint64_t)w[g >> 5] & ((1ull << (g & 31)) - 1ull)) != 0ull;
  if (guard && (sticky || (mant & 1ull))) ++mant;
  int E = B - 51;   // the biased exponent: p = E - 1 = B - 52
  if (mant >> 53) {
    mant >>= 1;
    ++E;
  }
  if (E >= 0x7FF) return sign | 0x7FF0000000000000ull;
  return sign | ((uint64_t)E << 52) | (mant & 0x000FFFFFFFFFFFFFull);
}

// The sum of a finished fp64 record: the inf / NaN rule, else the rounded limbs.
ES_FN uint64_t es_sum_bits(int64_t* w) {
  if (w[ES_PINF] && w[ES_NINF]) return 0x7FF8000000000000ull;
  if (w[ES_PINF]) return 0x7FF0000000000000ull;
  if (w[ES_NINF]) return 0xFFF0000000000000ull;
  return es_round_limbs(w);
}

// A record -> its compact result of RF_STATS_OUT words: { count, nan, the sum's bits, 0, min, max, 0, 0 } for an
// fp64 metric (min / max as the values' own bits), { count, 0, limb 0, limb 1, min, max, 0, 0 } for an int64
// one (the sum is limb 0 + limb 1 * 2^32, formed by the host: it may exceed 64 bits).  min / max are
// undefined when count == 0.  The record's limbs are consumed.
#ifndef RF_STATS_OUT
#define RF_STATS_OUT 8
#endif
ES_FN void es_finish(int64_t* w, int is_f64, int64_t* out) {
  const uint64_t kmin = ~(uint64_t)w[ES_MIN], kmax = (uint64_t)w[ES_MAX];
  out[0] = w[ES_COUNT];
  out[1] = w[ES_NAN];
  if (is_f64) {
    out[4] = (int64_t)es_unkey_f64_bits(kmin);
    out[5] = (int64_t)es_unkey_f64_bits(kmax);
    out[2] = (int64_t)es_sum_bits(w);
    out[3] = 0;
  } else {
    out[2] = w[0];
    out[3] = w[1];
    out[4] = (int64_t)es_unkey_i64(kmin);
    out[5] = (int64_t)es_unkey_i64(kmax);
  }
  out[6] = out[7] = 0;
}
#endif /* RF_EXACT_SUM_H */
