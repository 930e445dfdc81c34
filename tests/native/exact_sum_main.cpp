// Driver of tests/test_exact_sum_native.py: runs the fixed-point accumulator of rag_fin_amd/csrc/exact_sum.h --
// the text the device kernels compile -- over groups of values on the host, under ASan + UBSan.
//   exact_sum_main IN OUT
// IN:  int64 n_groups, then per group { int64 is_f64, int64 n, n values of 8 bytes (fp64 bits, or int64) }
// OUT: per group RF_STATS_OUT int64 words, es_finish's compact result
#include <cstdint>
#include <cstdio>
#include <vector>

#include "exact_sum.h"

static bool read_words(FILE* f, int64_t* dst, size_t n) { return fread(dst, 8, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "cannot open the files\n");
    return 2;
  }
  int64_t n_groups = 0;
  if (!read_words(in, &n_groups, 1) || n_groups < 0) return 3;
  for (int64_t g = 0; g < n_groups; ++g) {
    int64_t head[2];
    if (!read_words(in, head, 2) || head[1] < 0) return 3;
    std::vector<int64_t> values((size_t)head[1]);
    if (head[1] && !read_words(in, values.data(), values.size())) return 3;
    std::vector<int64_t> rec(RF_STATS_WORDS, 0);
    int64_t* w = rec.data();
    auto add = [w](int word, int64_t delta) { w[word] = (int64_t)((uint64_t)w[word] + (uint64_t)delta); };
    auto max = [w](int word, uint64_t key) {
      if (key > (uint64_t)w[word]) w[word] = (int64_t)key;
    };
    for (int64_t v : values) {
      if (head[0]) es_accumulate_f64((uint64_t)v, add, max);
      else es_accumulate_i64(v, add, max);
    }
    int64_t res[RF_STATS_OUT];
    es_finish(w, (int)head[0], res);
    if (fwrite(res, 8, RF_STATS_OUT, out) != RF_STATS_OUT) return 4;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
