// AddressSanitizer / UBSan driver for rag_fin_amd/csrc/analyzer.cpp (the host-side analyzer of the
// lexical index).  Built and run by tests/test_analyzer_sanitizer.py on the CPU:
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=all analyzer.cpp this.cpp
// Input file (little endian): int64 n_punct, int32 punct[n_punct], int64 n, int64 offsets[n + 1],
// text bytes.
// Output file: int64 sizes[4] = { n, n_tokens, n_terms, vocab bytes }, the vocab blob, int64
// vocab_off[n_terms + 1], int32 tok[n_tokens], int64 dl[n].
// Besides the batch it drives the argument-check paths with null / empty / degenerate arguments.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/ragfin.h"

// the library's error sink lives in index.hip (a HIP translation unit): stub for the host-only build
static char g_err[512];
void rf_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static std::vector<char> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> b((size_t)n);
  if (n && fread(b.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
  fclose(f);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s <input> <threads> <output>\n", argv[0]);
    return 2;
  }
  const std::vector<char> in = slurp(argv[1]);
  const int threads = atoi(argv[2]);
  const char* p = in.data();
  int64_t n, np_;
  memcpy(&np_, p, 8); p += 8;
  std::vector<int32_t> punct((size_t)np_);
  if (np_) memcpy(punct.data(), p, (size_t)np_ * 4);
  p += np_ * 4;
  memcpy(&n, p, 8); p += 8;
  std::vector<int64_t> off((size_t)n + 1);
  memcpy(off.data(), p, (size_t)(n + 1) * 8); p += (n + 1) * 8;
  const char* text = p;

  rf_analysis_t* a = nullptr;
  // argument checks first: none of these may touch memory
  if (rf_analyze(text, off.data(), n, punct.data(), (int)np_, threads, nullptr) == RF_OK) return 3;
  if (rf_analyze(text, nullptr, n, punct.data(), (int)np_, threads, &a) == RF_OK || a) return 3;
  if (rf_analyze(text, off.data(), -1, punct.data(), (int)np_, threads, &a) == RF_OK || a) return 3;
  if (rf_analyze(text, off.data(), n, nullptr, 3, threads, &a) == RF_OK || a) return 3;
  if (n >= 2 && off[(size_t)n] > 0) {   // offsets that go down
    std::vector<int64_t> bad(off);
    bad[1] = bad[(size_t)n] + 1;
    if (rf_analyze(text, bad.data(), n, punct.data(), (int)np_, threads, &a) == RF_OK || a) return 3;
  }
  int64_t sizes[4];
  if (rf_analysis_sizes(nullptr, sizes) == RF_OK || rf_analysis_read(nullptr, nullptr, nullptr, nullptr, nullptr) == RF_OK)
    return 3;
  if (rf_analyze(text, off.data(), 0, nullptr, 0, threads, &a) != RF_OK || !a) return 4;   // empty batch
  if (rf_analysis_sizes(a, sizes) != RF_OK || sizes[0] || sizes[1] || sizes[2] || sizes[3]) return 4;
  if (rf_analysis_read(a, nullptr, nullptr, nullptr, nullptr) != RF_OK) return 4;
  rf_analysis_destroy(a);
  a = nullptr;
  if (rf_analyze(text, off.data(), n, punct.data(), (int)np_, threads, &a) != RF_OK || !a) {
    fprintf(stderr, "analyze failed: %s\n", g_err);
    return 4;
  }
  if (rf_analysis_sizes(a, sizes) != RF_OK || sizes[0] != n) return 4;
  std::vector<char> blob((size_t)sizes[3]);
  std::vector<int64_t> voff((size_t)sizes[2] + 1), dl((size_t)n);
  std::vector<int32_t> tok((size_t)sizes[1]);
  if (rf_analysis_read(a, blob.data(), voff.data(), tok.data(), dl.data()) != RF_OK) return 4;
  int64_t total = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (dl[(size_t)i] < 0) return 5;
    total += dl[(size_t)i];
  }
  if (total != sizes[1]) return 5;
  for (int32_t t : tok)
    if (t < 0 || t >= sizes[2]) return 5;
  FILE* f = fopen(argv[3], "wb");
  if (!f) return 2;
  fwrite(sizes, 8, 4, f);
  fwrite(blob.data(), 1, blob.size(), f);
  fwrite(voff.data(), 8, voff.size(), f);
  fwrite(tok.data(), 4, tok.size(), f);
  fwrite(dl.data(), 8, dl.size(), f);
  fclose(f);
  rf_analysis_destroy(a);
  rf_analysis_destroy(nullptr);
  return 0;
}
