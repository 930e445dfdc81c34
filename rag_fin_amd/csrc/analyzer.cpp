// Native analyzer of the lexical index (host code, multi-threaded): texts -> the sorted dictionary,
// the term id of every token and the tokens per text (include/ragfin.h, "analyzer").
//
// The rules are the ASCII rules of tokenizer.cpp without its special tokens and its WordPiece step:
// control characters dropped without splitting on them, " \t\n\r" the whitespace, A-Z lower-cased,
// ASCII punctuation and the registered non-ASCII punctuation split off one character at a time.  The
// division of labour with rag_fin_amd/lexical.py (analyze_native) is the tokenizer's too: Unicode
// tables stay in Python's unicodedata, this file only walks UTF-8 sequences.
//
// Each thread interns a contiguous slice of the texts into a map of its own and keeps local ids; one
// merge sorts the distinct terms by their bytes and gives every thread a local -> global map; the
// slices are rewritten in parallel.  The result is a function of the texts alone.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/ragfin.h"

void rf_set_error(const char* fmt, ...);

struct rf_analysis {
  int64_t n = 0;
  std::string vocab_blob;          // every term followed by '\n'
  std::vector<int64_t> vocab_off;  // [n_terms + 1]
  std::vector<int32_t> tok;        // [n_tokens]
  std::vector<int64_t> dl;         // [n]
};

namespace {
inline bool an_punct(unsigned char c) {
  return (c >= 33 && c <= 47) || (c >= 58 && c <= 64) || (c >= 91 && c <= 96) || (c >= 123 && c <= 126);
}
inline bool an_space(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
inline bool an_dropped(unsigned char c) { return (c < 0x20 && !an_space(c)) || c == 0x7f; }
inline int an_utf8_len(unsigned char lead) {
  return lead < 0x80 ? 1 : (lead >> 5) == 0x6 ? 2 : (lead >> 4) == 0xe ? 3 : (lead >> 3) == 0x1e ? 4 : 1;
}

// one thread's share: texts [first, last), their tokens as local ids
struct Slice {
  int64_t first = 0, last = 0;
  std::unordered_map<std::string, int32_t> ids;
  std::vector<const std::string*> terms;   // local id -> the map's key (stable in an unordered_map)
  std::vector<int32_t> tok;
  std::vector<int32_t> to_global;
  int64_t tok_base = 0;
  bool failed = false;
};

struct Rules {
  std::vector<int32_t> punct;   // sorted
};

inline void emit(Slice& s, std::string& key, const char* p, size_t len) {
  key.assign(p, len);
  auto it = s.ids.find(key);
  int32_t id;
  if (it == s.ids.end()) {
    id = (int32_t)s.terms.size();
    it = s.ids.emplace(key, id).first;
    s.terms.push_back(&it->first);
  } else {
    id = it->second;
  }
  s.tok.push_back(id);
}

// the tokens of one text; returns how many
int64_t analyze_one(const Rules& R, const char* s, size_t n, Slice& out, std::string& word, std::string& key) {
  int64_t count = 0;
  size_t i = 0;
  while (i < n) {
    // next whitespace-delimited word, control characters dropped (they do not separate words)
    while (i < n && (an_space((unsigned char)s[i]) || an_dropped((unsigned char)s[i]))) ++i;
    word.clear();
    while (i < n && !an_space((unsigned char)s[i])) {
      unsigned char c = (unsigned char)s[i];
      if (!an_dropped(c)) word.push_back((char)(c >= 'A' && c <= 'Z' ? c + 32 : c));
      ++i;
    }
    if (word.empty()) continue;
    const char* w = word.data();
    const size_t wn = word.size();
    // the byte length of the punctuation character at p, or 0
    auto punct_len = [&](size_t p) -> size_t {
      const unsigned char c0 = (unsigned char)w[p];
      if (c0 < 0x80) return an_punct(c0) ? 1 : 0;
      if (R.punct.empty()) return 0;
      const int len = an_utf8_len(c0);
      if (len < 2 || p + (size_t)len > wn) return 0;
      int32_t cp = len == 2 ? (c0 & 0x1f) : len == 3 ? (c0 & 0x0f) : (c0 & 0x07);
      for (int q = 1; q < len; ++q) cp = (cp << 6) | ((unsigned char)w[p + q] & 0x3f);
      return std::binary_search(R.punct.begin(), R.punct.end(), cp) ? (size_t)len : 0;
    };
    size_t a = 0;
    while (a < wn) {
      const size_t pl = punct_len(a);
      if (pl) {
        emit(out, key, w + a, pl);
        a += pl;
        ++count;
        continue;
      }
      size_t b = a;
      while (b < wn && !punct_len(b)) b += (size_t)an_utf8_len((unsigned char)w[b]);
      if (b > wn) b = wn;   // a sequence cut short by the end of the word
      emit(out, key, w + a, b - a);
      a = b;
      ++count;
    }
  }
  return count;
}

template <class F>
void run_threads(int nt, F&& body) {
  if (nt <= 1) {
    body(0);
    return;
  }
  std::vector<std::thread> pool;
  pool.reserve((size_t)nt);
  for (int k = 0; k < nt; ++k) pool.emplace_back(body, k);
  for (auto& th : pool) th.join();
}
}  // namespace

extern "C" int rf_analyze(const char* text_bytes, const int64_t* offsets, int64_t n, const int32_t* punct_cps, int n_punct,
                          int n_threads, rf_analysis_t** out) {
  if (!out) {
    rf_set_error("rf_analyze: out is NULL");
    return RF_ERR_INVALID;
  }
  *out = nullptr;
  if (!offsets || n < 0 || n >= ((int64_t)1 << 31) || n_punct < 0 || (n_punct > 0 && !punct_cps) ||
      (n > 0 && !text_bytes && offsets[n] > offsets[0])) {
    rf_set_error("rf_analyze: bad argument (offsets, 0 <= n < 2^31, punct_cps with n_punct > 0, text_bytes)");
    return RF_ERR_INVALID;
  }
  if (n > 0 && offsets[0] < 0) {
    rf_set_error("rf_analyze: offsets start below 0");
    return RF_ERR_INVALID;
  }
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) {
      rf_set_error("rf_analyze: offsets not monotone at %lld", (long long)i);
      return RF_ERR_INVALID;
    }
  int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > 64) nt = 64;
  if ((int64_t)nt > (n + 63) / 64) nt = (int)std::max<int64_t>(1, (n + 63) / 64);   // at least ~64 texts per thread
  try {
    Rules R;
    if (n_punct > 0) R.punct.assign(punct_cps, punct_cps + n_punct);
    std::sort(R.punct.begin(), R.punct.end());
    std::unique_ptr<rf_analysis> A(new rf_analysis());
    A->n = n;
    A->dl.assign((size_t)n, 0);
    std::vector<Slice> slices((size_t)nt);
    // slices of about equal bytes, each a whole number of texts
    {
      const int64_t b0 = n ? offsets[0] : 0, total = n ? offsets[n] - b0 : 0;
      int64_t at = 0;
      for (int k = 0; k < nt; ++k) {
        slices[(size_t)k].first = at;
        if (k == nt - 1) {
          at = n;
        } else {
          const int64_t want = b0 + total / nt * (k + 1);
          at = std::lower_bound(offsets + at, offsets + n, want) - offsets;
        }
        slices[(size_t)k].last = at;
      }
    }
    run_threads(nt, [&](int k) {
      Slice& s = slices[(size_t)k];
      try {
        std::string word, key;
        for (int64_t i = s.first; i < s.last; ++i)
          A->dl[(size_t)i] = analyze_one(R, text_bytes + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), s, word, key);
      } catch (...) {
        s.failed = true;
      }
    });
    for (auto& s : slices)
      if (s.failed) throw std::bad_alloc();
    // the merge: the distinct terms of every slice, sorted by their bytes (std::string compares as unsigned char)
    std::unordered_map<std::string, int32_t> global;
    std::vector<const std::string*> terms;
    for (auto& s : slices)
      for (const std::string* t : s.terms)
        if (global.emplace(*t, 0).second) terms.push_back(t);
    if (terms.size() >= ((size_t)1 << 31)) {
      rf_set_error("rf_analyze: more than 2^31 - 1 distinct terms");
      return RF_ERR_INVALID;
    }
    std::sort(terms.begin(), terms.end(), [](const std::string* a, const std::string* b) { return *a < *b; });
    size_t blob_bytes = 0;
    for (const std::string* t : terms) blob_bytes += t->size() + 1;
    A->vocab_blob.reserve(blob_bytes);
    A->vocab_off.reserve(terms.size() + 1);
    for (size_t g = 0; g < terms.size(); ++g) {
      global[*terms[g]] = (int32_t)g;
      A->vocab_off.push_back((int64_t)A->vocab_blob.size());
      A->vocab_blob.append(*terms[g]);
      A->vocab_blob.push_back('\n');
    }
    A->vocab_off.push_back((int64_t)A->vocab_blob.size());
    int64_t n_tokens = 0;
    for (auto& s : slices) {
      s.tok_base = n_tokens;
      n_tokens += (int64_t)s.tok.size();
      s.to_global.resize(s.terms.size());
      for (size_t l = 0; l < s.terms.size(); ++l) s.to_global[l] = global.find(*s.terms[l])->second;
    }
    A->tok.resize((size_t)n_tokens);
    run_threads(nt, [&](int k) {
      const Slice& s = slices[(size_t)k];
      int32_t* dst = A->tok.data() + s.tok_base;
      for (size_t j = 0; j < s.tok.size(); ++j) dst[j] = s.to_global[(size_t)s.tok[j]];
    });
    *out = A.release();
    return RF_OK;
  } catch (...) {
    rf_set_error("rf_analyze: out of host memory");
    return RF_ERR_CAPACITY;   // not a bad argument: the caller may retry with fewer texts
  }
}

extern "C" int rf_analysis_sizes(const rf_analysis_t* a, int64_t* sizes4) {
  if (!a || !sizes4) {
    rf_set_error("rf_analysis_sizes: null argument");
    return RF_ERR_INVALID;
  }
  sizes4[0] = a->n;
  sizes4[1] = (int64_t)a->tok.size();
  sizes4[2] = (int64_t)a->vocab_off.size() - 1;
  sizes4[3] = (int64_t)a->vocab_blob.size();
  return RF_OK;
}

extern "C" int rf_analysis_read(const rf_analysis_t* a, char* vocab_blob, int64_t* vocab_off, int32_t* tok, int64_t* dl) {
  if (!a) {
    rf_set_error("rf_analysis_read: null handle");
    return RF_ERR_INVALID;
  }
  if (vocab_blob && !a->vocab_blob.empty()) memcpy(vocab_blob, a->vocab_blob.data(), a->vocab_blob.size());
  if (vocab_off) memcpy(vocab_off, a->vocab_off.data(), a->vocab_off.size() * sizeof(int64_t));
  if (tok && !a->tok.empty()) memcpy(tok, a->tok.data(), a->tok.size() * sizeof(int32_t));
  if (dl && !a->dl.empty()) memcpy(dl, a->dl.data(), a->dl.size() * sizeof(int64_t));
  return RF_OK;
}

extern "C" int rf_analysis_destroy(rf_analysis_t* a) {
  delete a;
  return RF_OK;
}
