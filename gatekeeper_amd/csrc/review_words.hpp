// Review words: the predicate classes of a plan whose whole effect is OR-ing bits into the plan's GLOBAL words of the row's review
// (every predicate has dst == D_GLOBAL: no stored value, no element marker, no element word).  What such a class leaves in the
// accumulators depends on the table's rows and on the plan alone -- both fixed for as long as a binding lives -- so the sweep need not
// walk its chunks again every time: the binding evaluates them ONCE into rwords[K][n_pad] (kernels.hip gk_bind_review_words), the chunk
// lists of the plan-specialised kernel leave them out, and the kernel ORs the K words of a review into its accumulators behind the
// chunk loop (the body variant of embed_sources.py).  Host-only and free of HIP: the GPU-less tests run the analysis and the list
// filter as they are (tests/native/review_words_test.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "chunks.hpp"
#include "plan.hpp"

namespace gk {

struct ReviewWords {
  std::vector<uint8_t> hoisted;   // [class id] (1-based, as jit_path_classes numbers them): 1 = a review-word class
  std::vector<uint32_t> words;    // the global words the hoisted classes can write, ascending: slot k of rwords holds words[k]
  uint32_t k() const { return (uint32_t)words.size(); }
  bool is_hoisted(uint32_t cls) const { return cls < hoisted.size() && hoisted[cls] != 0; }
  int slot_of(uint32_t word) const {
    for (size_t i = 0; i < words.size(); i++) if (words[i] == word) return (int)i;
    return -1;
  }
};

constexpr uint32_t GK_RW_MAX_WORD = 32;   // global words a review-word class may write: the binding kernel takes the word -> slot table as an argument

// classes: what jit_path_classes returns in *classes (entry 0 is empty).  A class with a bit beyond the plan's global words (no plan
// has one: the words are counted from the bits) or beyond GK_RW_MAX_WORD is left alone.
inline ReviewWords analyse_review_words(const std::vector<std::vector<Pred>>& classes, uint32_t n_gwords) {
  n_gwords = std::min(n_gwords, GK_RW_MAX_WORD);
  ReviewWords rw;
  rw.hoisted.assign(classes.size(), 0);
  for (size_t c = 1; c < classes.size(); c++) {
    bool all = !classes[c].empty();
    for (const Pred& p : classes[c]) all = all && p.dst == D_GLOBAL && p.op != P_STORE && p.op != P_PRESENT && (uint32_t)(p.bit >> 5) < n_gwords;
    if (!all) continue;
    rw.hoisted[c] = 1;
    for (const Pred& p : classes[c]) rw.words.push_back((uint32_t)(p.bit >> 5));
  }
  std::sort(rw.words.begin(), rw.words.end());
  rw.words.erase(std::unique(rw.words.begin(), rw.words.end()), rw.words.end());
  return rw;
}

// the bound paths the sweep keeps (kept) and the ones the binding pass evaluates (hoisted); ent = class id | GK_ENT_NEEDS_STR
inline void split_bound(const std::vector<BoundPath>& bound, const ReviewWords& rw, std::vector<BoundPath>* kept, std::vector<BoundPath>* hoisted) {
  for (const BoundPath& b : bound) {
    if (rw.is_hoisted(b.ent & ~GK_ENT_NEEDS_STR)) { if (hoisted) hoisted->push_back(b); }
    else if (kept) kept->push_back(b);
  }
}

// GK_REVIEW_WORDS=0: off (A/B aid: the parent's text and lists).  GK_REVIEW_WORDS_MIN=<n>: the table size from which the variant is
// asked for (default 8192: the size from which a table gets 256-review groups by itself; the tests lower it).
inline bool review_words_enabled() {
  static const bool on = !(getenv("GK_REVIEW_WORDS") && atoi(getenv("GK_REVIEW_WORDS")) == 0);
  return on;
}
inline uint32_t review_words_min_reviews() {
  static const uint32_t n = getenv("GK_REVIEW_WORDS_MIN") ? (uint32_t)atoll(getenv("GK_REVIEW_WORDS_MIN")) : 8192u;
  return n;
}
inline bool review_words_wanted(const ReviewWords& rw, uint32_t rpt, uint32_t n_reviews) {
  return review_words_enabled() && rw.k() > 0 && rpt >= 128u && n_reviews >= review_words_min_reviews();
}

}  // namespace gk
