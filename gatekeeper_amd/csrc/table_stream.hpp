// The pure part of a table's violation stream (gk_table_violations): what a cursor carries, the index over device entries and the pairs
// the host evaluation added, and how the two become one page.  Host only; no HIP and no dependency on the engine
// (tests/native/table_stream_test.cpp runs it under sanitizers).  Pages end where viol_page_end (viol_stream.hpp) says.
//
// An entry is a review with at least one bit, violation or autoreject, in some bitmap row.  The device names the reviews it evaluated
// itself; a review beyond its limits that the host evaluator answered (complete_on_host) has its entry from the (row, review) pairs
// that evaluation left beside the table.  The two kinds never name the same review -- the device masks every review whose too_big bit
// is set -- but nothing here relies on that: a review named by both gets ONE entry with the bits of both.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "viol_stream.hpp"

namespace gk {

// ---- cursor: | stream generation 28 | word 32 |.  The generation is never 0 (viol_next_gen), so no cursor of a stream is 0 ("start").
constexpr uint32_t TABLE_CUR_WORD_BITS = 32;
// 0: the generation does not fit (nothing viol_next_gen produces)
inline uint64_t table_cursor_pack(uint32_t gen, uint32_t word) {
  if (gen == 0 || gen >> VIOL_CUR_GEN_BITS) return 0;
  return ((uint64_t)gen << TABLE_CUR_WORD_BITS) | word;
}
// false: not a cursor of the stream generation `gen_now` over `words` bitmap words
inline bool table_cursor_check(uint64_t cursor, uint32_t gen_now, uint32_t words, uint32_t* word) {
  const uint64_t gen = cursor >> TABLE_CUR_WORD_BITS;
  const uint32_t w = (uint32_t)(cursor & 0xFFFFFFFFull);
  if (gen == 0 || gen_now == 0 || gen != gen_now || w >= words) return false;
  *word = w;
  return true;
}

typedef std::vector<std::pair<uint32_t, uint32_t>> TablePairs;   // (bitmap row, review)

// per bitmap word the reviews (< n_reviews) that a pair of a row below `rows` names
inline std::vector<uint64_t> table_host_words(const TablePairs& viol, const TablePairs& err, uint32_t rows, uint32_t n_reviews) {
  std::vector<uint64_t> words(((size_t)n_reviews + 63u) / 64u, 0);
  for (const TablePairs* p : {&viol, &err})
    for (const auto& hp : *p)
      if (hp.first < rows && hp.second < n_reviews) words[hp.second / 64u] |= 1ull << (hp.second % 64u);
  return words;
}

// The stream's index: prefix[w] = entries before bitmap word w ([words + 1]).  cnt[w] = the device's entries of the word; where the
// host names reviews too (`host`, per word; may be empty), `any` -- the device's reviews as a bit word -- says which of them are new.
// false: the sizes do not belong together.
inline bool table_prefix(const std::vector<uint32_t>& cnt, const std::vector<uint64_t>& any, const std::vector<uint64_t>& host, std::vector<uint64_t>* prefix) {
  const size_t words = cnt.size();
  const bool merged = !host.empty();
  if (merged && (host.size() != words || any.size() != words)) return false;
  prefix->assign(words + 1, 0);
  for (size_t w = 0; w < words; w++)
    (*prefix)[w + 1] = (*prefix)[w] + (merged ? (uint64_t)__builtin_popcountll(any[w] | host[w]) : (uint64_t)cnt[w]);
  return true;
}

// One page: the device's entries of the words [w0, w1) (reviews ascending, masks [entries][mw]) and the host's pairs inside that word
// range become `reviews` (ascending) with their masks.  Pairs of rows at or beyond `rows` and of reviews at or beyond n_reviews are
// dropped.  false: the device's lists do not belong together (sizes, order, a review outside the range).
inline bool table_merge_page(const std::vector<uint32_t>& dev_reviews, const std::vector<uint64_t>& dev_viol, const std::vector<uint64_t>& dev_err, uint32_t mw,
                             const TablePairs& host_viol, const TablePairs& host_err, uint32_t rows, uint32_t n_reviews, uint32_t w0, uint32_t w1,
                             std::vector<uint32_t>* reviews, std::vector<uint64_t>* viol, std::vector<uint64_t>* err) {
  if (dev_viol.size() != dev_reviews.size() * (size_t)mw || dev_err.size() != dev_viol.size()) return false;
  for (size_t i = 0; i < dev_reviews.size(); i++)
    if (dev_reviews[i] / 64u < w0 || dev_reviews[i] / 64u >= w1 || dev_reviews[i] >= n_reviews || (i && dev_reviews[i] <= dev_reviews[i - 1])) return false;
  auto on_page = [&](const std::pair<uint32_t, uint32_t>& hp) { return hp.first < rows && hp.first / 64u < mw && hp.second < n_reviews && hp.second / 64u >= w0 && hp.second / 64u < w1; };
  std::vector<uint32_t> host;
  for (const TablePairs* p : {&host_viol, &host_err})
    for (const auto& hp : *p) if (on_page(hp)) host.push_back(hp.second);
  if (host.empty()) { *reviews = dev_reviews; *viol = dev_viol; *err = dev_err; return true; }
  std::sort(host.begin(), host.end());
  host.erase(std::unique(host.begin(), host.end()), host.end());
  *reviews = viol_merge_slots(dev_reviews, host);
  viol->assign(reviews->size() * (size_t)mw, 0);
  err->assign(reviews->size() * (size_t)mw, 0);
  size_t at = 0;
  for (size_t i = 0; i < dev_reviews.size(); i++) {
    while ((*reviews)[at] != dev_reviews[i]) at++;   // (every device review is in the union)
    for (uint32_t k = 0; k < mw; k++) { (*viol)[at * mw + k] = dev_viol[i * mw + k]; (*err)[at * mw + k] = dev_err[i * mw + k]; }
  }
  for (const auto& hp : host_viol) if (on_page(hp)) (*viol)[viol_find(*reviews, hp.second) * mw + hp.first / 64u] |= 1ull << (hp.first % 64u);
  for (const auto& hp : host_err) if (on_page(hp)) (*err)[viol_find(*reviews, hp.second) * mw + hp.first / 64u] |= 1ull << (hp.first % 64u);
  return true;
}

}  // namespace gk
