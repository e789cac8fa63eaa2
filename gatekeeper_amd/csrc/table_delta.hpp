// The pure part of a table's changes stream (gk_table_changes): how the objects of two list-based audit cycles are lined up by key, how
// the bitmap rows of two constraint sets are, what a cursor over the two sides of a stream carries, the index over device entries and
// the reviews only the host knows, and how a page's device entries take those reviews' masks.  Host only; no HIP and no dependency on
// the engine (tests/native/table_delta_test.cpp runs it under sanitizers).  Pages end where viol_page_end (viol_stream.hpp) says.
//
// Side 0 of a stream is the table NOW (entries ascending by review), side 1 the snapshot's reviews that no review of the table matches
// (GONE; ascending by the snapshot's review index).  A review is HOST-KNOWN when the masks of one of its sides do not lie in a bitmap:
// the host evaluation answered it (now, or in the cycle the snapshot was taken of).  The device is told to leave such reviews alone
// (`drop`) and to emit those the host decided have an entry (`extra`); the page then takes the host's masks for them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string_view>
#include <utility>
#include <vector>

#include "table_stream.hpp"

namespace gk {

constexpr uint32_t DELTA_NONE = 0xFFFFFFFFu;

// ---- the key join.  order_x = the reviews of side x stably sorted by key (table_key_order: equal keys in review order), key_x(i) the
// key of review i.  then_of[i] = the snapshot review that review i of the table continues (DELTA_NONE: new), now_of[p] the inverse
// (DELTA_NONE: gone), unmatched = the gone reviews as bit words.  The i-th occurrence of a key matches the i-th on the other side; an
// empty key matches nothing.
template <class KeyNow, class KeyThen>
inline void delta_join(const std::vector<uint32_t>& order_now, KeyNow&& key_now, const std::vector<uint32_t>& order_then, KeyThen&& key_then,
                       std::vector<uint32_t>* then_of, std::vector<uint32_t>* now_of, std::vector<uint64_t>* unmatched) {
  const size_t nn = order_now.size(), nt = order_then.size();
  then_of->assign(nn, DELTA_NONE);
  now_of->assign(nt, DELTA_NONE);
  unmatched->assign((nt + 63u) / 64u, 0);
  size_t i = 0, j = 0;
  while (i < nn && j < nt) {
    const std::string_view a = key_now(order_now[i]), b = key_then(order_then[j]);
    if (a.empty()) { i++; continue; }
    if (b.empty()) { j++; continue; }
    const int c = a.compare(b);
    if (c < 0) i++;
    else if (c > 0) j++;
    else { (*then_of)[order_now[i]] = order_then[j]; (*now_of)[order_then[j]] = order_now[i]; i++; j++; }
  }
  for (size_t p = 0; p < nt; p++) if ((*now_of)[p] == DELTA_NONE) (*unmatched)[p / 64u] |= 1ull << (p % 64u);
}

// ---- the row map: row_of[now row] = the snapshot's row of the same constraint id (DELTA_NONE: the id is new), and its inverse
inline void delta_row_map(const std::vector<uint32_t>& ids_now, const std::vector<uint32_t>& ids_then, std::vector<uint32_t>* row_of, std::vector<uint32_t>* now_row_of) {
  std::vector<std::pair<uint32_t, uint32_t>> then;   // (id, row)
  for (uint32_t r = 0; r < ids_then.size(); r++) then.emplace_back(ids_then[r], r);
  std::sort(then.begin(), then.end());
  row_of->assign(ids_now.size(), DELTA_NONE);
  now_row_of->assign(ids_then.size(), DELTA_NONE);
  for (uint32_t r = 0; r < ids_now.size(); r++) {
    const auto it = std::lower_bound(then.begin(), then.end(), std::make_pair(ids_now[r], 0u));
    if (it == then.end() || it->first != ids_now[r] || (*now_row_of)[it->second] != DELTA_NONE) continue;   // (an id listed twice: its first row)
    (*row_of)[r] = it->second;
    (*now_row_of)[it->second] = r;
  }
}

// ---- cursor: | stream generation 28 | side 1 | word 31 |.  The generation is never 0 (viol_next_gen), so no cursor of a stream is 0.
constexpr uint32_t DELTA_CUR_WORD_BITS = 31;
inline uint64_t delta_cursor_pack(uint32_t gen, uint32_t side, uint32_t word) {
  if (gen == 0 || gen >> VIOL_CUR_GEN_BITS || side > 1u || word >> DELTA_CUR_WORD_BITS) return 0;
  return ((uint64_t)gen << 32) | ((uint64_t)side << DELTA_CUR_WORD_BITS) | word;
}
// false: not a cursor of the stream generation `gen_now` over words[side] bitmap words
inline bool delta_cursor_check(uint64_t cursor, uint32_t gen_now, const uint32_t words[2], uint32_t* side, uint32_t* word) {
  const uint64_t gen = cursor >> 32;
  const uint32_t s = (uint32_t)(cursor >> DELTA_CUR_WORD_BITS) & 1u, w = (uint32_t)cursor & ((1u << DELTA_CUR_WORD_BITS) - 1u);
  if (gen == 0 || gen_now == 0 || gen != gen_now || w >= words[s]) return false;
  *side = s; *word = w;
  return true;
}

// ---- the index of one side.  `dev` = the device's changed words, `drop` the host-known reviews, `extra` those of them that have an
// entry (both may be empty: none).  entries[w] = (dev & ~drop) | extra -- what the device emits when it is given the same two words --
// and prefix[w] = entries before word w ([words + 1]).  false: the sizes do not belong together, or extra names a review outside drop.
inline bool delta_prefix(const std::vector<uint64_t>& dev, const std::vector<uint64_t>& drop, const std::vector<uint64_t>& extra, std::vector<uint64_t>* entries,
                         std::vector<uint64_t>* prefix) {
  const size_t words = dev.size();
  if ((!drop.empty() && drop.size() != words) || (!extra.empty() && extra.size() != words)) return false;
  entries->assign(words, 0);
  prefix->assign(words + 1, 0);
  for (size_t w = 0; w < words; w++) {
    const uint64_t d = drop.empty() ? 0ull : drop[w], x = extra.empty() ? 0ull : extra[w];
    if (x & ~d) return false;
    (*entries)[w] = (dev[w] & ~d) | x;
    (*prefix)[w + 1] = (*prefix)[w] + (uint64_t)__builtin_popcountll((*entries)[w]);
  }
  return true;
}

// where a stream goes on: the first word with entries at or after (side, word), side 0 before side 1; false: the stream has ended
inline bool delta_next(const std::vector<uint64_t> prefix[2], uint32_t* side, uint32_t* word) {
  for (uint32_t s = *side, w = *word; s < 2u; s++, w = 0) {
    const uint32_t words = prefix[s].empty() ? 0u : (uint32_t)(prefix[s].size() - 1), nx = viol_next_word(prefix[s], w);
    if (nx < words) { *side = s; *word = nx; return true; }
  }
  return false;
}

// ---- host-known reviews: per review of a side what the host knows of its masks ([mw] words each, in the table's row order NOW)
struct DeltaKnown {
  bool now = false, was = false;          // the side's masks are the host's (else: the device's, filled in by delta_known_fill)
  std::vector<uint64_t> nv, ne, wv, we;   // viol / err now, viol / err then
};
typedef std::map<uint32_t, DeltaKnown> DeltaKnownMap;

inline DeltaKnown& delta_known_at(DeltaKnownMap* m, uint32_t review, uint32_t mw) {
  DeltaKnown& k = (*m)[review];
  if (k.nv.empty()) { k.nv.assign(mw, 0); k.ne.assign(mw, 0); k.wv.assign(mw, 0); k.we.assign(mw, 0); }
  return k;
}
// The two sides' maps.  now_done / then_done = the reviews the host evaluation answered (whatever it found); the pairs are
// (bitmap row, review) of that cycle.  then_of / now_of: delta_join's; now_row_of: delta_row_map's (a snapshot row whose id is no longer
// loaded is dropped).  A snapshot review that continues in the table goes into `now` under the table's review; a gone one into `gone`.
inline void delta_known_build(const std::vector<uint32_t>& now_done, const TablePairs& now_viol, const TablePairs& now_err, uint32_t n_now, uint32_t rows_now,
                              const std::vector<uint32_t>& then_done, const TablePairs& then_viol, const TablePairs& then_err,
                              const std::vector<uint32_t>& now_of, const std::vector<uint32_t>& now_row_of, DeltaKnownMap* now, DeltaKnownMap* gone) {
  const uint32_t mw = (rows_now + 63u) / 64u;
  now->clear(); gone->clear();
  for (uint32_t r : now_done) if (r < n_now) delta_known_at(now, r, mw).now = true;
  for (int kind = 0; kind < 2; kind++)
    for (const auto& hp : kind ? now_err : now_viol) {
      const auto it = now->find(hp.second);
      if (it == now->end() || !it->second.now || hp.first >= rows_now) continue;   // (a pair of a review the evaluation did not answer: none of it)
      (kind ? it->second.ne : it->second.nv)[hp.first / 64u] |= 1ull << (hp.first % 64u);
    }
  auto then_at = [&](uint32_t p) -> DeltaKnown* {
    if (p >= now_of.size()) return nullptr;
    return now_of[p] == DELTA_NONE ? &delta_known_at(gone, p, mw) : now_of[p] < n_now ? &delta_known_at(now, now_of[p], mw) : nullptr;
  };
  for (uint32_t p : then_done) if (DeltaKnown* k = then_at(p)) k->was = true;
  for (int kind = 0; kind < 2; kind++)
    for (const auto& hp : kind ? then_err : then_viol) {
      if (hp.second >= now_of.size() || !std::binary_search(then_done.begin(), then_done.end(), hp.second)) continue;
      if (hp.first >= now_row_of.size() || now_row_of[hp.first] == DELTA_NONE) continue;
      DeltaKnown* k = then_at(hp.second);
      const uint32_t row = now_row_of[hp.first];
      if (k && row < rows_now) (kind ? k->we : k->wv)[row / 64u] |= 1ull << (row % 64u);
    }
}

// the known reviews as bit words of a side of `words` words
inline std::vector<uint64_t> delta_known_words(const DeltaKnownMap& m, uint32_t words) {
  std::vector<uint64_t> out(words, 0);
  for (const auto& kv : m) if (kv.first / 64u < words) out[kv.first / 64u] |= 1ull << (kv.first % 64u);
  return out;
}

// The device's entries of some words (reviews ascending, four masks [entries][mw]) give the known reviews among them the masks of the
// sides the host does not know; false: the lists do not belong together.
inline bool delta_known_fill(DeltaKnownMap* m, const std::vector<uint32_t>& reviews, uint32_t mw, const std::vector<uint64_t>& viol, const std::vector<uint64_t>& err,
                             const std::vector<uint64_t>& was_viol, const std::vector<uint64_t>& was_err) {
  const size_t words = reviews.size() * (size_t)mw;
  if (viol.size() != words || err.size() != words || was_viol.size() != words || was_err.size() != words) return false;
  for (size_t i = 0; i < reviews.size(); i++) {
    const auto it = m->find(reviews[i]);
    if (it == m->end()) continue;
    DeltaKnown& k = it->second;
    if (k.nv.size() != mw) return false;
    for (uint32_t j = 0; j < mw; j++) {
      if (!k.now) { k.nv[j] = viol[i * mw + j]; k.ne[j] = err[i * mw + j]; }
      if (!k.was) { k.wv[j] = was_viol[i * mw + j]; k.we[j] = was_err[i * mw + j]; }
    }
  }
  return true;
}

// Which known reviews have an entry, as bit words: the masks differ, or the review is in `moved` (matched, versions given on both sides
// and different) and has a result now.  `unanswered` = the reviews beyond the limits now that no host evaluation answered (the device's
// too_big words without the reviews of now_done): never an entry.  Both word lists may be empty.
inline std::vector<uint64_t> delta_known_decide(const DeltaKnownMap& m, uint32_t words, const std::vector<uint64_t>& moved, const std::vector<uint64_t>& unanswered) {
  std::vector<uint64_t> out(words, 0);
  for (const auto& kv : m) {
    const uint32_t w = kv.first / 64u;
    const uint64_t bit = 1ull << (kv.first % 64u);
    if (w >= words || (!unanswered.empty() && (unanswered[w] & bit))) continue;
    const DeltaKnown& k = kv.second;
    bool any = false, differs = false;
    for (size_t j = 0; j < k.nv.size(); j++) { any = any || k.nv[j] || k.ne[j]; differs = differs || k.nv[j] != k.wv[j] || k.ne[j] != k.we[j]; }
    if (differs || (any && !moved.empty() && (moved[w] & bit))) out[w] |= bit;
  }
  return out;
}

// One page: the device's entries of the words [w0, w1) of a side -- which the device emitted under the side's drop / extra words -- with
// the masks of the known reviews replaced by what the map holds.  false: the lists do not belong together (sizes, order, a review
// outside the range or beyond n).
inline bool delta_merge_page(const DeltaKnownMap& m, const std::vector<uint32_t>& reviews, uint32_t mw, uint32_t n, uint32_t w0, uint32_t w1, std::vector<uint64_t>* viol,
                             std::vector<uint64_t>* err, std::vector<uint64_t>* was_viol, std::vector<uint64_t>* was_err) {
  const size_t words = reviews.size() * (size_t)mw;
  if (viol->size() != words || err->size() != words || was_viol->size() != words || was_err->size() != words) return false;
  for (size_t i = 0; i < reviews.size(); i++) {
    if (reviews[i] / 64u < w0 || reviews[i] / 64u >= w1 || reviews[i] >= n || (i && reviews[i] <= reviews[i - 1])) return false;
    if (m.empty()) continue;
    const auto it = m.find(reviews[i]);
    if (it == m.end()) continue;
    const DeltaKnown& k = it->second;
    if (k.nv.size() != mw) return false;
    for (uint32_t j = 0; j < mw; j++) { (*viol)[i * mw + j] = k.nv[j]; (*err)[i * mw + j] = k.ne[j]; (*was_viol)[i * mw + j] = k.wv[j]; (*was_err)[i * mw + j] = k.we[j]; }
  }
  return true;
}

}  // namespace gk
