// The pure part of the resident-set changes stream (gk_resident_changes) that viol_stream.hpp does not already hold: the pairs only the
// host knows -- autoreject pairs, violating pairs the host evaluator completed -- are no part of the device bitmaps, so they are kept
// with the baseline as sparse lists and compared here.  Host only; no HIP and no dependency on the engine
// (tests/native/delta_stream_test.cpp runs it under sanitizers).
//
// A list holds (slot, row) pairs of ONE chunk under the shown mask of its state, ascending and without repeats.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <utility>
#include <vector>

namespace gk {

using DeltaPair = std::pair<uint32_t, uint32_t>;   // (slot, bitmap row)

// ascending and without repeats, whatever order the pairs came in
inline void delta_pairs_sort(std::vector<DeltaPair>* v) {
  std::sort(v->begin(), v->end());
  v->erase(std::unique(v->begin(), v->end()), v->end());
}

// the slots whose rows differ between the two lists, ascending and without repeats
inline std::vector<uint32_t> delta_pairs_changed(const std::vector<DeltaPair>& now, const std::vector<DeltaPair>& base) {
  std::vector<DeltaPair> diff;
  std::set_symmetric_difference(now.begin(), now.end(), base.begin(), base.end(), std::back_inserter(diff));
  std::vector<uint32_t> slots;
  for (const DeltaPair& p : diff)
    if (slots.empty() || slots.back() != p.first) slots.push_back(p.first);
  return slots;
}

// dst[i][row] |= 1 for every pair whose slot is slots[i] (the page: ascending; dst is [slots][mw]); rows at or beyond `rows` are dropped
inline void delta_pairs_or(const std::vector<DeltaPair>& pairs, const std::vector<uint32_t>& slots, uint32_t mw, uint32_t rows, std::vector<uint64_t>* dst) {
  if (slots.empty() || dst->size() != slots.size() * (size_t)mw) return;
  auto it = std::lower_bound(pairs.begin(), pairs.end(), DeltaPair(slots.front(), 0u));
  size_t at = 0;
  for (; it != pairs.end() && it->first <= slots.back(); ++it) {
    while (at < slots.size() && slots[at] < it->first) at++;
    if (at == slots.size()) break;
    if (slots[at] != it->first || it->second >= rows || it->second / 64u >= mw) continue;
    (*dst)[at * mw + it->second / 64u] |= 1ull << (it->second % 64u);
  }
}

}  // namespace gk
