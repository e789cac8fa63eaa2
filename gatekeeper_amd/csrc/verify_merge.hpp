// What a verification of the plan-specialised kernel against the bytecode kernel hands out per plan group (dev_verify_diff, device.hpp)
// and the host merge of those answers over the plan groups of a table and the chunks of the resident set (gk_table_verify,
// gk_resident_verify): a later group's rows are appended below the earlier ones' -- counts land at, entry rows are shifted by, the group's
// row base --, a later chunk's reviews are shifted by the slots of the chunks before it and its counts are added to the same rows; the
// entries are then sorted by (kind, row, review) and the smallest max_entries of what the device stored are kept.  Host only; no
// dependency on the engine (tests/native/verify_merge_test.cpp runs it under sanitizers).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gk {

enum : uint32_t { VERIFY_VIOL = 0, VERIFY_ERR = 1, VERIFY_MATCH = 2, VERIFY_TOO_BIG = 3 };   // (= GK_VERIFY_* of gkgpu.h)
struct VerifyEntry { uint32_t kind, row, review, a_bit; };   // a_bit: the bit on the specialised side
struct VerifyDiff {
  std::vector<uint64_t> diff[3];    // [kind][nc] differing reviews per bitmap row (VERIFY_MATCH only with want_match)
  uint64_t diff_too_big = 0;
  uint64_t entries_total = 0;       // differences in all: what the device wanted to store
  std::vector<VerifyEntry> entries; // min(entries_total, cap) of them, in no particular order
  float ms = 0;                     // device time of the comparison
};

inline bool verify_entry_less(const VerifyEntry& a, const VerifyEntry& b) {
  if (a.kind != b.kind) return a.kind < b.kind;
  if (a.row != b.row) return a.row < b.row;
  return a.review < b.review;
}

struct VerifyMerge {
  std::vector<uint64_t> diff[3];    // [kind][n_rows]
  uint64_t diff_too_big = 0, entries_total = 0;
  std::vector<VerifyEntry> entries;
  float ms = 0;
  void begin(uint32_t n_rows, bool want_match) {
    for (int k = 0; k < 3; k++) diff[k].assign(k < 2 || want_match ? n_rows : 0, 0);
    diff_too_big = entries_total = 0; entries.clear(); ms = 0;
  }
  // one plan group of one table: rows [row_base, row_base + its rows), reviews from review_base on.  Rows beyond n_rows are dropped
  // (the caller sized the merge for the rows it reports).
  void add(const VerifyDiff& d, uint32_t row_base, uint32_t review_base) {
    for (int k = 0; k < 3; k++)
      for (size_t r = 0; r < d.diff[k].size() && row_base + r < diff[k].size(); r++) diff[k][row_base + r] += d.diff[k][r];
    diff_too_big += d.diff_too_big;
    entries_total += d.entries_total;
    ms += d.ms;
    for (VerifyEntry en : d.entries) {
      if (en.kind != VERIFY_TOO_BIG) en.row += row_base;
      en.review += review_base;
      entries.push_back(en);
    }
  }
  // ascending by (kind, row, review); the smallest max_entries of what the device stored
  void finish(uint32_t max_entries) {
    std::sort(entries.begin(), entries.end(), verify_entry_less);
    if (entries.size() > max_entries) entries.resize(max_entries);
  }
  uint64_t diff_total() const {
    uint64_t n = diff_too_big;
    for (int k = 0; k < 3; k++) for (uint64_t v : diff[k]) n += v;
    return n;
  }
};

}  // namespace gk
