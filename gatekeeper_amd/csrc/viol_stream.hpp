// The pure part of the resident-set violation stream (gk_resident_violations): where a page ends, what a cursor carries, how the
// device's entries of one plan group, the err-only / host-only slots and the other groups' entries become one page.  Host only; no HIP
// and no dependency on the engine (tests/native/viol_stream_test.cpp runs it under sanitizers).
//
// A chunk's entries are described by `prefix`, the exclusive prefix sum of its entries per 64-slot bitmap word ([words + 1]).  A page
// is a run of whole words [w0, w1) of ONE chunk.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <vector>

namespace gk {

// the first word at or after `w` that has entries; the number of words when there is none
inline uint32_t viol_next_word(const std::vector<uint64_t>& prefix, uint32_t w) {
  const uint32_t words = prefix.empty() ? 0u : (uint32_t)(prefix.size() - 1);
  if (w >= words) return words;
  // (prefix is non-decreasing: the first element above prefix[w] is the end of the first word with entries)
  const size_t end = (size_t)(std::upper_bound(prefix.begin() + w, prefix.end(), prefix[w]) - prefix.begin());
  return end > words ? words : (uint32_t)(end - 1);
}

// The end w1 of the page that begins at word w0 (< words): the longest run of whole words whose entries fit in max_objects.  A limit
// below 64 counts as 64, so the page always takes at least the word w0, whatever it holds.
inline uint32_t viol_page_end(const std::vector<uint64_t>& prefix, uint32_t w0, uint32_t max_objects) {
  const uint32_t words = prefix.empty() ? 0u : (uint32_t)(prefix.size() - 1);
  if (w0 >= words) return words;
  const uint64_t room = std::max<uint32_t>(max_objects, 64u);
  // the last w1 with prefix[w1] - prefix[w0] <= room
  const size_t w1 = (size_t)(std::upper_bound(prefix.begin() + w0, prefix.end(), prefix[w0] + room) - prefix.begin()) - 1;
  return (uint32_t)std::max<size_t>(w1, (size_t)w0 + 1);
}

// ---- cursor: | stream generation 28 | chunk 8 | word 28 |.  The generation is never 0, so no cursor of a stream is 0 ("start").
struct ViolCursor { uint32_t gen = 0, chunk = 0, word = 0; };
constexpr uint32_t VIOL_CUR_WORD_BITS = 28, VIOL_CUR_CHUNK_BITS = 8, VIOL_CUR_GEN_BITS = 28;
// the generation that follows `gen` (1 .. 2^28 - 1, skipping 0)
inline uint32_t viol_next_gen(uint32_t gen) {
  const uint32_t g = (gen + 1u) & ((1u << VIOL_CUR_GEN_BITS) - 1u);
  return g ? g : 1u;
}
// 0: one of the fields does not fit its bits (nothing this engine can produce: 17 chunks at most, 2^32 slots per chunk = 2^26 words)
inline uint64_t viol_cursor_pack(const ViolCursor& c) {
  if (c.gen == 0 || c.gen >> VIOL_CUR_GEN_BITS || c.chunk >> VIOL_CUR_CHUNK_BITS || c.word >> VIOL_CUR_WORD_BITS) return 0;
  return ((uint64_t)c.gen << (VIOL_CUR_CHUNK_BITS + VIOL_CUR_WORD_BITS)) | ((uint64_t)c.chunk << VIOL_CUR_WORD_BITS) | c.word;
}
// false: not a cursor of the stream generation `gen_now` over chunks of `chunk_words[i]` words each
inline bool viol_cursor_check(uint64_t cursor, uint32_t gen_now, const std::vector<uint32_t>& chunk_words, ViolCursor* out) {
  ViolCursor c;
  c.word = (uint32_t)(cursor & ((1ull << VIOL_CUR_WORD_BITS) - 1ull));
  c.chunk = (uint32_t)((cursor >> VIOL_CUR_WORD_BITS) & ((1ull << VIOL_CUR_CHUNK_BITS) - 1ull));
  c.gen = (uint32_t)(cursor >> (VIOL_CUR_CHUNK_BITS + VIOL_CUR_WORD_BITS));
  if (c.gen == 0 || c.gen != gen_now || c.chunk >= chunk_words.size() || c.word >= chunk_words[c.chunk]) return false;
  *out = c;
  return true;
}

// ---- one page.  Slot lists are ascending and without repeats.
// the union of two slot lists
inline std::vector<uint32_t> viol_merge_slots(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b) {
  std::vector<uint32_t> out;
  out.reserve(a.size() + b.size());
  std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out));
  return out;
}

// dst[0 .. mw) |= the `nrows` low bits of src, moved up by row0 bits: a plan group's rows into their place among all constraints.
// src has ceil(nrows / 64) words; bits of src at or beyond nrows, and bits that would land beyond dst, are dropped.
inline void viol_or_shifted(uint64_t* dst, uint32_t mw, const uint64_t* src, uint32_t nrows, uint32_t row0) {
  const uint32_t sw = (nrows + 63u) / 64u, word0 = row0 / 64u, sh = row0 % 64u;
  for (uint32_t i = 0; i < sw; i++) {
    uint64_t x = src[i];
    if (i == sw - 1u && nrows % 64u) x &= (1ull << (nrows % 64u)) - 1ull;
    if (!x) continue;
    if (word0 + i < mw) dst[word0 + i] |= x << sh;
    if (sh && word0 + i + 1u < mw) dst[word0 + i + 1u] |= x >> (64u - sh);
  }
}

// A group's device entries into the page: `slots` is the page (every review of `reviews` is among them), dst is [slots][mw].
// false: a review that is not on the page -- the lists do not belong together.
inline bool viol_scatter(const std::vector<uint32_t>& slots, uint32_t mw, const std::vector<uint32_t>& reviews, const std::vector<uint64_t>& masks, uint32_t nrows,
                         uint32_t row0, std::vector<uint64_t>* dst) {
  const uint32_t sw = (nrows + 63u) / 64u;
  if (masks.size() != reviews.size() * (size_t)sw || dst->size() != slots.size() * (size_t)mw) return false;
  size_t at = 0;
  for (size_t i = 0; i < reviews.size(); i++) {
    while (at < slots.size() && slots[at] < reviews[i]) at++;
    if (at == slots.size() || slots[at] != reviews[i]) return false;
    viol_or_shifted(dst->data() + at * mw, mw, masks.data() + i * sw, nrows, row0);
  }
  return true;
}

// the index of `slot` on the page; slots.size() when it is not there
inline size_t viol_find(const std::vector<uint32_t>& slots, uint32_t slot) {
  const auto it = std::lower_bound(slots.begin(), slots.end(), slot);
  return it != slots.end() && *it == slot ? (size_t)(it - slots.begin()) : slots.size();
}

}  // namespace gk
