// TEST ONLY: the review-words analysis and the list filter (csrc/review_words.hpp, csrc/chunks.hpp) on hand-built predicate classes and a
// hand-built slot index.  Stand-alone: tests/test_review_words_native.py builds it plain and with -fsanitize=address,undefined and runs both.
#include "review_words.hpp"

#include <cstdio>
#include <cstdlib>

using namespace gk;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static Pred pred(uint32_t op, uint32_t dst, uint32_t bit) {
  Pred p{};
  p.op = (uint8_t)op; p.dst = (uint8_t)dst; p.bit = (uint16_t)bit;
  return p;
}

int main() {
  // classes (1-based, entry 0 empty): 1 = two global bits in words 0 and 2 | 2 = an element bit | 3 = global + element | 4 = an element marker
  // 5 = a stored value | 6 = one global bit in word 1 | 7 = a global bit beyond the plan's words
  std::vector<std::vector<Pred>> classes(8);
  classes[1] = {pred(P_CMP, D_GLOBAL, 5), pred(P_TYPE, D_GLOBAL, 64 + 3)};
  classes[2] = {pred(P_CMP, D_ELEM, 1)};
  classes[3] = {pred(P_DEFINED, D_GLOBAL, 7), pred(P_CMP, D_ELEM, 2)};
  classes[4] = {pred(P_PRESENT, D_ELEM, 0)};
  classes[5] = {pred(P_STORE, D_ELEM, 0)};
  classes[6] = {pred(P_BITS, D_GLOBAL, 32 + 9)};
  classes[7] = {pred(P_CMP, D_GLOBAL, 3 * 32 + 1)};
  const ReviewWords rw = analyse_review_words(classes, 3);
  CHECK(rw.hoisted.size() == 8);
  CHECK(rw.is_hoisted(1) && rw.is_hoisted(6));
  CHECK(!rw.is_hoisted(0) && !rw.is_hoisted(2) && !rw.is_hoisted(3) && !rw.is_hoisted(4) && !rw.is_hoisted(5) && !rw.is_hoisted(7) && !rw.is_hoisted(99));
  CHECK(rw.k() == 3 && rw.words[0] == 0 && rw.words[1] == 1 && rw.words[2] == 2);
  CHECK(rw.slot_of(2) == 2 && rw.slot_of(7) == -1);
  // a P_STORE / P_PRESENT with a global destination disqualifies as well, and so does an empty plan
  std::vector<std::vector<Pred>> odd(3);
  odd[1] = {pred(P_STORE, D_GLOBAL, 1)};
  odd[2] = {pred(P_PRESENT, D_GLOBAL, 1)};
  CHECK(analyse_review_words(odd, 4).k() == 0);
  CHECK(analyse_review_words({}, 4).k() == 0 && analyse_review_words(classes, 0).k() == 0);
  // words beyond GK_RW_MAX_WORD stay with the sweep
  std::vector<std::vector<Pred>> far(2);
  far[1] = {pred(P_CMP, D_GLOBAL, GK_RW_MAX_WORD * 32)};
  CHECK(analyse_review_words(far, GK_RW_MAX_WORD + 4).k() == 0);

  // three groups x four slots.  slot 0 -> class 1 (hoisted), slot 1 -> class 2, slot 2 -> class 6 (hoisted, reads strings), slot 3 -> class 4
  // rows per (group, slot): group 0 {70, 10, 64, 3}, group 1 {5, 0, 130, 0} (only hoisted paths), group 2 {0, 0, 0, 0}
  const uint32_t S = 4, G = 3;
  const uint32_t n[G][S] = {{70, 10, 64, 3}, {5, 0, 130, 0}, {0, 0, 0, 0}};
  std::vector<uint32_t> ix(G * (S + 1));
  uint32_t row = 0;
  for (uint32_t g = 0; g < G; g++) {
    for (uint32_t s = 0; s < S; s++) { ix[g * (S + 1) + s] = row; row += n[g][s]; }
    ix[g * (S + 1) + S] = row;
  }
  const std::vector<BoundPath> bound = {{0, 1, 3}, {1, 2, 3}, {2, 6u | GK_ENT_NEEDS_STR, 5}, {3, 4, 2}};
  std::vector<BoundPath> kept, hoisted;
  split_bound(bound, rw, &kept, &hoisted);
  CHECK(kept.size() == 2 && kept[0].slot == 1 && kept[1].slot == 3);
  CHECK(hoisted.size() == 2 && hoisted[0].slot == 0 && hoisted[1].slot == 2);
  const ChunkLists full = build_chunk_lists(ix.data(), G, S, bound, 64, 4);
  const ChunkLists part = build_chunk_lists(ix.data(), G, S, kept, 64, 4);
  CHECK(full.n_chunks == 2 + 1 + 1 + 1 + 1 + 3 && part.n_chunks == 2);
  CHECK(part.n_chunks < full.n_chunks && part.capg <= full.capg);
  CHECK(full.n_overflow_groups == 0 && part.n_overflow_groups == 0);
  // group 1 holds rows of hoisted paths only: a valid list of zero chunks, no overflow flag; group 2 is empty either way
  CHECK(part.d[1 * part.capg].st == 0 && part.d[1 * part.capg].info == 0);
  CHECK(full.d[1 * full.capg].st == 4 && part.d[2 * part.capg].st == 0 && part.d[2 * part.capg].info == 0);
  CHECK(part.d[0].st == 2 && !(part.d[0].info & GK_LIST_OVERFLOW));
  for (uint32_t i = 1; i <= 2; i++) { const uint32_t ent = part.d[i].info >> GK_DESC_ENT_SHIFT; CHECK((ent & GK_DESC_ENT_MASK) == 2 || (ent & GK_DESC_ENT_MASK) == 4); }
  // a list capacity the kept paths fit and the full set does not: the overflow test looks at the kept paths only
  const ChunkLists tight_full = build_chunk_lists(ix.data(), G, S, bound, 4, 4), tight_part = build_chunk_lists(ix.data(), G, S, kept, 4, 4);
  CHECK(tight_full.n_overflow_groups == 2 && tight_part.n_overflow_groups == 0);
  // every path hoisted: every group's list is empty and none overflows
  std::vector<BoundPath> only = {{0, 1, 3}, {2, 6u | GK_ENT_NEEDS_STR, 5}}, k2, h2;
  split_bound(only, rw, &k2, &h2);
  CHECK(k2.empty() && h2.size() == 2);
  const ChunkLists none = build_chunk_lists(ix.data(), G, S, k2, 64, 4);
  CHECK(none.n_chunks == 0 && none.n_overflow_groups == 0 && none.capg == 1 && none.d.size() == G);
  for (uint32_t g = 0; g < G; g++) CHECK(none.d[g].st == 0 && none.d[g].info == 0);
  // the size threshold and the geometry
  CHECK(!review_words_wanted(ReviewWords{}, 256, 1u << 20));
  CHECK(!review_words_wanted(rw, 64, 1u << 20));
  puts("review words ok");
  return 0;
}
