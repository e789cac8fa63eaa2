// Stand-alone program (its own main; never loaded into Python; built plain and with -fsanitize=address,undefined by
// tests/test_viol_stream_native.py) for the host side of the resident-set violation stream:
//   * csrc/viol_stream.hpp: page bounds from a prefix array, cursor packing and checking, the merge of a page's slot lists, mask shifts;
//   * the CPU stand-in of dev_viol_index / dev_viol_entries (hostemu_viol.cpp, compiled into this program) against a bit-by-bit
//     reference over seeded random bitmaps.
// hostemu_viol.cpp needs only device.hpp's public dev_last_viol, which this program supplies over a table type of its own.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "device.hpp"
#include "viol_stream.hpp"

namespace gk {
struct DevTable { std::vector<uint64_t> viol; };
void dev_last_viol(const DevTable* t, uint32_t, std::vector<uint64_t>* viol) { *viol = t->viol; }
}  // namespace gk

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static std::vector<uint64_t> prefix_of(const std::vector<uint32_t>& cnt) {
  std::vector<uint64_t> p(cnt.size() + 1, 0);
  for (size_t i = 0; i < cnt.size(); i++) p[i + 1] = p[i] + cnt[i];
  return p;
}

static void page_cases() {
  using gk::viol_next_word;
  using gk::viol_page_end;
  for (uint32_t n : {0u, 1u, 63u, 64u, 65u}) {   // one word of n entries (65: 64 + 1 over two words)
    const std::vector<uint64_t> p = prefix_of(n <= 64 ? std::vector<uint32_t>{n} : std::vector<uint32_t>{64, n - 64});
    const uint32_t words = (uint32_t)p.size() - 1;
    CHECK(viol_next_word(p, 0) == (n ? 0u : words));
    CHECK(viol_page_end(p, 0, 64) == 1u);                       // 64 entries of room: exactly the first word, whatever it holds
    CHECK(viol_page_end(p, 0, 65) == words);                    // 65: both words of the 65-entry case
    CHECK(viol_page_end(p, 0, 1000000) == words);
    CHECK(viol_page_end(p, 0, 0) == 1u && viol_page_end(p, 0, 1) == 1u && viol_page_end(p, 0, 63) == 1u);   // below 64 counts as 64
    if (n == 65) CHECK(viol_next_word(p, 1) == 1u && viol_page_end(p, 1, 0) == 2u);
  }
  CHECK(viol_next_word({}, 0) == 0u && viol_page_end({}, 0, 64) == 0u);
  CHECK(viol_next_word({0}, 0) == 0u && viol_page_end({0}, 0, 64) == 0u);   // a chunk of no words
  {   // empty words at both ends and in the middle
    const std::vector<uint64_t> p = prefix_of({0, 0, 3, 0, 0, 64, 1, 0, 0});
    CHECK(viol_next_word(p, 0) == 2u && viol_next_word(p, 2) == 2u && viol_next_word(p, 3) == 5u && viol_next_word(p, 6) == 6u);
    CHECK(viol_next_word(p, 7) == 9u && viol_next_word(p, 8) == 9u && viol_next_word(p, 9) == 9u && viol_next_word(p, 100) == 9u);
    CHECK(viol_page_end(p, 2, 64) == 5u);     // 3 entries + the empty words behind them; 64 more do not fit
    CHECK(viol_page_end(p, 2, 67) == 6u);     // 3 + 64
    CHECK(viol_page_end(p, 2, 68) == 9u);     // everything, trailing empty words included
    CHECK(viol_page_end(p, 5, 1) == 6u);      // a full word is taken whole even when the caller asked for less
    CHECK(viol_page_end(p, 5, 64) == 6u && viol_page_end(p, 5, 65) == 9u && viol_page_end(p, 6, 64) == 9u);
    CHECK(viol_page_end(p, 0, 2) == 5u);      // from an empty word (the engine never starts there): still ends behind the first entries
    CHECK(viol_page_end(p, 9, 64) == 9u && viol_page_end(p, 12, 64) == 9u);
    // walking the stream: every entry on exactly one page, no page empty, no page above its room
    for (uint32_t room : {0u, 64u, 66u, 67u, 1000u}) {
      uint64_t seen = 0;
      uint32_t pages = 0;
      for (uint32_t w = viol_next_word(p, 0); w < 9u; pages++) {
        const uint32_t w1 = viol_page_end(p, w, room);
        CHECK(w1 > w && p[w1] - p[w] > 0 && p[w1] - p[w] <= std::max(room, 64u));
        CHECK(w1 == 9u || p[w1 + 1] - p[w] > std::max(room, 64u));   // maximal: the next word would not fit
        seen += p[w1] - p[w];
        w = viol_next_word(p, w1);
      }
      CHECK(seen == 68 && pages >= 1);
    }
  }
}

static void cursor_cases() {
  using gk::ViolCursor;
  const std::vector<uint32_t> words{3, 0, 1000};
  for (uint32_t gen : {1u, 77u, (1u << 28) - 1u})
    for (uint32_t chunk : {0u, 2u})
      for (uint32_t word : {0u, 2u, 999u}) {
        if (word >= words[chunk]) continue;
        ViolCursor c;
        c.gen = gen; c.chunk = chunk; c.word = word;
        const uint64_t packed = gk::viol_cursor_pack(c);
        ViolCursor back;
        CHECK(packed != 0 && gk::viol_cursor_check(packed, gen, words, &back) && back.gen == gen && back.chunk == chunk && back.word == word);
        CHECK(!gk::viol_cursor_check(packed, gk::viol_next_gen(gen), words, &back));   // another stream generation
      }
  ViolCursor c, back;
  c.gen = 5; c.chunk = 0; c.word = 2;
  const uint64_t ok = gk::viol_cursor_pack(c);
  CHECK(gk::viol_cursor_check(ok, 5, words, &back));
  CHECK(!gk::viol_cursor_check(ok + 1, 5, words, &back));                    // word 3 of a 3-word chunk
  CHECK(!gk::viol_cursor_check(ok + (1ull << 28), 5, words, &back));         // chunk 1 has no words
  CHECK(!gk::viol_cursor_check(ok + (3ull << 28), 5, words, &back));         // chunk 3 does not exist
  CHECK(!gk::viol_cursor_check(ok, 5, {}, &back));                           // no chunks at all
  CHECK(!gk::viol_cursor_check(ok & ((1ull << 36) - 1), 0, words, &back));   // generation 0 is never handed out, even when the engine has none yet
  CHECK(!gk::viol_cursor_check(0xDEADBEEFull, 5, words, &back) && !gk::viol_cursor_check(0xDEADBEEFull, 0, words, &back) && !gk::viol_cursor_check(~0ull, 5, words, &back));
  // fields that do not fit their bits are not packed
  c.gen = 0; CHECK(gk::viol_cursor_pack(c) == 0);
  c.gen = 1u << 28; CHECK(gk::viol_cursor_pack(c) == 0);
  c.gen = 5; c.chunk = 256; CHECK(gk::viol_cursor_pack(c) == 0);
  c.chunk = 0; c.word = 1u << 28; CHECK(gk::viol_cursor_pack(c) == 0);
  CHECK(gk::viol_next_gen(0) == 1u && gk::viol_next_gen(1) == 2u && gk::viol_next_gen((1u << 28) - 1u) == 1u);
}

static void merge_cases() {
  using V = std::vector<uint32_t>;
  const V dev{10, 20, 30};
  // err-only / host-only slots in front of, between and behind the device's entries; the same slot from two sources
  CHECK((gk::viol_merge_slots(dev, V{1, 2}) == V{1, 2, 10, 20, 30}));
  CHECK((gk::viol_merge_slots(dev, V{15, 25}) == V{10, 15, 20, 25, 30}));
  CHECK((gk::viol_merge_slots(dev, V{31, 64}) == V{10, 20, 30, 31, 64}));
  CHECK((gk::viol_merge_slots(dev, V{5, 20, 30, 99}) == V{5, 10, 20, 30, 99}));
  CHECK((gk::viol_merge_slots(dev, V{}) == dev) && (gk::viol_merge_slots(V{}, dev) == dev) && gk::viol_merge_slots(V{}, V{}).empty());
  CHECK((gk::viol_merge_slots(gk::viol_merge_slots(dev, V{20}), V{10, 11}) == V{10, 11, 20, 30}));
  const V page{5, 10, 20, 30, 99};
  CHECK(gk::viol_find(page, 5) == 0 && gk::viol_find(page, 99) == 4 && gk::viol_find(page, 20) == 2);
  CHECK(gk::viol_find(page, 0) == 5 && gk::viol_find(page, 21) == 5 && gk::viol_find(page, 100) == 5 && gk::viol_find(V{}, 3) == 0);
  // two groups of 3 and 70 rows into 73 rows: the second group's rows begin at bit 3 and run into the second word
  std::vector<uint64_t> dst(page.size() * 2, 0);
  CHECK(gk::viol_scatter(page, 2, V{10, 30}, {0b101, 0b010}, 3, 0, &dst));
  CHECK(gk::viol_scatter(page, 2, V{5, 30}, {~0ull, 0x3Full, 1ull | 1ull << 63, 0x20ull}, 70, 3, &dst));
  CHECK(dst[0] == (~0ull << 3) && dst[1] == 0x1FFull);                                   // slot 5: all 70 rows of group two
  CHECK(dst[2] == 0b101 && dst[3] == 0 && dst[4] == 0 && dst[5] == 0);                   // slot 10: group one only; slot 20: nothing
  CHECK(dst[6] == (0b010 | 1ull << 3) && dst[7] == (1ull << 2 | 0x20ull << 3));          // slot 30: both groups; row 63 of group two = bit 66
  CHECK(dst[8] == 0 && dst[9] == 0);
  CHECK(!gk::viol_scatter(page, 2, V{11}, {1}, 3, 0, &dst));                             // a review that is not on the page
  CHECK(!gk::viol_scatter(page, 2, V{10}, {1, 2}, 3, 0, &dst));                          // masks of another width
  std::vector<uint64_t> small(3, 0);
  CHECK(!gk::viol_scatter(page, 2, V{10}, {1}, 3, 0, &small));
}

static void shift_cases() {
  // every row r of a 70-row group must land at bit row0 + r, for row0 = 0, 24, 63, 64 -- and nothing else may be set
  for (uint32_t row0 : {0u, 24u, 63u, 64u})
    for (uint32_t nrows : {1u, 22u, 64u, 70u}) {
      const uint32_t mw = (row0 + nrows + 63u) / 64u + 1u;
      for (uint32_t r = 0; r < nrows; r++) {
        std::vector<uint64_t> src((nrows + 63u) / 64u, 0), dst(mw, 0);
        src[r / 64] = 1ull << (r % 64);
        if (nrows % 64) src.back() |= ~0ull << (nrows % 64);   // garbage beyond the group's rows is dropped
        gk::viol_or_shifted(dst.data(), mw, src.data(), nrows, row0);
        for (uint32_t b = 0; b < mw * 64u; b++) CHECK((((dst[b / 64] >> (b % 64)) & 1ull) != 0) == (b == row0 + r));
      }
      std::vector<uint64_t> all((nrows + 63u) / 64u, ~0ull), dst(mw, 0), narrow(1, 0);
      gk::viol_or_shifted(dst.data(), mw, all.data(), nrows, row0);
      for (uint32_t b = 0; b < mw * 64u; b++) CHECK((((dst[b / 64] >> (b % 64)) & 1ull) != 0) == (b >= row0 && b < row0 + nrows));
      gk::viol_or_shifted(narrow.data(), 1, all.data(), nrows, row0);   // a destination that is too short is not overrun
      for (uint32_t b = 0; b < 64u; b++) CHECK((((narrow[0] >> b) & 1ull) != 0) == (b >= row0 && b < row0 + nrows));
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64, seeded: the same bitmaps in every run
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static void stand_in_cases() {
  for (uint32_t nc : {1u, 50u, 64u, 65u, 130u})
    for (uint32_t n : {1u, 64u, 65u, 700u})
      for (int density = 0; density < 3; density++) {   // sparse, half, dense rows; bits beyond n are set as well (they must not count)
        const uint32_t nt = (n + 63u) / 64u, mw = (nc + 63u) / 64u;
        gk::DevTable t;
        t.viol.assign((size_t)nc * nt, 0);
        for (auto& w : t.viol) w = density == 0 ? (rnd() & rnd() & rnd() & rnd() & rnd()) : density == 1 ? rnd() : (rnd() | rnd() | rnd());
        std::vector<uint64_t> shown(nt);
        for (auto& w : shown) w = rnd() | rnd();
        // bit by bit
        std::vector<uint32_t> want_rev, want_cnt(nt, 0);
        std::vector<uint64_t> want_mask, want_any(nt, 0);
        for (uint32_t s = 0; s < n; s++) {
          if (!((shown[s / 64] >> (s % 64)) & 1ull)) continue;
          std::vector<uint64_t> m(mw, 0);
          bool any = false;
          for (uint32_t r = 0; r < nc; r++)
            if ((t.viol[(size_t)r * nt + s / 64] >> (s % 64)) & 1ull) { m[r / 64] |= 1ull << (r % 64); any = true; }
          if (!any) continue;
          want_rev.push_back(s);
          want_mask.insert(want_mask.end(), m.begin(), m.end());
          want_cnt[s / 64]++;
          want_any[s / 64] |= 1ull << (s % 64);
        }
        std::vector<uint32_t> cnt, rev;
        std::vector<uint64_t> any, mask;
        gk::dev_viol_index(&t, nc, n, shown, 1, &cnt, &any);
        CHECK(cnt == want_cnt && any == want_any);
        gk::dev_viol_index(&t, nc, n, shown, 1, &cnt);
        CHECK(cnt == want_cnt);
        gk::dev_viol_entries(&t, nc, n, shown, 1, 0, nt, &rev, &mask);
        CHECK(rev == want_rev && mask == want_mask);
        // word ranges: the pieces are the whole, in order
        std::vector<uint32_t> cat_rev;
        std::vector<uint64_t> cat_mask;
        for (uint32_t w0 = 0; w0 < nt; w0 += 3) {
          gk::dev_viol_entries(&t, nc, n, shown, 1, w0, std::min(nt, w0 + 3), &rev, &mask);
          cat_rev.insert(cat_rev.end(), rev.begin(), rev.end());
          cat_mask.insert(cat_mask.end(), mask.begin(), mask.end());
        }
        CHECK(cat_rev == want_rev && cat_mask == want_mask);
        gk::dev_viol_entries(&t, nc, n, shown, 1, nt, nt, &rev, &mask);
        CHECK(rev.empty() && mask.empty());
        // a hidden set: nothing
        gk::dev_viol_entries(&t, nc, n, std::vector<uint64_t>(nt, 0), 2, 0, nt, &rev, &mask);
        CHECK(rev.empty() && mask.empty());
      }
  // what the entries refuse
  gk::DevTable t;
  t.viol.assign(2 * 3, 0);
  std::vector<uint32_t> cnt, rev;
  std::vector<uint64_t> mask;
  auto throws = [](auto&& f) { try { f(); } catch (const std::runtime_error&) { return true; } return false; };
  CHECK(throws([&] { gk::dev_viol_index(&t, 2, 130, std::vector<uint64_t>(2, ~0ull), 1, &cnt); }));             // shown too short
  CHECK(throws([&] { gk::dev_viol_index(&t, 2, 300, std::vector<uint64_t>(5, ~0ull), 1, &cnt); }));             // more reviews than the table has words for
  CHECK(throws([&] { gk::dev_viol_entries(&t, 2, 130, std::vector<uint64_t>(3, ~0ull), 1, 2, 4, &rev, &mask); }));   // a range beyond the words
  CHECK(throws([&] { gk::dev_viol_entries(&t, 2, 130, std::vector<uint64_t>(3, ~0ull), 1, 2, 1, &rev, &mask); }));
  gk::DevTable none;
  CHECK(throws([&] { gk::dev_viol_index(&none, 2, 130, std::vector<uint64_t>(3, ~0ull), 1, &cnt); }));          // never evaluated
}

int main() {
  struct { const char* name; void (*fn)(); } cases[] = {{"pages", page_cases}, {"cursor", cursor_cases}, {"merge", merge_cases}, {"shift", shift_cases},
                                                        {"stand_in", stand_in_cases}};
  for (auto& c : cases) {
    const int before = failures;
    c.fn();
    printf("%s %s\n", failures > before ? "FAIL" : "ok", c.name);
  }
  return failures ? 1 : 0;
}
