// Stand-alone program (its own main; never loaded into Python; built plain and with -fsanitize=address,undefined by
// tests/test_table_stream_native.py) for the host side of a table's violation stream (gk_table_violations):
//   * csrc/table_stream.hpp: cursor packing and checking, the index with host-only entries in the prefix and where its pages end
//     (viol_page_end / viol_next_word of viol_stream.hpp), the merge of host pairs into a page;
//   * the CPU stand-in of dev_tviol_index / dev_tviol_entries (hostemu_tviol.cpp, compiled into this program) -- through its public
//     entries, fed by dev_tviol_note -- against a bit-by-bit reference over seeded random bitmaps, one plan and several groups.
// hostemu_tviol.cpp needs nothing of device.hpp but its own entries; a table is only an address to it.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "device.hpp"
#include "table_stream.hpp"

namespace gk {
struct DevTable { int unused = 0; };
}  // namespace gk

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static void cursor_cases() {
  for (uint32_t gen : {1u, 77u, (1u << 28) - 1u})
    for (uint32_t word : {0u, 2u, 64u, 15624u, 0xFFFFFFFEu}) {
      const uint64_t packed = gk::table_cursor_pack(gen, word);
      uint32_t back = ~0u;
      CHECK(packed != 0 && gk::table_cursor_check(packed, gen, word + 1u, &back) && back == word);
      CHECK(!gk::table_cursor_check(packed, gen, word, &back));                      // the table has no such word
      CHECK(!gk::table_cursor_check(packed, gk::viol_next_gen(gen), word + 1u, &back));   // another stream generation
      CHECK(!gk::table_cursor_check(packed, 0, word + 1u, &back));                    // no stream yet
    }
  uint32_t back = 0;
  CHECK(gk::table_cursor_pack(0, 5) == 0 && gk::table_cursor_pack(1u << 28, 5) == 0);   // generations nobody hands out
  CHECK(!gk::table_cursor_check(0, 1, 10, &back));                                    // 0 is "start", never a position
  CHECK(!gk::table_cursor_check(5, 1, 10, &back) && !gk::table_cursor_check(5, 0, 10, &back));   // generation 0
  CHECK(!gk::table_cursor_check(0xDEADBEEFDEADBEEFull, 1, 10, &back) && !gk::table_cursor_check(~0ull, 1, 10, &back));
  CHECK(!gk::table_cursor_check(gk::table_cursor_pack(1, 0), 1, 0, &back));           // a table without words
}

static void page_cases() {
  using gk::TablePairs;
  // 5 words, 300 reviews; the device names cnt[w] reviews, the host answered reviews 70 (word 1: no device entry there), 130 and 131
  // (word 2, next to two device entries) and 299 (the last review)
  const std::vector<uint32_t> cnt{3, 0, 2, 0, 0};
  const std::vector<uint64_t> any{0b111ull, 0, (1ull << 5) | (1ull << 9), 0, 0};
  const TablePairs hv{{0, 70}, {3, 130}, {64, 130}, {1, 299}, {2, 300}, {200, 71}};   // (review 300 and row 200 do not exist: dropped)
  const TablePairs he{{5, 131}, {3, 130}};
  const std::vector<uint64_t> host = gk::table_host_words(hv, he, 130, 300);
  CHECK(host.size() == 5 && host[0] == 0 && host[1] == 1ull << 6 && host[2] == ((1ull << 2) | (1ull << 3)) && host[3] == 0 && host[4] == 1ull << 43);
  std::vector<uint64_t> prefix;
  CHECK(gk::table_prefix(cnt, any, host, &prefix) && (prefix == std::vector<uint64_t>{0, 3, 4, 8, 8, 9}));
  CHECK(gk::table_prefix(cnt, {}, {}, &prefix) && (prefix == std::vector<uint64_t>{0, 3, 3, 5, 5, 5}));   // the device alone: no any words needed
  CHECK(!gk::table_prefix(cnt, {}, host, &prefix) && !gk::table_prefix(cnt, any, std::vector<uint64_t>(4, 0), &prefix));
  // a review named by both sources counts once
  CHECK(gk::table_prefix({1}, {1ull << 7}, {1ull << 7}, &prefix) && prefix.back() == 1);
  CHECK(gk::table_prefix(cnt, any, host, &prefix));
  // pages: a word with host-only entries is a word with entries; the trailing host entry keeps the stream open to the last word
  CHECK(gk::viol_next_word(prefix, 1) == 1u && gk::viol_next_word(prefix, 3) == 4u && gk::viol_next_word(prefix, 5) == 5u);
  CHECK(gk::viol_page_end(prefix, 0, 64) == 5u);
  std::vector<uint64_t> wide;
  CHECK(gk::table_prefix({64, 0, 60, 0}, {~0ull, 0, ~0ull >> 4, 0}, {0, 1, 0xFull << 60, 1ull << 63}, &wide) && (wide == std::vector<uint64_t>{0, 64, 65, 129, 130}));
  CHECK(gk::viol_page_end(wide, 0, 64) == 1u && gk::viol_page_end(wide, 0, 65) == 2u && gk::viol_page_end(wide, 1, 64) == 2u && gk::viol_page_end(wide, 1, 65) == 3u);
  CHECK(gk::viol_page_end(wide, 2, 1) == 3u && gk::viol_page_end(wide, 3, 64) == 4u);
}

static void merge_cases() {
  using gk::TablePairs;
  using V = std::vector<uint32_t>;
  using M = std::vector<uint64_t>;
  const uint32_t mw = 3, rows = 130, n = 300;
  const V dev{64, 69, 133};
  const M dv{1, 0, 0, 0, 1ull << 63, 0, 0, 0, 2}, de{0, 0, 0, 2, 0, 0, 4, 0, 0};
  const TablePairs hv{{0, 70}, {129, 70}, {64, 130}, {3, 10}, {2, 200}, {130, 72}, {1, 300}};
  const TablePairs he{{63, 131}, {5, 70}};
  V rev;
  M v, e;
  // words [1, 3): reviews 64 .. 191.  Host reviews 70, 130 and 131 join; review 10 (word 0) and 200 (word 3) are not on the page
  CHECK(gk::table_merge_page(dev, dv, de, mw, hv, he, rows, n, 1, 3, &rev, &v, &e));
  CHECK((rev == V{64, 69, 70, 130, 131, 133}));
  CHECK((v == M{1, 0, 0, 0, 1ull << 63, 0, 1, 0, 2, 0, 1, 0, 0, 0, 0, 0, 0, 2}));
  CHECK((e == M{0, 0, 0, 2, 0, 0, 1ull << 5, 0, 0, 0, 0, 0, 1ull << 63, 0, 0, 4, 0, 0}));
  // without host pairs on the page: the device's lists as they are
  CHECK(gk::table_merge_page(dev, dv, de, mw, {{3, 10}}, {}, rows, n, 1, 3, &rev, &v, &e) && rev == dev && v == dv && e == de);
  // a host pair for a review the device names too: one entry, both bits
  CHECK(gk::table_merge_page(dev, dv, de, mw, {{7, 69}}, {{8, 69}}, rows, n, 1, 3, &rev, &v, &e) && rev == dev);
  CHECK(v[3] == 1ull << 7 && v[4] == 1ull << 63 && e[3] == (2 | 1ull << 8));
  // host entries alone
  CHECK(gk::table_merge_page({}, {}, {}, mw, hv, he, rows, n, 0, 1, &rev, &v, &e) && (rev == V{10}) && (v == M{8, 0, 0}) && (e == M{0, 0, 0}));
  CHECK(gk::table_merge_page({}, {}, {}, mw, {}, {}, rows, n, 0, 5, &rev, &v, &e) && rev.empty() && v.empty() && e.empty());
  // lists that do not belong together
  CHECK(!gk::table_merge_page(dev, dv, de, 2, hv, he, rows, n, 1, 3, &rev, &v, &e));                       // masks of another width
  CHECK(!gk::table_merge_page(dev, dv, M(8, 0), mw, hv, he, rows, n, 1, 3, &rev, &v, &e));
  CHECK(!gk::table_merge_page(dev, dv, de, mw, hv, he, rows, n, 2, 3, &rev, &v, &e));                      // review 64 lies before the page
  CHECK(!gk::table_merge_page(dev, dv, de, mw, hv, he, rows, n, 1, 2, &rev, &v, &e));                      // review 133 behind it
  CHECK(!gk::table_merge_page({69, 64, 133}, dv, de, mw, hv, he, rows, n, 1, 3, &rev, &v, &e));            // not ascending
  CHECK(!gk::table_merge_page({64, 64, 133}, dv, de, mw, hv, he, rows, n, 1, 3, &rev, &v, &e));
  CHECK(!gk::table_merge_page({64, 69, 133}, dv, de, mw, hv, he, rows, 133, 1, 3, &rev, &v, &e));          // beyond the table's reviews
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64, seeded: the same bitmaps in every run
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the constraints cut into plan groups of at most group_max rows (0: one plan); more than eight groups at 130 / 12
static void stand_in_shape(uint32_t nc, uint32_t n, uint32_t group_max, int density) {
  const uint32_t nt = (n + 63u) / 64u + (n % 3u == 0 ? 1u : 0u);   // (a table may have more words per row than its reviews need)
  const uint32_t pw = (n + 63u) / 64u, mw = (nc + 63u) / 64u;
  std::vector<gk::DevTable> tables((group_max ? (nc + group_max - 1) / group_max : 1) + 1);
  std::vector<gk::TviolSide> sides;
  std::vector<gk::EvalOut> outs;
  for (uint32_t row0 = 0, g = 0; row0 < nc; g++) {
    const uint32_t rows = group_max ? std::min(group_max, nc - row0) : nc;
    gk::EvalOut o;
    o.n_reviews = n; o.n_constraints = rows; o.n_tiles = nt;
    o.viol.resize((size_t)rows * nt); o.err.resize((size_t)rows * nt); o.too_big.resize(nt);
    // sparse, half, dense; bits beyond n are set as well (they must not count)
    for (auto& w : o.viol) w = density == 0 ? (rnd() & rnd() & rnd() & rnd() & rnd() & rnd()) : density == 1 ? (rnd() & rnd()) : (rnd() | rnd());
    for (auto& w : o.err) w = density == 0 ? (rnd() & rnd() & rnd() & rnd() & rnd() & rnd() & rnd()) : density == 1 ? (rnd() & rnd() & rnd()) : rnd();
    for (auto& w : o.too_big) w = rnd() & rnd() & rnd() & rnd();
    if (density == 0 && nt > 1) for (uint32_t r = 0; r < rows; r++) { o.viol[(size_t)r * nt + 1] = 0; o.err[(size_t)r * nt + 1] = 0; }   // a word without entries
    sides.push_back(gk::TviolSide{&tables[g], rows, row0});
    gk::dev_tviol_note(&tables[g], o);
    outs.push_back(std::move(o));
    row0 += rows;
  }
  sides.push_back(gk::TviolSide{&tables.back(), 0, nc});   // a group without rows is skipped, evaluated or not
  // bit by bit
  std::vector<uint32_t> want_rev, want_cnt(pw, 0);
  std::vector<uint64_t> want_viol, want_err, want_any(pw, 0);
  uint64_t want_beyond = 0;
  for (uint32_t s = 0; s < n; s++) {
    bool big = false, any = false;
    std::vector<uint64_t> mv(mw, 0), me(mw, 0);
    for (size_t g = 0; g < outs.size(); g++) {
      const gk::EvalOut& o = outs[g];
      big = big || ((o.too_big[s / 64] >> (s % 64)) & 1ull);
      for (uint32_t r = 0; r < o.n_constraints; r++) {
        const uint32_t row = sides[g].row0 + r;
        if ((o.viol[(size_t)r * nt + s / 64] >> (s % 64)) & 1ull) { mv[row / 64] |= 1ull << (row % 64); any = true; }
        if ((o.err[(size_t)r * nt + s / 64] >> (s % 64)) & 1ull) { me[row / 64] |= 1ull << (row % 64); any = true; }
      }
    }
    if (big) { want_beyond++; continue; }
    if (!any) continue;
    want_rev.push_back(s);
    want_viol.insert(want_viol.end(), mv.begin(), mv.end());
    want_err.insert(want_err.end(), me.begin(), me.end());
    want_cnt[s / 64]++;
    want_any[s / 64] |= 1ull << (s % 64);
  }
  std::vector<uint32_t> cnt, rev;
  std::vector<uint64_t> any, v, e;
  uint64_t beyond = 0;
  float ms = -1;
  gk::dev_tviol_index(sides, n, &cnt, &any, &beyond, &ms);
  CHECK(cnt == want_cnt && any == want_any && beyond == want_beyond && ms == 0);
  gk::dev_tviol_index(sides, n, &cnt, nullptr, &beyond, &ms);
  CHECK(cnt == want_cnt && beyond == want_beyond);
  std::vector<uint32_t> off(pw + 1, 0);
  for (uint32_t w = 0; w < pw; w++) off[w + 1] = off[w] + cnt[w];
  gk::dev_tviol_entries(sides, n, off, 0, pw, &rev, &v, &e, &ms);
  CHECK(rev == want_rev && v == want_viol && e == want_err);
  // word ranges: the pieces are the whole, in order
  std::vector<uint32_t> cat_rev;
  std::vector<uint64_t> cat_v, cat_e;
  for (uint32_t w0 = 0; w0 < pw; w0 += 3) {
    gk::dev_tviol_entries(sides, n, off, w0, std::min(pw, w0 + 3), &rev, &v, &e, &ms);
    cat_rev.insert(cat_rev.end(), rev.begin(), rev.end());
    cat_v.insert(cat_v.end(), v.begin(), v.end());
    cat_e.insert(cat_e.end(), e.begin(), e.end());
  }
  CHECK(cat_rev == want_rev && cat_v == want_viol && cat_e == want_err);
  gk::dev_tviol_entries(sides, n, off, pw, pw, &rev, &v, &e, &ms);
  CHECK(rev.empty() && v.empty() && e.empty());
  // an index of other bitmaps is noticed, not followed
  auto throws = [](auto&& f) { try { f(); } catch (const std::runtime_error&) { return true; } return false; };
  if (!want_rev.empty()) {
    std::vector<uint32_t> wrong = off;
    for (uint32_t w = want_rev[0] / 64 + 1; w <= pw; w++) wrong[w]++;
    CHECK(throws([&] { gk::dev_tviol_entries(sides, n, wrong, 0, pw, &rev, &v, &e, &ms); }));
  }
  CHECK(throws([&] { gk::dev_tviol_entries(sides, n, std::vector<uint32_t>(pw, 0), 0, pw, &rev, &v, &e, &ms); }));   // an index of another size
  CHECK(throws([&] { gk::dev_tviol_entries(sides, n, off, 0, pw + 1, &rev, &v, &e, &ms); }));                         // a range beyond the words
  CHECK(throws([&] { gk::dev_tviol_entries(sides, n, off, pw, pw == 0 ? 1 : pw - 1, &rev, &v, &e, &ms); }));
  CHECK(throws([&] { gk::dev_tviol_index(sides, n + 1, &cnt, nullptr, &beyond, &ms); }));                             // another review count
  std::vector<gk::TviolSide> other = sides;
  other[0].nc++;
  CHECK(throws([&] { gk::dev_tviol_index(other, n, &cnt, nullptr, &beyond, &ms); }));                                 // evaluated for other rows
  for (auto& t : tables) gk::dev_tviol_forget(&t);
  CHECK(throws([&] { gk::dev_tviol_index(sides, n, &cnt, nullptr, &beyond, &ms); }));                                 // nothing kept any more
}

static void stand_in_cases() {
  for (uint32_t nc : {1u, 63u, 64u, 65u, 130u})
    for (uint32_t n : {1u, 63u, 64u, 65u, 200u, 4133u})
      for (int density = 0; density < 3; density++) stand_in_shape(nc, n, 0, density);
  // plan groups: row0 = 0, 50, 100 (the middle group straddles bit 64 of the mask); 0, 20, 40; eleven groups of 12
  for (uint32_t n : {1u, 65u, 200u, 4133u})
    for (int density = 0; density < 3; density++) {
      stand_in_shape(130, n, 50, density);
      stand_in_shape(50, n, 20, density);
      stand_in_shape(130, n, 12, density);
    }
  // a table without constraints: no entries, nothing beyond
  gk::DevTable t;
  std::vector<uint32_t> cnt;
  uint64_t beyond = 7;
  float ms = 0;
  gk::dev_tviol_index({gk::TviolSide{&t, 0, 0}}, 130, &cnt, nullptr, &beyond, &ms);
  CHECK(cnt == std::vector<uint32_t>(3, 0) && beyond == 0);
}

int main() {
  struct { const char* name; void (*fn)(); } cases[] = {{"cursor", cursor_cases}, {"pages", page_cases}, {"merge", merge_cases}, {"stand_in", stand_in_cases}};
  for (auto& c : cases) {
    const int before = failures;
    c.fn();
    printf("%s %s\n", failures > before ? "FAIL" : "ok", c.name);
  }
  return failures ? 1 : 0;
}
