// Stand-alone test of the pure part of gk_table_changes (csrc/table_delta.hpp) and of the CPU stand-in's loops
// (tests/native/hostemu_tchg.cpp) against a bit-by-bit reference.  Own main; built plain and under sanitizers by
// tests/test_table_delta_native.py; never loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "table_delta.hpp"

using namespace gk;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

namespace gk {
struct TchgFlat { const uint64_t *viol, *err, *big; uint32_t rows, pw, n; };
struct TchgGroup { const uint64_t *viol, *err, *big; uint32_t nc, nt, row0; };
void tchg_flatten_words(const std::vector<TchgGroup>& gs, uint32_t rows, uint32_t pw, std::vector<uint64_t>* out_viol, std::vector<uint64_t>* out_err,
                        std::vector<uint64_t>* out_big);
void tchg_align_words(const TchgFlat& s, uint32_t n, const uint32_t* then_of, const std::vector<uint32_t>& row_of, std::vector<uint64_t>* was_viol,
                      std::vector<uint64_t>* was_err, std::vector<uint64_t>* was_big);
void tchg_index_words(const TchgFlat& now, const TchgFlat& was, const uint64_t* moved, const uint64_t* only, std::vector<uint32_t>* cnt,
                      std::vector<uint64_t>* changed, std::vector<uint64_t>* big, uint64_t* beyond);
void tchg_entries_words(const TchgFlat& now, const TchgFlat& was, const uint64_t* moved, const uint64_t* only, uint32_t w0, uint32_t w1, const uint64_t* drop,
                        const uint64_t* extra, std::vector<uint32_t>* reviews, std::vector<uint64_t>* viol, std::vector<uint64_t>* err,
                        std::vector<uint64_t>* was_viol, std::vector<uint64_t>* was_err);
}  // namespace gk

static std::vector<uint32_t> key_order(const std::vector<std::string>& keys) {
  std::vector<uint32_t> o(keys.size());
  for (uint32_t i = 0; i < o.size(); i++) o[i] = i;
  std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  return o;
}
static void join(const std::vector<std::string>& now, const std::vector<std::string>& then, std::vector<uint32_t>* then_of, std::vector<uint32_t>* now_of,
                 std::vector<uint64_t>* unmatched) {
  delta_join(key_order(now), [&](uint32_t i) { return std::string_view(now[i]); }, key_order(then), [&](uint32_t i) { return std::string_view(then[i]); }, then_of, now_of,
             unmatched);
}

static void test_join() {
  const uint32_t N = DELTA_NONE;
  std::vector<uint32_t> then_of, now_of;
  std::vector<uint64_t> un;
  // duplicates match by occurrence; an empty key matches nothing; keys with an embedded NUL compare whole
  const std::vector<std::string> then = {"b", "a", "", "b", std::string("k\0x", 3), "z", "b"};
  const std::vector<std::string> now = {"", "b", std::string("k\0y", 3), "b", "a", "q", std::string("k\0x", 3)};
  join(now, then, &then_of, &now_of, &un);
  CHECK((then_of == std::vector<uint32_t>{N, 0, N, 3, 1, N, 4}));
  CHECK((now_of == std::vector<uint32_t>{1, 4, N, 3, 6, N, N}));
  CHECK(un.size() == 1 && un[0] == ((1ull << 2) | (1ull << 5) | (1ull << 6)));
  // more occurrences now than then
  join({"d", "d", "d"}, {"d"}, &then_of, &now_of, &un);
  CHECK((then_of == std::vector<uint32_t>{0, N, N}) && (now_of == std::vector<uint32_t>{0}) && un[0] == 0);
  // disjoint sets
  join({"a", "c"}, {"b", "d", "e"}, &then_of, &now_of, &un);
  CHECK((then_of == std::vector<uint32_t>{N, N}) && (now_of == std::vector<uint32_t>{N, N, N}) && un[0] == 7);
  // one side empty, both
  join({}, {"x", "y"}, &then_of, &now_of, &un);
  CHECK(then_of.empty() && now_of.size() == 2 && un[0] == 3);
  join({"x"}, {}, &then_of, &now_of, &un);
  CHECK((then_of == std::vector<uint32_t>{N}) && now_of.empty() && un.empty());
  join({}, {}, &then_of, &now_of, &un);
  CHECK(then_of.empty() && now_of.empty() && un.empty());
  // 130 gone reviews: three words, the last partial
  std::vector<std::string> many(130, "");
  for (uint32_t i = 0; i < 130; i++) many[i] = "o" + std::to_string(1000 + i);
  join({"o1064"}, many, &then_of, &now_of, &un);
  CHECK(then_of[0] == 64 && un.size() == 3 && un[0] == ~0ull && un[1] == ~1ull && un[2] == 3);
  std::printf("ok join\n");
}

static void test_rows() {
  const uint32_t N = DELTA_NONE;
  std::vector<uint32_t> row_of, now_row_of;
  delta_row_map({7, 3, 9, 12}, {3, 5, 7, 9}, &row_of, &now_row_of);   // 5 removed, 12 added, the rest reordered
  CHECK((row_of == std::vector<uint32_t>{2, 0, 3, N}) && (now_row_of == std::vector<uint32_t>{1, N, 0, 2}));
  delta_row_map({1, 2}, {}, &row_of, &now_row_of);
  CHECK((row_of == std::vector<uint32_t>{N, N}) && now_row_of.empty());
  delta_row_map({}, {1, 2}, &row_of, &now_row_of);
  CHECK(row_of.empty() && (now_row_of == std::vector<uint32_t>{N, N}));
  delta_row_map({4, 4}, {4}, &row_of, &now_row_of);   // (an id listed twice never happens; its first row wins)
  CHECK((row_of == std::vector<uint32_t>{0, N}) && (now_row_of == std::vector<uint32_t>{0}));
  std::printf("ok rows\n");
}

static void test_cursor() {
  const uint32_t words[2] = {5, 3};
  uint32_t side = 9, word = 9;
  CHECK(delta_cursor_pack(0, 0, 1) == 0 && delta_cursor_pack(1u << 28, 0, 1) == 0 && delta_cursor_pack(1, 2, 0) == 0 && delta_cursor_pack(1, 0, 1u << 31) == 0);
  const uint64_t a = delta_cursor_pack(7, 0, 4), b = delta_cursor_pack(7, 1, 2);
  CHECK(a && b && a != b);
  CHECK(delta_cursor_check(a, 7, words, &side, &word) && side == 0 && word == 4);
  CHECK(delta_cursor_check(b, 7, words, &side, &word) && side == 1 && word == 2);
  CHECK(!delta_cursor_check(a, 8, words, &side, &word) && !delta_cursor_check(0, 7, words, &side, &word) && !delta_cursor_check(a, 0, words, &side, &word));
  CHECK(!delta_cursor_check(delta_cursor_pack(7, 0, 5), 7, words, &side, &word) && !delta_cursor_check(delta_cursor_pack(7, 1, 3), 7, words, &side, &word));
  CHECK(delta_cursor_check(delta_cursor_pack((1u << 28) - 1, 1, 0), (1u << 28) - 1, words, &side, &word) && side == 1 && word == 0);
  std::printf("ok cursor\n");
}

static void test_pages() {
  // side 0: words 0 and 2 have entries, 1 and 3 none; side 1: only its word 1
  std::vector<uint64_t> entries, prefix[2];
  CHECK(delta_prefix({0x7, 0, ~0ull, 0}, {}, {}, &entries, &prefix[0]) && (prefix[0] == std::vector<uint64_t>{0, 3, 3, 67, 67}));
  CHECK(delta_prefix({0, 0x30, 0}, {0, 0x11, 0}, {0, 0x01, 0}, &entries, &prefix[1]));   // bit 4 dropped (known, no entry), bit 0 added, bit 5 the device's
  CHECK(entries[1] == 0x21 && (prefix[1] == std::vector<uint64_t>{0, 0, 2, 2}));
  CHECK(!delta_prefix({0, 0}, {0}, {}, &entries, &prefix[1]) && !delta_prefix({0}, {1}, {2}, &entries, &prefix[1]));   // sizes; extra outside drop
  CHECK(delta_prefix({0, 0x30, 0}, {0, 0x11, 0}, {0, 0x01, 0}, &entries, &prefix[1]));
  uint32_t side = 0, word = 0;
  CHECK(delta_next(prefix, &side, &word) && side == 0 && word == 0);
  CHECK(viol_page_end(prefix[0], 0, 64) == 2);    // words 0 and 1 fit, word 2 (64 more) does not
  side = 0; word = 2;
  CHECK(delta_next(prefix, &side, &word) && side == 0 && word == 2);
  CHECK(viol_page_end(prefix[0], 2, 1) == 4);     // below 64 counts as 64; the empty word behind it rides along
  side = 0; word = 3;                             // the side boundary: nothing left on side 0, the stream goes on at side 1's first word with entries
  CHECK(delta_next(prefix, &side, &word) && side == 1 && word == 1);
  CHECK(viol_page_end(prefix[1], 1, 1000000) == 3);
  side = 1; word = 2;
  CHECK(!delta_next(prefix, &side, &word));
  CHECK(viol_page_end(prefix[0], 0, 1000000) == 4);   // a page never crosses the sides: it ends with its side's words
  // nothing at all / only gone entries
  std::vector<uint64_t> none[2] = {{0, 0, 0}, {0, 0}};
  side = 0; word = 0;
  CHECK(!delta_next(none, &side, &word));
  std::vector<uint64_t> gone_only[2] = {{0, 0}, {0, 0, 5}};
  side = 0; word = 0;
  CHECK(delta_next(gone_only, &side, &word) && side == 1 && word == 1);
  std::vector<uint64_t> empty_sides[2] = {{0}, {0}};
  side = 0; word = 0;
  CHECK(!delta_next(empty_sides, &side, &word));
  std::printf("ok pages\n");
}

static void test_merge() {
  // rows now: ids {7, 3, 9} ; then: {3, 5, 7}: then row 0 -> now row 1, then row 1 dropped, then row 2 -> now row 0
  std::vector<uint32_t> row_of, now_row_of;
  delta_row_map({7, 3, 9}, {3, 5, 7}, &row_of, &now_row_of);
  // then reviews 0..3, now reviews 0..4; now 1 <- then 2, now 3 <- then 0, then 1 and 3 gone
  const std::vector<uint32_t> now_of = {3, DELTA_NONE, 1, DELTA_NONE};
  DeltaKnownMap now, gone;
  // the host answered now-review 1 (viol row 2) and now-review 4 (nothing); then it answered then-review 2 (viol rows 0 and 1, err row 2), then-review 3
  // (viol row 1: a dropped row) and then-review 1 (err row 0)
  delta_known_build({1, 4}, {{2, 1}, {0, 2}}, {}, 5, 3, {1, 2, 3}, {{0, 2}, {1, 2}, {1, 3}}, {{2, 2}, {0, 1}}, now_of, now_row_of, &now, &gone);
  CHECK(now.size() == 2 && gone.size() == 2);
  CHECK(now[1].now && now[1].was && now[1].nv[0] == 4 && now[1].ne[0] == 0 && now[1].wv[0] == 2 && now[1].we[0] == 1);   // (the pair of review 2, which the host did not answer now, is dropped)
  CHECK(now[4].now && !now[4].was && now[4].nv[0] == 0);
  CHECK(gone[1].was && !gone[1].now && gone[1].we[0] == 2 && gone[1].wv[0] == 0);
  CHECK(gone[3].was && gone[3].wv[0] == 0);   // only a dropped row: nothing in the rows of the table now
  CHECK((delta_known_words(now, 1) == std::vector<uint64_t>{0x12}) && (delta_known_words(gone, 1) == std::vector<uint64_t>{0xA}));
  // the device's entries of the word give review 4 its then-side (review 1's device masks are not taken: both sides are the host's)
  CHECK(delta_known_fill(&now, {1, 2, 4}, 1, {0xFF, 1, 0xFF}, {0xFF, 0, 0xFF}, {0xFF, 1, 6}, {0xFF, 2, 0}));
  CHECK(now[1].nv[0] == 4 && now[1].wv[0] == 2 && now[4].nv[0] == 0 && now[4].wv[0] == 6 && now[4].we[0] == 0);
  CHECK(!delta_known_fill(&now, {1}, 1, {}, {}, {}, {}));
  CHECK((delta_known_decide(now, 1, {}, {}) == std::vector<uint64_t>{0x12}));
  CHECK((delta_known_decide(now, 1, {}, {0x10}) == std::vector<uint64_t>{0x02}));   // review 4 beyond the limits and unanswered now: never an entry
  CHECK((delta_known_decide(gone, 1, {}, {}) == std::vector<uint64_t>{0x2}));       // then-review 3 had nothing in today's rows
  now[1].wv[0] = 4; now[1].we[0] = 0;                                               // equal masks: an entry only when its version moved
  CHECK((delta_known_decide(now, 1, {}, {}) == std::vector<uint64_t>{0x10}) && (delta_known_decide(now, 1, {0x02}, {}) == std::vector<uint64_t>{0x12}));
  now[1].nv[0] = 0; now[1].wv[0] = 0;                                               // ... and it has a result now
  CHECK((delta_known_decide(now, 1, {0x02}, {}) == std::vector<uint64_t>{0x10}));
  now[1].nv[0] = 4; now[1].wv[0] = 2; now[1].we[0] = 1;
  // a page of word 0: the device emitted 1, 2, 4 (1 and 4 through `extra`, with whatever its bitmaps hold); the host's masks replace them
  std::vector<uint64_t> v = {0xFF, 1, 0xFF}, e = {0xFF, 0, 0xFF}, wv = {0, 1, 0}, we = {0, 2, 0};
  CHECK(delta_merge_page(now, {1, 2, 4}, 1, 5, 0, 1, &v, &e, &wv, &we));
  CHECK((v == std::vector<uint64_t>{4, 1, 0}) && (e == std::vector<uint64_t>{0, 0, 0}) && (wv == std::vector<uint64_t>{2, 1, 6}) && (we == std::vector<uint64_t>{1, 2, 0}));
  CHECK(!delta_merge_page(now, {2, 1}, 1, 5, 0, 1, &v, &e, &wv, &we));   // not ascending
  std::vector<uint64_t> one = {0};
  CHECK(!delta_merge_page(now, {64}, 1, 65, 0, 1, &one, &one, &one, &one) && !delta_merge_page(now, {5}, 1, 5, 0, 1, &one, &one, &one, &one));
  CHECK(!delta_merge_page(now, {1}, 1, 5, 0, 1, &v, &one, &one, &one));   // sizes
  // the gone side
  std::vector<uint64_t> gv = {0}, ge = {0}, gwv = {0}, gwe = {0};
  CHECK(delta_merge_page(gone, {1}, 1, 4, 0, 1, &gv, &ge, &gwv, &gwe) && gwe[0] == 2 && gwv[0] == 0 && gv[0] == 0);
  std::printf("ok merge\n");
}

// ---- the stand-in against a bit-by-bit reference
struct Group { std::vector<uint64_t> viol, err, big; uint32_t nc, nt, row0; };
static bool bit(const std::vector<uint64_t>& v, size_t word, uint32_t b) { return (v[word] >> b) & 1ull; }

static void stand_in_case(std::mt19937_64& rng, const std::vector<uint32_t>& group_rows, uint32_t n, uint32_t n_then, uint32_t rows_then, bool with_moved, bool identity) {
  const uint32_t pw = (n + 63) / 64, spw = (n_then + 63) / 64;
  uint32_t rows = 0;
  std::vector<Group> gs;
  auto sparse = [&]() { return rng() & rng() & rng(); };
  for (uint32_t nc : group_rows) {
    Group g;
    g.nc = nc; g.nt = pw + (uint32_t)(rng() % 3); g.row0 = rows;
    g.viol.resize((size_t)nc * g.nt); g.err.resize((size_t)nc * g.nt); g.big.resize(g.nt);
    for (auto& x : g.viol) x = sparse();
    for (auto& x : g.err) x = sparse() & rng();
    for (auto& x : g.big) x = sparse() & rng() & rng();
    rows += nc;
    gs.push_back(g);
  }
  if (identity) { CHECK(n == n_then); }
  // the snapshot, flat
  std::vector<uint64_t> sv((size_t)rows_then * spw), se(sv.size()), sb(spw);
  for (auto& x : sv) x = sparse();
  for (auto& x : se) x = sparse() & rng();
  for (auto& x : sb) x = sparse() & rng() & rng();
  // a random partial injection of the table's reviews into the snapshot's, a random row map
  std::vector<uint32_t> perm(n_then), then_of(n, DELTA_NONE), row_of(rows, DELTA_NONE), rperm(rows_then);
  for (uint32_t i = 0; i < n_then; i++) perm[i] = i;
  std::shuffle(perm.begin(), perm.end(), rng);
  for (uint32_t i = 0, k = 0; i < n && k < n_then; i++) if (rng() % 8) then_of[i] = perm[k++];
  for (uint32_t i = 0; i < rows_then; i++) rperm[i] = i;
  std::shuffle(rperm.begin(), rperm.end(), rng);
  for (uint32_t r = 0, k = 0; r < rows && k < rows_then; r++) if (rng() % 5) row_of[r] = rperm[k++];
  if (identity) for (uint32_t i = 0; i < n; i++) then_of[i] = i;
  std::vector<uint64_t> moved(pw), only(pw);
  for (auto& x : moved) x = sparse();
  for (auto& x : only) x = rng() | rng();
  const uint64_t* mv = with_moved ? moved.data() : nullptr;
  const uint64_t* on = identity ? only.data() : nullptr;
  // the stand-in
  std::vector<TchgGroup> tg;
  if (!identity) for (const Group& g : gs) tg.push_back(TchgGroup{g.viol.data(), g.err.data(), g.big.data(), g.nc, g.nt, g.row0});
  std::vector<uint64_t> fv, fe, fb, wv, we, wb;
  tchg_flatten_words(tg, rows, pw, &fv, &fe, &fb);
  const TchgFlat snap{sv.data(), se.data(), sb.data(), rows_then, spw, n_then};
  tchg_align_words(snap, n, identity ? nullptr : then_of.data(), row_of, &wv, &we, &wb);
  const TchgFlat nowf{identity ? nullptr : fv.data(), identity ? nullptr : fe.data(), identity ? nullptr : fb.data(), rows, pw, n};
  const TchgFlat wasf{wv.data(), we.data(), wb.data(), rows, pw, n};
  std::vector<uint32_t> cnt;
  std::vector<uint64_t> changed, big;
  uint64_t beyond = 0;
  tchg_index_words(nowf, wasf, mv, on, &cnt, &changed, &big, &beyond);
  // the reference, review by review and bit by bit
  const uint32_t mw = (rows + 63) / 64;
  std::vector<uint64_t> ref_changed(pw, 0), ref_big(pw, 0);
  std::vector<std::vector<uint64_t>> masks(n, std::vector<uint64_t>(4 * (size_t)mw, 0));
  uint64_t ref_beyond = 0;
  for (uint32_t i = 0; i < n; i++) {
    bool too_big = false, any = false, differs = false;
    if (!identity) for (const Group& g : gs) too_big = too_big || bit(g.big, i / 64, i % 64);
    const uint32_t p = then_of[i];
    const bool was_big = p != DELTA_NONE && bit(sb, p / 64, p % 64);
    if (!identity)
      for (const Group& g : gs)
        for (uint32_t r = 0; r < g.nc; r++) {
          if (bit(g.viol, (size_t)r * g.nt + i / 64, i % 64)) masks[i][(g.row0 + r) / 64] |= 1ull << ((g.row0 + r) % 64);
          if (bit(g.err, (size_t)r * g.nt + i / 64, i % 64)) masks[i][mw + (g.row0 + r) / 64] |= 1ull << ((g.row0 + r) % 64);
        }
    for (uint32_t r = 0; r < rows; r++) {
      if (p == DELTA_NONE || was_big || row_of[r] == DELTA_NONE) continue;
      if (bit(sv, (size_t)row_of[r] * spw + p / 64, p % 64)) masks[i][2 * (size_t)mw + r / 64] |= 1ull << (r % 64);
      if (bit(se, (size_t)row_of[r] * spw + p / 64, p % 64)) masks[i][3 * (size_t)mw + r / 64] |= 1ull << (r % 64);
    }
    for (uint32_t k = 0; k < mw; k++) {
      any = any || masks[i][k] || masks[i][mw + k];
      differs = differs || masks[i][k] != masks[i][2 * (size_t)mw + k] || masks[i][mw + k] != masks[i][3 * (size_t)mw + k];
    }
    if (too_big) { ref_big[i / 64] |= 1ull << (i % 64); ref_beyond++; continue; }
    if (on && !bit(only, i / 64, i % 64)) continue;
    if (differs || (mv && any && bit(moved, i / 64, i % 64))) ref_changed[i / 64] |= 1ull << (i % 64);
  }
  CHECK(changed == ref_changed && big == ref_big && beyond == ref_beyond);
  for (uint32_t w = 0; w < pw; w++) CHECK(cnt[w] == (uint32_t)__builtin_popcountll(changed[w]));
  // entries of a word range under random drop / extra words
  const uint32_t w0 = pw > 2 ? 1 : 0, w1 = pw;
  std::vector<uint64_t> drop(w1 - w0), extra(w1 - w0);
  for (uint32_t w = w0; w < w1; w++) { drop[w - w0] = sparse(); extra[w - w0] = drop[w - w0] & rng(); }
  std::vector<uint32_t> rev;
  std::vector<uint64_t> ev, ee, ewv, ewe;
  tchg_entries_words(nowf, wasf, mv, on, w0, w1, drop.data(), extra.data(), &rev, &ev, &ee, &ewv, &ewe);
  size_t at = 0;
  for (uint32_t i = w0 * 64; i < n; i++) {
    const uint64_t b = 1ull << (i % 64);
    const bool in = ((ref_changed[i / 64] & ~drop[i / 64 - w0]) | extra[i / 64 - w0]) & b;
    if (!in) continue;
    CHECK(at < rev.size() && rev[at] == i);
    for (uint32_t k = 0; k < mw; k++) {
      CHECK(ev[at * mw + k] == masks[i][k] && ee[at * mw + k] == masks[i][mw + k]);
      CHECK(ewv[at * mw + k] == masks[i][2 * (size_t)mw + k] && ewe[at * mw + k] == masks[i][3 * (size_t)mw + k]);
    }
    at++;
  }
  CHECK(at == rev.size() && ev.size() == at * mw && ewe.size() == at * mw);
}

static void test_stand_in() {
  std::mt19937_64 rng(20261021);
  std::vector<uint32_t> eleven(11, 5);
  eleven[3] = 1; eleven[7] = 23;
  for (uint32_t n : {1u, 63u, 64u, 65u, 200u, 1000u}) {
    for (bool moved : {false, true}) {
      stand_in_case(rng, {1}, n, n + 3, 1, moved, false);
      stand_in_case(rng, {50}, n, n > 10 ? n - 7 : n, 64, moved, false);          // one group
      stand_in_case(rng, {50, 50, 30}, n, n + 70, 129, moved, false);             // three groups whose rows straddle a mask word
      stand_in_case(rng, eleven, n, n, 70, moved, false);                         // eleven groups
      stand_in_case(rng, {200, 60}, n, n + 1, 300, moved, false);                 // five mask words
    }
    stand_in_case(rng, {70}, n, n, 70, false, true);                                // the gone side: no groups, the identity, `only`
    stand_in_case(rng, {260}, n, n, 300, false, true);
  }
  std::printf("ok stand_in\n");
}

int main() {
  test_join();
  test_rows();
  test_cursor();
  test_pages();
  test_merge();
  test_stand_in();
  return 0;
}
