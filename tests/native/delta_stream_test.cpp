// Stand-alone test of the resident-set changes stream's pieces that need no engine and no device (built and run, with and without
// sanitizers, by tests/test_delta_stream_native.py; tests/test_resident_changes.py checks the whole path against the oracle):
//   * the CPU stand-in of dev_delta_keep / dev_delta_index / dev_delta_entries / dev_delta_drop (hostemu_delta.cpp, compiled into this
//     program) against a bit-by-bit reference over seeded random now / base / shown_now / shown_base bitmaps;
//   * csrc/delta_stream.hpp: the host-side diff of the sparse (slot, row) pair lists.
// hostemu_delta.cpp needs only device.hpp's public dev_last_viol, which this program supplies over a table type of its own.
#include <cstdio>
#include <set>
#include <stdexcept>
#include <vector>

#include "delta_stream.hpp"
#include "device.hpp"

namespace gk {
struct DevTable { std::vector<uint64_t> viol; };
void dev_last_viol(const DevTable* t, uint32_t, std::vector<uint64_t>* viol) { *viol = t->viol; }
}  // namespace gk

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // SplitMix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// about one bit in 2^k set
static uint64_t sparse(int k) { uint64_t x = ~0ull; for (int i = 0; i < k; i++) x &= rnd(); return x; }

template <class F> static bool throws(F&& f) { try { f(); } catch (const std::runtime_error&) { return true; } return false; }

struct Ref { std::vector<uint32_t> reviews; std::vector<uint64_t> now, was; };
static bool bit(const std::vector<uint64_t>& v, size_t word, uint32_t b) { return (v[word] >> b) & 1ull; }
// bit by bit, review by review: no word arithmetic shared with the code under test
static Ref reference(const std::vector<uint64_t>& now, const std::vector<uint64_t>* base, const std::vector<uint64_t>& sn, const std::vector<uint64_t>& sb, uint32_t nc,
                     uint32_t nt, uint32_t n, uint32_t w0, uint32_t w1, const std::vector<uint64_t>* extra, std::vector<uint32_t>* cnt, std::vector<uint64_t>* changed) {
  Ref out;
  const uint32_t mw = (nc + 63u) / 64u, pw = (n + 63u) / 64u;
  cnt->assign(pw, 0); changed->assign(pw, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t w = i / 64u, b = i % 64u;
    std::vector<uint64_t> a(mw, 0), z(mw, 0);
    for (uint32_t r = 0; r < nc; r++) {
      if (bit(sn, w, b) && bit(now, (size_t)r * nt + w, b)) a[r / 64u] |= 1ull << (r % 64u);
      if (base && bit(sb, w, b) && bit(*base, (size_t)r * nt + w, b)) z[r / 64u] |= 1ull << (r % 64u);
    }
    const bool differs = a != z;
    if (differs) { (*cnt)[w]++; (*changed)[w] |= 1ull << b; }
    if (w < w0 || w >= w1) continue;
    if (differs || (extra && bit(*extra, w - w0, b))) {
      out.reviews.push_back(i);
      out.now.insert(out.now.end(), a.begin(), a.end());
      out.was.insert(out.was.end(), z.begin(), z.end());
    }
  }
  return out;
}

static void stand_in_case(uint32_t n, uint32_t nc, bool with_base, int density) {
  const uint32_t pw = (n + 63u) / 64u, nt = pw + (uint32_t)(rnd() % 3u);   // (rows may be longer than the words that carry reviews)
  gk::DevTable t;
  std::vector<uint64_t> base((size_t)nc * nt), sn(pw), sb(pw);
  t.viol.resize((size_t)nc * nt);
  for (auto& x : base) x = sparse(density);
  // now = base with a few bits moved, so that most words do not change at all
  for (size_t i = 0; i < base.size(); i++) t.viol[i] = base[i] ^ sparse(density + 3);
  for (uint32_t w = 0; w < pw; w++) { sb[w] = ~sparse(4); sn[w] = sb[w] ^ sparse(6); }
  if (pw >= 3 && nc >= 1) {
    // word 0: changed only in base (a bit that is shown on both sides and set at the baseline alone)
    for (uint32_t r = 0; r < nc; r++) { t.viol[(size_t)r * nt] = 0; base[(size_t)r * nt] = 0; }
    sn[0] = sb[0] = ~0ull;
    base[(size_t)(nc - 1) * nt] = 1ull << 17;
    // word 1: changed only in shown (equal bitmaps, one review no longer shown)
    for (uint32_t r = 0; r < nc; r++) t.viol[(size_t)r * nt + 1] = base[(size_t)r * nt + 1] = (r == 0 ? 1ull << 5 : 0ull);
    sb[1] = ~0ull; sn[1] = ~(1ull << 5);
  }
  if (n % 64u) {
    // the last word: changed in bits at or beyond n only -- no entry
    const uint64_t beyond = ~((1ull << (n % 64u)) - 1ull);
    for (uint32_t r = 0; r < nc; r++) { t.viol[(size_t)r * nt + pw - 1] = base[(size_t)r * nt + pw - 1] & ~beyond; base[(size_t)r * nt + pw - 1] |= beyond & rnd(); }
    sn[pw - 1] = sb[pw - 1] = ~0ull;
  }
  // the baseline is what dev_delta_keep copies: evaluate "then", keep, evaluate "now"
  const std::vector<uint64_t> now = t.viol;
  gk::dev_delta_drop(&t);
  CHECK(!gk::dev_delta_has(&t, nc) && gk::dev_delta_bytes(&t) == 0);
  if (with_base) {
    t.viol = base;
    gk::dev_delta_keep(&t, nc, n, sb, 1);
    t.viol = now;
    CHECK(gk::dev_delta_has(&t, nc) && !gk::dev_delta_has(&t, nc + 1) && gk::dev_delta_bytes(&t) == ((uint64_t)nc * nt + pw) * 8u);
  }
  std::vector<uint32_t> cnt, want_cnt;
  std::vector<uint64_t> changed, want_changed;
  float ms = 1;
  gk::dev_delta_index(&t, nc, n, sn, 2, true, &cnt, &changed, &ms);
  reference(now, with_base ? &base : nullptr, sn, sb, nc, nt, n, 0, 0, nullptr, &want_cnt, &want_changed);
  CHECK(cnt == want_cnt && changed == want_changed && ms == 0);
  if (pw >= 3 && with_base) CHECK(changed[0] == 1ull << 17 && changed[1] == 1ull << 5);
  if (n % 64u && with_base) CHECK(changed[pw - 1] == 0);
  // use_base = false: the baseline reads as zero although one is kept
  gk::dev_delta_index(&t, nc, n, sn, 2, false, &cnt, &changed, &ms);
  reference(now, nullptr, sn, sb, nc, nt, n, 0, 0, nullptr, &want_cnt, &want_changed);
  CHECK(cnt == want_cnt && changed == want_changed);
  // pages: the whole table, every single word, a run that begins at a nonzero word; with and without merged words from other sources
  gk::dev_delta_index(&t, nc, n, sn, 2, true, &cnt, &changed, &ms);
  std::vector<uint32_t> off(pw + 1, 0);
  for (uint32_t w = 0; w < pw; w++) off[w + 1] = off[w] + cnt[w];
  auto page = [&](uint32_t w0, uint32_t w1, bool merged) {
    std::vector<uint64_t> extra(w1 - w0);
    for (auto& x : extra) x = sparse(4);
    std::vector<uint32_t> o(w1 - w0 + 1, 0);
    for (uint32_t w = w0; w < w1; w++) {
      uint64_t m = changed[w] | (merged ? extra[w - w0] : 0ull);
      if (n - w * 64u < 64u) m &= (1ull << (n - w * 64u)) - 1ull;
      o[w - w0 + 1] = o[w - w0] + (uint32_t)__builtin_popcountll(m);
    }
    std::vector<uint32_t> rev;
    std::vector<uint64_t> a, z;
    gk::dev_delta_entries(&t, nc, n, sn, 2, true, w0, w1, o, merged ? &extra : nullptr, &rev, &a, &z, &ms);
    if (merged && n % 64u && w1 == pw) extra.back() &= (1ull << (n % 64u)) - 1ull;   // (the reference walks the reviews below n only)
    const Ref want = reference(now, with_base ? &base : nullptr, sn, sb, nc, nt, n, w0, w1, merged ? &extra : nullptr, &want_cnt, &want_changed);
    CHECK(rev == want.reviews && a == want.now && z == want.was);
    if (!merged) CHECK(rev.size() == off[w1] - off[w0]);
  };
  page(0, pw, false); page(0, pw, true);
  if (pw <= 4) for (uint32_t w = 0; w < pw; w++) { page(w, w + 1, false); page(w, w + 1, true); }
  if (pw > 2) { page(1, pw, false); page(pw / 2, pw, true); page(pw - 1, pw, false); page(1, 1, false); }
  // what the device entries refuse: an index of other bitmaps, a range beyond the table, a baseline of another row count
  std::vector<uint32_t> rev;
  std::vector<uint64_t> a, z;
  std::vector<uint32_t> wrong(pw + 1, 0);
  for (uint32_t w = 0; w < pw; w++) wrong[w + 1] = wrong[w] + cnt[w] + (w == 0 ? 1u : 0u);
  CHECK(throws([&] { gk::dev_delta_entries(&t, nc, n, sn, 2, true, 0, pw, wrong, nullptr, &rev, &a, &z, &ms); }));
  CHECK(throws([&] { gk::dev_delta_entries(&t, nc, n, sn, 2, true, 0, pw + 1, std::vector<uint32_t>(pw + 2, 0), nullptr, &rev, &a, &z, &ms); }));
  CHECK(throws([&] { gk::dev_delta_entries(&t, nc, n, sn, 2, true, 0, pw, std::vector<uint32_t>(pw, 0), nullptr, &rev, &a, &z, &ms); }));
  if (with_base && nc > 1) {
    gk::DevTable other = t;
    other.viol.resize((size_t)(nc - 1) * nt);
    gk::dev_delta_keep(&other, nc - 1, n, sb, 1);
    other.viol = now;
    CHECK(throws([&] { gk::dev_delta_index(&other, nc, n, sn, 2, true, &cnt, &changed, &ms); }));
    gk::dev_delta_drop(&other);
  }
  gk::dev_delta_drop(&t);
  CHECK(!gk::dev_delta_has(&t, nc));
}

static void stand_in_cases() {
  for (uint32_t n : {1u, 63u, 64u, 65u, 130u, 16500u})
    for (uint32_t nc : {1u, 3u, 5u, 64u, 65u, 70u}) {
      for (bool with_base : {true, false}) stand_in_case(n, nc, with_base, n > 1000u ? 6 : 2);
    }
  gk::DevTable empty;
  std::vector<uint32_t> cnt;
  std::vector<uint64_t> changed;
  float ms = 0;
  CHECK(throws([&] { gk::dev_delta_index(&empty, 3, 10, {0}, 1, true, &cnt, &changed, &ms); }));   // never evaluated
  CHECK(throws([&] { gk::dev_delta_keep(&empty, 3, 10, {0}, 1); }));
  printf(failures ? "FAILED stand_in\n" : "ok stand_in\n");
}

static void pair_cases() {
  using gk::DeltaPair;
  const int before = failures;
  std::vector<DeltaPair> v = {{7, 2}, {3, 1}, {7, 2}, {3, 0}, {100, 69}};
  gk::delta_pairs_sort(&v);
  CHECK((v == std::vector<DeltaPair>{{3, 0}, {3, 1}, {7, 2}, {100, 69}}));
  CHECK(gk::delta_pairs_changed(v, v).empty() && gk::delta_pairs_changed({}, {}).empty());
  CHECK((gk::delta_pairs_changed(v, {}) == std::vector<uint32_t>{3, 7, 100}));                       // everything is new: each slot once
  CHECK((gk::delta_pairs_changed({}, v) == std::vector<uint32_t>{3, 7, 100}));                       // everything resolved
  CHECK((gk::delta_pairs_changed(v, {{3, 0}, {3, 1}, {7, 3}, {100, 69}}) == std::vector<uint32_t>{7}));   // another row of the same slot
  CHECK((gk::delta_pairs_changed(v, {{3, 0}, {7, 2}, {100, 69}, {101, 0}}) == std::vector<uint32_t>{3, 101}));
  // random lists against sets
  for (int round = 0; round < 200; round++) {
    std::set<DeltaPair> a, b;
    for (int i = 0; i < 40; i++) { a.insert({(uint32_t)(rnd() % 50u), (uint32_t)(rnd() % 70u)}); if (rnd() % 3u) b.insert({(uint32_t)(rnd() % 50u), (uint32_t)(rnd() % 70u)}); }
    for (const DeltaPair& p : a) if (rnd() % 2u) b.insert(p);
    const std::vector<DeltaPair> av(a.begin(), a.end()), bv(b.begin(), b.end());
    std::set<uint32_t> want;
    for (const DeltaPair& p : a) if (!b.count(p)) want.insert(p.first);
    for (const DeltaPair& p : b) if (!a.count(p)) want.insert(p.first);
    CHECK(gk::delta_pairs_changed(av, bv) == std::vector<uint32_t>(want.begin(), want.end()));
    // the page: some slots, two mask words; rows at or beyond `rows` are dropped
    std::vector<uint32_t> slots;
    for (uint32_t s = 0; s < 50; s++) if (rnd() % 2u) slots.push_back(s);
    const uint32_t rows = 1u + (uint32_t)(rnd() % 70u);
    std::vector<uint64_t> got(slots.size() * 2u, 0), exp(slots.size() * 2u, 0);
    gk::delta_pairs_or(av, slots, 2, rows, &got);
    for (size_t i = 0; i < slots.size(); i++)
      for (const DeltaPair& p : a) if (p.first == slots[i] && p.second < rows) exp[i * 2u + p.second / 64u] |= 1ull << (p.second % 64u);
    CHECK(got == exp);
  }
  std::vector<uint64_t> none;
  gk::delta_pairs_or(v, {}, 2, 70, &none);
  CHECK(none.empty());
  printf(failures != before ? "FAILED pairs\n" : "ok pairs\n");
}

int main() {
  stand_in_cases();
  pair_cases();
  return failures ? 1 : 0;
}
