// Stand-alone program (its own main; never loaded into Python; built plain and with -fsanitize=address,undefined by
// tests/test_verify_native.py) for the host side of gk_table_verify / gk_resident_verify:
//   * csrc/verify_merge.hpp: the merge of the plan groups' and chunks' answers -- row bases, review bases, the sort, the truncation;
//   * the CPU stand-in of dev_verify_diff / dev_verify_flip (hostemu_verify.cpp, compiled into this program) against a bit-by-bit
//     reference over seeded random bitmaps: tail masks, a review beyond the limits on either side, the caller's mask, a capacity
//     smaller than the differences.
// hostemu_verify.cpp needs only device.hpp's public dev_eval_launch / dev_eval_finish / dev_plan_upload, which this program supplies
// over table and plan types of its own: an "evaluation" hands out the bitmaps the case put into the table.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <tuple>
#include <vector>

#include "device.hpp"
#include "verify_merge.hpp"

namespace gk {
struct DevTable { std::vector<uint64_t> v[4]; uint32_t n = 0, nc = 0; };
struct DevPlan { int unused = 0; };
void dev_eval_launch(const DevPlan*, const DevTable*, const EvalOptions&) {}
void dev_eval_finish(const DevPlan*, const DevTable* t, const EvalOptions& opt, EvalOut* o) {
  if (!opt.download) throw std::runtime_error("the stand-in evaluates with download");
  o->n_reviews = t->n; o->n_constraints = t->nc; o->n_tiles = (t->n + 63) / 64;
  o->viol = t->v[0]; o->err = t->v[1]; o->too_big = t->v[3];
  o->match.clear();
  if (opt.want_match) o->match = t->v[2];
}
static int plans_uploaded = 0;
DevPlan* dev_plan_upload(int, const HostPlan&, const HostPlan&) { plans_uploaded++; return new DevPlan(); }
}  // namespace gk

// both sides of a verification through the stand-in's dev_verify_eval, as the engine does it
static void eval_sides(gk::DevTable* a, gk::DevTable* b, uint32_t nc, bool want_match) {
  static gk::DevPlan plan;
  a->nc = b->nc = nc;
  gk::EvalOptions oa;
  oa.download = false; oa.want_match = want_match;
  gk::EvalOptions ob = oa;
  ob.bytecode = true;
  gk::EvalOut ea, eb;
  gk::dev_verify_eval(&plan, a, oa, &ea);
  gk::dev_verify_eval(&plan, b, ob, &eb);
  if (eb.specialised) throw std::runtime_error("a bytecode evaluation counts as specialised");
}

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t> Ent;   // kind, row, review, a_bit
static std::vector<Ent> sorted_entries(const std::vector<gk::VerifyEntry>& v) {
  std::vector<Ent> out;
  for (const gk::VerifyEntry& e : v) out.emplace_back(e.kind, e.row, e.review, e.a_bit);
  std::sort(out.begin(), out.end());
  return out;
}

// bit by bit: review r of row c differs for kind k iff the bits differ, r < n, r is in the mask and in neither side's too_big
static void reference(const gk::DevTable& a, const gk::DevTable& b, uint32_t nc, uint32_t n, bool want_match, const std::vector<uint64_t>* mask, gk::VerifyDiff* out,
                      std::vector<Ent>* all) {
  const uint32_t pw = (n + 63) / 64;
  auto bit = [&](const std::vector<uint64_t>& v, size_t row, uint32_t r) { return (uint32_t)((v[row * pw + r / 64] >> (r % 64)) & 1ull); };
  for (int k = 0; k < 3; k++) out->diff[k].assign(k < 2 || want_match ? nc : 0, 0);
  out->diff_too_big = 0;
  all->clear();
  for (uint32_t r = 0; r < n; r++) {
    if (mask && !(((*mask)[r / 64] >> (r % 64)) & 1ull)) continue;
    const uint32_t ba = bit(a.v[3], 0, r), bb = bit(b.v[3], 0, r);
    if (ba != bb) { out->diff_too_big++; all->emplace_back(gk::VERIFY_TOO_BIG, 0u, r, ba); }
    if (ba || bb) continue;
    for (uint32_t k = 0; k < (want_match ? 3u : 2u); k++)
      for (uint32_t c = 0; c < nc; c++)
        if (bit(a.v[k], c, r) != bit(b.v[k], c, r)) { out->diff[k][c]++; all->emplace_back(k, c, r, bit(a.v[k], c, r)); }
  }
  std::sort(all->begin(), all->end());
}

static void stand_in_case(uint32_t n, uint32_t nc, bool want_match, bool with_mask, uint32_t density /* one difference in 2^density bits */, uint32_t cap) {
  const uint32_t pw = (n + 63) / 64;
  gk::DevTable a, b;
  a.n = b.n = n;
  for (int k = 0; k < 3; k++) { a.v[k].resize((size_t)nc * pw); for (auto& w : a.v[k]) w = rnd(); b.v[k] = a.v[k]; }
  a.v[3].assign(pw, 0); b.v[3].assign(pw, 0);
  // differences everywhere, the bits beyond n included (the two kernels owe nothing there: garbage on both sides)
  for (int k = 0; k < 3; k++) for (auto& w : b.v[k]) { uint64_t m = ~0ull; for (uint32_t d = 0; d < density; d++) m &= rnd(); w ^= m; }
  if (n % 64) for (uint32_t c = 0; c < nc; c++) a.v[c % 3][(size_t)c * pw + pw - 1] ^= ~0ull << (n % 64);
  for (uint32_t i = 0; i < n / 16 + 2 && n; i++) {   // reviews beyond the limits: on both sides, on a alone, on b alone
    const uint32_t r = (uint32_t)(rnd() % n), how = (uint32_t)(rnd() % 3);
    if (how != 2) a.v[3][r / 64] |= 1ull << (r % 64);
    if (how != 1) b.v[3][r / 64] |= 1ull << (r % 64);
  }
  std::vector<uint64_t> mask(pw);
  for (auto& w : mask) w = rnd() | rnd();
  gk::VerifyDiff got, want;
  std::vector<Ent> all;
  reference(a, b, nc, n, want_match, with_mask ? &mask : nullptr, &want, &all);
  eval_sides(&a, &b, nc, want_match);
  gk::dev_verify_diff(&a, &b, nc, n, want_match, with_mask ? &mask : nullptr, cap, &got);
  gk::dev_verify_forget(&a); gk::dev_verify_forget(&b);
  for (int k = 0; k < 3; k++) CHECK(got.diff[k] == want.diff[k]);
  CHECK(got.diff_too_big == want.diff_too_big);
  CHECK(got.entries_total == all.size());
  CHECK(got.entries.size() == std::min<size_t>(all.size(), cap));
  const std::vector<Ent> ge = sorted_entries(got.entries);
  CHECK(std::adjacent_find(ge.begin(), ge.end()) == ge.end());                       // no entry twice
  CHECK(std::includes(all.begin(), all.end(), ge.begin(), ge.end()));                 // each a real difference, with the right bit of side a
  if (cap >= all.size()) CHECK(ge == all);
}

static void stand_in_cases() {
  for (uint32_t n : {1u, 8u, 63u, 64u, 65u, 200u, 8200u})
    for (uint32_t nc : {1u, 3u, 50u})
      for (int m = 0; m < 4; m++) {
        if (n == 8200u && nc == 50u && m) continue;
        stand_in_case(n, nc, (m & 1) != 0, (m & 2) != 0, 6, 1u << 20);
        stand_in_case(n, nc, (m & 1) != 0, (m & 2) != 0, 2, 16);   // fewer entries than differences
        stand_in_case(n, nc, (m & 1) != 0, (m & 2) != 0, 64, 16);  // (next to) equal bitmaps; exactly equal ones below
      }
  {   // exactly equal: nothing at all, also with garbage beyond n on one side
    gk::DevTable a, b;
    a.n = b.n = 200;
    for (int k = 0; k < 3; k++) { a.v[k].assign(4 * 5, 0x5555AAAA5555AAAAull); b.v[k] = a.v[k]; }
    a.v[3].assign(4, 0); b.v[3].assign(4, 0);
    for (uint32_t c = 0; c < 5; c++) b.v[0][c * 4 + 3] ^= ~0ull << 8;   // bits 200..255
    gk::VerifyDiff d;
    bool threw = false;
    try { gk::dev_verify_diff(&a, &b, 5, 200, true, nullptr, 64, &d); } catch (const std::exception&) { threw = true; }   // nothing evaluated yet
    CHECK(threw);
    eval_sides(&a, &b, 5, true);
    gk::dev_verify_diff(&a, &b, 5, 200, true, nullptr, 64, &d);
    CHECK(d.entries_total == 0 && d.entries.empty() && d.diff_too_big == 0);
    for (int k = 0; k < 3; k++) CHECK(d.diff[k] == std::vector<uint64_t>(5, 0));
    // the flip: one bit, then the word that holds 8 valid reviews
    gk::dev_verify_flip(&b, 5, gk::VERIFY_ERR, 4, 64, false);
    gk::dev_verify_diff(&a, &b, 5, 200, false, nullptr, 64, &d);
    CHECK(d.entries_total == 1 && d.diff[1][4] == 1 && d.diff[2].empty());
    CHECK(sorted_entries(d.entries) == std::vector<Ent>{Ent(gk::VERIFY_ERR, 4, 64, (uint32_t)((a.v[1][4 * 4 + 1]) & 1ull))});
    gk::dev_verify_flip(&b, 5, gk::VERIFY_ERR, 4, 64, false);
    gk::dev_verify_flip(&b, 5, gk::VERIFY_VIOL, 2, 199, true);
    gk::dev_verify_diff(&a, &b, 5, 200, false, nullptr, 64, &d);
    CHECK(d.entries_total == 8 && d.diff[0][2] == 8);
    gk::dev_verify_flip(&b, 5, gk::VERIFY_TOO_BIG, 3, 7, false);   // (row ignored)
    gk::dev_verify_diff(&a, &b, 5, 200, false, nullptr, 64, &d);
    CHECK(d.diff_too_big == 1 && d.entries_total == 9);
    threw = false;
    try { gk::dev_verify_flip(&b, 5, gk::VERIFY_VIOL, 5, 0, false); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { gk::dev_verify_flip(&b, 5, gk::VERIFY_VIOL, 0, 200, false); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { gk::dev_verify_diff(&a, &b, 6, 200, false, nullptr, 64, &d); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    // an evaluation behind the flips brings the table's own bitmaps back; the twin: none without GK_HOSTEMU_JIT, one uploaded without it otherwise
    eval_sides(&a, &b, 5, false);
    gk::dev_verify_diff(&a, &b, 5, 200, false, nullptr, 64, &d);
    CHECK(d.entries_total == 0 && d.diff_too_big == 0);
    gk::HostPlan hp;
    unsetenv("GK_HOSTEMU_JIT");
    CHECK(gk::dev_verify_twin(0, hp, hp) == nullptr && gk::plans_uploaded == 0);
    setenv("GK_HOSTEMU_JIT", "1", 1);
    gk::DevPlan* twin = gk::dev_verify_twin(0, hp, hp);
    CHECK(twin != nullptr && gk::plans_uploaded == 1 && getenv("GK_HOSTEMU_JIT") != nullptr);
    delete twin;
    gk::EvalOut ea;
    gk::EvalOptions oa;
    static gk::DevPlan plan;
    gk::dev_verify_eval(&plan, &a, oa, &ea);
    CHECK(ea.specialised);
    unsetenv("GK_HOSTEMU_JIT");
    gk::dev_verify_forget(&a); gk::dev_verify_forget(&b);
  }
  printf(failures ? "FAILED stand_in\n" : "ok stand_in\n");
}

static gk::VerifyDiff group_of(uint32_t nc, bool want_match, std::vector<gk::VerifyEntry> entries, uint64_t extra_total, uint64_t too_big) {
  gk::VerifyDiff d;
  for (int k = 0; k < 3; k++) d.diff[k].assign(k < 2 || want_match ? nc : 0, 0);
  for (const gk::VerifyEntry& e : entries) if (e.kind < 3) d.diff[e.kind][e.row]++;
  d.diff_too_big = too_big;
  d.entries_total = entries.size() + extra_total;
  d.entries = std::move(entries);
  d.ms = 0.5f;
  return d;
}

static void merge_cases() {
  using gk::VerifyEntry;
  const int before = failures;
  // three plan groups of 3, 2 and 4 rows over one table; the second chunk of a resident set behind 1000 slots
  gk::VerifyMerge m;
  m.begin(9, true);
  m.add(group_of(3, true, {VerifyEntry{0, 2, 70, 1}, VerifyEntry{2, 0, 5, 0}, VerifyEntry{3, 0, 9, 1}}, 0, 1), 0, 0);
  m.add(group_of(2, true, {VerifyEntry{0, 1, 3, 0}, VerifyEntry{0, 0, 3, 1}}, 0, 0), 3, 0);
  m.add(group_of(4, true, {VerifyEntry{1, 3, 0, 1}, VerifyEntry{0, 0, 1, 0}}, 5, 0), 5, 0);
  m.add(group_of(3, true, {VerifyEntry{0, 2, 70, 0}, VerifyEntry{3, 0, 9, 0}}, 0, 1), 0, 1000);
  m.add(group_of(2, true, {}, 0, 0), 3, 1000);
  m.add(group_of(4, true, {VerifyEntry{1, 3, 0, 1}}, 0, 0), 5, 1000);
  CHECK(m.diff[0] == (std::vector<uint64_t>{0, 0, 2, 1, 1, 1, 0, 0, 0}));
  CHECK(m.diff[1] == (std::vector<uint64_t>{0, 0, 0, 0, 0, 0, 0, 0, 2}));
  CHECK(m.diff[2] == (std::vector<uint64_t>{1, 0, 0, 0, 0, 0, 0, 0, 0}));
  CHECK(m.diff_too_big == 2 && m.entries_total == 15 && m.diff_total() == 10 && m.ms == 3.0f);
  gk::VerifyMerge all = m;
  all.finish(100);
  const std::vector<Ent> want = {Ent(0, 2, 70, 1), Ent(0, 2, 1070, 0), Ent(0, 3, 3, 1), Ent(0, 4, 3, 0), Ent(0, 5, 1, 0), Ent(1, 8, 0, 1), Ent(1, 8, 1000, 1),
                                 Ent(2, 0, 5, 0), Ent(3, 0, 9, 1), Ent(3, 0, 1009, 0)};
  std::vector<Ent> got;
  for (const VerifyEntry& e : all.entries) got.emplace_back(e.kind, e.row, e.review, e.a_bit);
  CHECK(got == want);   // ascending by (kind, row, review): rows shifted by the group's base (not for too_big), reviews by the chunk's
  for (uint32_t keep : {0u, 1u, 4u, 10u}) {   // truncation keeps the smallest
    gk::VerifyMerge t = m;
    t.finish(keep);
    got.clear();
    for (const VerifyEntry& e : t.entries) got.emplace_back(e.kind, e.row, e.review, e.a_bit);
    CHECK(got == std::vector<Ent>(want.begin(), want.begin() + keep));
    CHECK(t.entries_total == 15 && t.diff_total() == 10);
  }
  // without the match kind; rows beyond the merge's size are dropped, not written
  gk::VerifyMerge s;
  s.begin(2, false);
  s.add(group_of(3, false, {VerifyEntry{0, 2, 1, 1}, VerifyEntry{1, 1, 1, 1}}, 0, 0), 0, 0);
  CHECK(s.diff[0] == (std::vector<uint64_t>{0, 0}) && s.diff[1] == (std::vector<uint64_t>{0, 1}) && s.diff[2].empty());
  s.begin(0, false);
  s.finish(5);
  CHECK(s.entries.empty() && s.diff_total() == 0);
  printf(failures == before ? "ok merge\n" : "FAILED merge\n");
}

int main() {
  stand_in_cases();
  merge_cases();
  return failures ? 1 : 0;
}
