// Stand-alone test of the pure part of the device key join (csrc/key_join.hpp) and of the CPU stand-in's dev_kjoin
// (tests/native/hostemu_kjoin.cpp) against delta_join over the same sides.  Own main; built plain and under sanitizers by
// tests/test_key_join_native.py; never loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>

#include "device.hpp"

using namespace gk;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

typedef std::vector<std::string> Keys;

static std::vector<uint32_t> key_order(const Keys& keys) {
  std::vector<uint32_t> o(keys.size());
  for (uint32_t i = 0; i < o.size(); i++) o[i] = i;
  std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  return o;
}
struct Joined {
  std::vector<uint32_t> then_of, now_of;
  std::vector<uint64_t> unmatched;
  bool operator==(const Joined& o) const { return then_of == o.then_of && now_of == o.now_of && unmatched == o.unmatched; }
};
static Joined full_join(const Keys& now, const Keys& then) {
  Joined j;
  delta_join(key_order(now), [&](uint32_t i) { return std::string_view(now[i]); }, key_order(then), [&](uint32_t i) { return std::string_view(then[i]); }, &j.then_of, &j.now_of,
             &j.unmatched);
  return j;
}
static KjPacked pack(const Keys& keys) {
  KjPacked pk;
  CHECK(kjoin_pack((uint32_t)keys.size(), [&](uint32_t i) { return std::string_view(keys[i]); }, &pk));
  return pk;
}

static void test_pack() {
  // record boundaries: 4 + length bytes rounded up to 16 -- 11 and 12 end in the first unit, 13 needs a second, 27 / 28 / 29 likewise
  const uint32_t lens[] = {0, 11, 12, 13, 27, 28, 29};
  const uint32_t units[] = {1, 1, 1, 2, 2, 2, 3};
  Keys keys;
  for (uint32_t l : lens) {
    std::string k(l, '\0');
    for (uint32_t i = 0; i < l; i++) k[i] = (char)(0x80 + l + i);   // (no zero byte: padding shows)
    keys.push_back(k);
  }
  const KjPacked pk = pack(keys);
  CHECK(pk.off.size() == 7 && pk.rec.size() == 12);
  uint32_t at = 0;
  for (size_t i = 0; i < keys.size(); i++) {
    CHECK(kjoin_units(lens[i]) == units[i] && pk.off[i] == at);
    const unsigned char* p = reinterpret_cast<const unsigned char*>(pk.rec.data() + at);
    CHECK(pk.rec[at].w[0] == lens[i] && kjoin_key(pk.rec.data() + at) == keys[i]);
    for (uint32_t b = 4 + lens[i]; b < units[i] * 16u; b++) CHECK(p[b] == 0);   // zero padding
    at += units[i];
  }
  CHECK(reinterpret_cast<uintptr_t>(pk.rec.data()) % 16u == 0);
  // an empty side
  KjPacked none;
  CHECK(kjoin_pack(0, [&](uint32_t) { return std::string_view(); }, &none) && none.rec.empty() && none.off.empty());
  // the offsets do not fit (a faked size): refused, nothing truncated; exactly the size fits
  KjPacked small;
  CHECK(!kjoin_pack(7, [&](uint32_t i) { return std::string_view(keys[i]); }, &small, 11) && small.rec.empty() && small.off.empty());
  CHECK(kjoin_pack(7, [&](uint32_t i) { return std::string_view(keys[i]); }, &small, 12) && small.off == pk.off);
  std::printf("ok pack\n");
}

static void test_hash() {
  const Keys keys = {"a", "b", "ab", std::string("a\0", 2), "aaaaaaaaaaaa", "aaaaaaaaaaaaa", "aaaaaaaaaaab", std::string(40, 'x'), std::string(40, 'x') + "y"};
  const KjPacked pk = pack(keys);
  std::set<uint64_t> full, low3;
  for (size_t i = 0; i < keys.size(); i++) {
    const KjUnit* rec = pk.rec.data() + pk.off[i];
    const uint64_t h = kjoin_hash(rec, kjoin_units(rec->w[0]));
    full.insert(kjoin_mask(h, 64));
    low3.insert(kjoin_mask(h, 3));
    CHECK(kjoin_mask(h, 64) == h && kjoin_mask(h, 100) == h && kjoin_mask(h, 3) == (h & 7u) && kjoin_mask(h, 0) == 0 && kjoin_mask(h, 63) == (h & ~(1ull << 63)));
    // equal records, equal hashes: a second packing of the same key elsewhere
    const KjPacked again = pack({"pad-pad-pad-pad-pad", keys[i]});
    const KjUnit* r2 = again.rec.data() + again.off[1];
    CHECK(kjoin_hash(r2, kjoin_units(r2->w[0])) == h && kjoin_same(rec, r2, kjoin_units(rec->w[0])));
  }
  CHECK(full.size() == keys.size() && low3.size() <= 8);
  CHECK(kjoin_capacity(0) == 1 && kjoin_capacity(1) == 2 && kjoin_capacity(2) == 4 && kjoin_capacity(3) == 8 && kjoin_capacity(64) == 128 && kjoin_capacity(65) == 256);
  std::printf("ok hash\n");
}

// the flagged sets the kernels' rules give: every review whose key occurs more than once on some side and is present then
static void flag_sets(const Keys& now, const Keys& then, std::vector<uint64_t>* fn, std::vector<uint64_t>* ft) {
  fn->assign((now.size() + 63) / 64, 0); ft->assign((then.size() + 63) / 64, 0);
  auto count = [](const Keys& ks, const std::string& k) { size_t c = 0; for (const auto& x : ks) c += x == k; return c; };
  for (size_t r = 0; r < now.size(); r++)
    if (!now[r].empty() && count(then, now[r]) && (count(then, now[r]) > 1 || count(now, now[r]) > 1)) (*fn)[r / 64] |= 1ull << (r % 64);
  for (size_t p = 0; p < then.size(); p++)
    if (!then[p].empty() && (count(then, then[p]) > 1 || count(now, then[p]) > 1)) (*ft)[p / 64] |= 1ull << (p % 64);
}

static void test_resolve() {
  // duplicates 2 then : 1 now, 1 : 2, 3 : 2 and 2 : 3 among unique keys; empty keys on both sides
  const Keys then = {"u1", "a", "", "c", "a", "b", "c", "d", "c", "d", "u2", "gone"};
  const Keys now = {"d", "", "a", "u2", "b", "d", "b", "c", "new", "c", "d", "u1", "n2", "n2"};
  const Joined want = full_join(now, then);
  std::vector<uint64_t> fn, ft;
  flag_sets(now, then, &fn, &ft);
  // what the device leaves for the unflagged reviews: unique keys paired, everything else none; unmatched of the unflagged only
  Joined got;
  got.then_of.assign(now.size(), DELTA_NONE); got.now_of.assign(then.size(), DELTA_NONE); got.unmatched.assign(1, 0);
  for (uint32_t r = 0; r < now.size(); r++)
    for (uint32_t p = 0; p < then.size(); p++)
      if (!now[r].empty() && now[r] == then[p] && !((fn[0] >> r) & 1)) { got.then_of[r] = p; got.now_of[p] = r; }
  for (uint32_t p = 0; p < then.size(); p++) if (got.now_of[p] == DELTA_NONE && !((ft[0] >> p) & 1)) got.unmatched[0] |= 1ull << p;
  std::vector<uint32_t> rn, rt;
  kjoin_resolve(fn, ft, (uint32_t)now.size(), (uint32_t)then.size(), [&](uint32_t i) { return std::string_view(now[i]); }, [&](uint32_t i) { return std::string_view(then[i]); },
                &got.then_of, &got.now_of, &got.unmatched, &rn, &rt);
  CHECK(got == want);
  CHECK(rn.size() == 8 && rt.size() == 8);   // now: a, b b, c c, d d d; then: a a, b, c c c, d d
  // an empty key among the flagged matches nothing, and flag bits beyond the sides are ignored
  const Keys t2 = {"", "k", "k"}, n2 = {"k", ""};
  Joined g2;
  g2.then_of.assign(2, DELTA_NONE); g2.now_of.assign(3, DELTA_NONE); g2.unmatched.assign(1, 0);
  kjoin_resolve({~0ull}, {~0ull}, 2, 3, [&](uint32_t i) { return std::string_view(n2[i]); }, [&](uint32_t i) { return std::string_view(t2[i]); }, &g2.then_of, &g2.now_of,
                &g2.unmatched);
  CHECK(g2 == full_join(n2, t2));
  // nothing flagged: nothing touched
  Joined g3 = want;
  kjoin_resolve({0}, {0}, (uint32_t)now.size(), (uint32_t)then.size(), [&](uint32_t i) { return std::string_view(now[i]); }, [&](uint32_t i) { return std::string_view(then[i]); },
                &g3.then_of, &g3.now_of, &g3.unmatched);
  CHECK(g3 == want);
  std::printf("ok resolve\n");
}

static Joined stand_in(const Keys& now, const Keys& then, uint32_t bits, KjoinStats* st, std::vector<uint64_t>* fn, std::vector<uint64_t>* ft) {
  const KjPacked pn = pack(now), pt = pack(then);
  DevKeys *dn = dev_keys_put(0, pn.rec.data(), pn.rec.size(), pn.off.data(), (uint32_t)now.size()), *dt = dev_keys_put(0, pt.rec.data(), pt.rec.size(), pt.off.data(), (uint32_t)then.size());
  CHECK(dev_keys_bytes(dn) == pn.rec.size() * 16u + now.size() * 4u);
  Joined j;
  float ms = -1;
  DevJoin* keep = nullptr;
  const auto key_at = [](const void* c, uint32_t i) { return std::string_view((*static_cast<const Keys*>(c))[i]); };
  dev_kjoin(dn, dt, bits, KjKeyFn{key_at, &now}, KjKeyFn{key_at, &then}, &j.then_of, &j.now_of, &j.unmatched, fn, ft, st, &ms, &keep);
  CHECK(ms == 0 && keep);
  dev_join_free(keep);
  dev_keys_free(dn); dev_keys_free(dt);
  return j;
}

static void test_stand_in() {
  std::mt19937 rng(20240521);
  const uint32_t sizes[] = {0, 1, 63, 64, 65, 257};
  for (uint32_t nn : sizes)
    for (uint32_t nt : sizes)
      for (uint32_t bits : {64u, 3u, 0u})
        for (int dups = 0; dups < 2; dups++) {
          // keys from a pool a little larger than the sides (unique draws), or a small one (many duplicates); some empty
          const uint32_t pool = dups ? 40u : 600u;
          auto draw = [&](uint32_t n) {
            Keys ks;
            std::set<uint32_t> used;
            while (ks.size() < n) {
              const uint32_t v = rng() % pool;
              if (!dups && !used.insert(v).second) continue;
              ks.push_back(dups && v % 17 == 0 ? std::string() : std::string("g\0v1\0Kind\0ns", 12) + std::to_string(v % 7) + std::string(1, '\0') + "name-" + std::to_string(v) + std::string(v % 23, 'x'));
            }
            return ks;
          };
          const Keys now = draw(nn), then = draw(nt);
          KjoinStats st;
          std::vector<uint64_t> fn, ft, want_fn, want_ft;
          const Joined got = stand_in(now, then, bits, &st, &fn, &ft);
          CHECK(got == full_join(now, then));
          flag_sets(now, then, &want_fn, &want_ft);
          CHECK(fn == want_fn && ft == want_ft);   // the flagged sets are what the contract says, whatever the hashes collide on
          size_t cn = 0, ct = 0;
          for (uint64_t w : fn) cn += (size_t)__builtin_popcountll(w);
          for (uint64_t w : ft) ct += (size_t)__builtin_popcountll(w);
          CHECK(st.n_now == nn && st.n_then == nt && st.device == 1 && st.fallback == 0 && st.host_resolved_now == cn && st.host_resolved_then == ct);
          CHECK(st.capacity >= 2 * nt && st.capacity >= 1 && (st.capacity & (st.capacity - 1)) == 0 && (nt == 0 || st.capacity < 4 * nt));
          if (!dups) CHECK(cn == 0 && ct == 0);
        }
  std::printf("ok stand_in\n");
}

int main() {
  test_pack();
  test_hash();
  test_resolve();
  test_stand_in();
  return 0;
}
