// Stand-alone program (its own main; never loaded into Python; built plain and with -fsanitize=address,undefined by
// tests/test_audit_merge.py) for the two pieces of the resident-set audit that equal object keys reach and the resident set's public
// interface cannot produce (a live resident object's key is its inventory path, so no two tie):
//   * audit_merge (csrc/audit_merge.hpp): the host merge of the chunks' candidates -- order, the tie rule across chunks, overflow;
//   * the CPU stand-in of dev_audit_select (hostemu_audit.cpp, compiled into this program): mask, totals, tie rule, cap and overflow flag.
// hostemu_audit.cpp needs only device.hpp's public dev_last_viol, which this program supplies over a table type of its own.
#include <cstdio>
#include <string>
#include <vector>

#include "audit_merge.hpp"
#include "device.hpp"

namespace gk {
struct DevTable { std::vector<uint64_t> viol; };
void dev_last_viol(const DevTable* t, uint32_t, std::vector<uint64_t>* viol) { *viol = t->viol; }
}  // namespace gk

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static std::vector<uint32_t> objs_of(const std::vector<gk::AuditCand>& v) { std::vector<uint32_t> o; for (auto& c : v) o.push_back(c.obj); return o; }

static void merge_cases() {
  using gk::AuditCand;
  const std::string a = "a", b = "b", c = std::string("c\0x", 3), d = "d";
  {   // order by key bytes, cut to k; equal keys keep their input order
    std::vector<AuditCand> v{{d, 4}, {b, 2}, {a, 1}, {c, 3}};
    CHECK(gk::audit_merge(&v, 2, 66));
    CHECK((objs_of(v) == std::vector<uint32_t>{1, 2}));
  }
  {   // a candidate equal in key to the k-th is kept, whichever chunk it came from; a larger key is not
    std::vector<AuditCand> v{{a, 1}, {b, 2}, {d, 9}, {b, 7}, {c, 3}, {b, 8}};
    CHECK(gk::audit_merge(&v, 2, 66));
    CHECK((objs_of(v) == std::vector<uint32_t>{1, 2, 7, 8}));
  }
  {   // fewer than k: everything, sorted; k == 0: nothing; an empty list
    std::vector<AuditCand> v{{b, 2}, {a, 1}};
    CHECK(gk::audit_merge(&v, 5, 69) && (objs_of(v) == std::vector<uint32_t>{1, 2}));
    std::vector<AuditCand> z{{b, 2}, {a, 1}};
    CHECK(gk::audit_merge(&z, 0, 64) && z.empty());
    std::vector<AuditCand> e;
    CHECK(gk::audit_merge(&e, 3, 67) && e.empty());
  }
  {   // more ties than the stride holds: cut to the stride and reported
    std::vector<AuditCand> v;
    for (uint32_t i = 0; i < 70; i++) v.push_back({b, i});
    v.push_back({a, 100});
    CHECK(!gk::audit_merge(&v, 2, 66));
    CHECK(v.size() == 66 && v[0].obj == 100 && v[1].obj == 0 && v[65].obj == 64);
  }
  {   // a key is bytes: an embedded \0 sorts below every other byte, a prefix below its extensions
    const std::string k1("g\0v\0K\0ns\0a", 10), k2("g\0v\0K\0ns\0a0", 11), k3("g\0v\0K\0ns0\0a", 11);
    std::vector<AuditCand> v{{k3, 3}, {k2, 2}, {k1, 1}};
    CHECK(gk::audit_merge(&v, 3, 67) && (objs_of(v) == std::vector<uint32_t>{1, 2, 3}));
  }
}

static void select_cases() {
  // 200 reviews, key order = reverse slot order, the key ranks tie in runs of 5 positions (positions 5 i .. 5 i + 4 share rank i)
  const uint32_t n = 200, nt = (n + 63) / 64;
  std::vector<uint32_t> order(n), grp(n);
  for (uint32_t p = 0; p < n; p++) { order[p] = n - 1 - p; grp[p] = p / 5; }
  gk::DevTable t;
  t.viol.assign(3 * (size_t)nt, 0);
  auto set = [&](uint32_t row, uint32_t p) { const uint32_t r = order[p]; t.viol[(size_t)row * nt + r / 64] |= 1ull << (r % 64); };
  for (uint32_t p = 0; p < n; p++) set(0, p);                  // row 0: everything violates
  for (uint32_t p : {3u, 11u, 12u, 14u, 15u, 199u}) set(1, p);   // row 1: sparse
  // row 2: nothing
  std::vector<uint64_t> shown(nt, ~0ull);
  std::vector<uint32_t> pairs, idx, cnt, ovf;
  const uint32_t k = 2, cap = k + 64;
  gk::dev_audit_select(&t, 3, n, order, grp, shown, 1, k, cap, &pairs, &idx, &cnt, &ovf);
  CHECK(pairs[0] == 200 && cnt[0] == 5 && !ovf[0]);             // the 2nd lies in the run of rank 0: all five of the run
  for (uint32_t i = 0; i < 5; i++) CHECK(idx[i] == order[i]);
  CHECK(pairs[1] == 6 && cnt[1] == 4 && !ovf[1]);               // 3, 11 and the ties of 11's rank (12, 14); 15 starts the next rank
  CHECK(idx[cap + 0] == order[3] && idx[cap + 1] == order[11] && idx[cap + 2] == order[12] && idx[cap + 3] == order[14]);
  CHECK(pairs[2] == 0 && cnt[2] == 0 && !ovf[2] && idx[2 * (size_t)cap] == 0xFFFFFFFFu);
  // the mask: position 3 hidden -> the list starts at 11, the 2nd is 12, 14 ties, and the total drops by one
  shown[order[3] / 64] &= ~(1ull << (order[3] % 64));
  gk::dev_audit_select(&t, 3, n, order, grp, shown, 2, k, cap, &pairs, &idx, &cnt, &ovf);
  CHECK(pairs[0] == 199 && pairs[1] == 5 && cnt[1] == 3 && idx[cap] == order[11] && idx[cap + 2] == order[14]);
  // k == 0: totals only
  gk::dev_audit_select(&t, 3, n, order, grp, shown, 2, 0, 64, &pairs, &idx, &cnt, &ovf);
  CHECK(pairs[0] == 199 && pairs[1] == 5 && cnt[0] == 0 && cnt[1] == 0 && !ovf[0]);
  // overflow: 100 positions of ONE rank, all violating, k = 3: 67 fit, the flag says that more tie
  std::vector<uint32_t> one(n);
  for (uint32_t p = 0; p < n; p++) one[p] = p < 100 ? 0 : p;
  std::fill(shown.begin(), shown.end(), ~0ull);
  gk::dev_audit_select(&t, 3, n, order, one, shown, 3, 3, 67, &pairs, &idx, &cnt, &ovf);
  CHECK(pairs[0] == 200 && cnt[0] == 67 && ovf[0] == 1 && idx[66] == order[66]);
  CHECK(cnt[1] == 6 - 1 && !ovf[1]);                            // 3, 11, 12, 14, 15 share rank 0 with the 3rd; 199 does not
}

int main() {
  merge_cases();
  printf("%s merge\n", failures ? "FAIL" : "ok");
  const int before = failures;
  select_cases();
  printf("%s select_stand_in\n", failures > before ? "FAIL" : "ok");
  return failures ? 1 : 0;
}
