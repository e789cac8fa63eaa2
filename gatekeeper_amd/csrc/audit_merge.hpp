// Host merge of one constraint's audit candidates over the chunks of the resident set (gk_resident_audit).  Every chunk hands in
// its k smallest shown violators by object key plus the key ties of its k-th (dev_audit_select); the k smallest of the whole set,
// and every tie of THEIR k-th, are among those: a chunk's k-th key is never below the set's.  At most 17 x (k + 64) entries per
// constraint, so a plain sort.  Host only; no dependency on the engine (tests/native/audit_merge_test.cpp runs it under sanitizers).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string_view>
#include <vector>

namespace gk {

struct AuditCand {
  std::string_view key;   // the object key's bytes (group \0 version \0 kind \0 namespace \0 name): LimitQueue's leading fields
  uint32_t obj;           // what the caller wants back (the resident object's id)
};

// Sorts `cands` by key bytes (equal keys keep their input order) and keeps the k smallest plus every further one whose key equals
// the k-th.  false: more are left than `stride` holds -- the list is cut to `stride` and the caller flags the row as overflowed.
inline bool audit_merge(std::vector<AuditCand>* cands, uint32_t k, uint32_t stride) {
  std::vector<AuditCand>& v = *cands;
  std::stable_sort(v.begin(), v.end(), [](const AuditCand& a, const AuditCand& b) { return a.key < b.key; });
  size_t keep = k == 0 ? 0 : std::min<size_t>(v.size(), k);
  if (k != 0 && keep == k) while (keep < v.size() && v[keep].key == v[k - 1].key) keep++;
  v.resize(keep, AuditCand{});
  if (keep <= stride) return true;
  v.resize(stride, AuditCand{});
  return false;
}

}  // namespace gk
