// The pure part of the device-side key join of a table's changes stream (gk_table_changes with GK_CHANGES_DEVICE_JOIN, gk_table_join):
// how one side's object keys are packed into records for the device, the hash that gives a record its home in the join's table, and how
// the reviews the device leaves to the host are settled.  Host only but for kjoin_hash / kjoin_mask / kjoin_units, which are plain C++
// the kernels (kernels.hip gk_kjoin_*) and the CPU stand-in (tests/native/hostemu_kjoin.cpp) compile as they stand; no HIP call and no
// dependency on the engine (tests/native/key_join_test.cpp runs it under sanitizers).
//
// The join's rules are delta_join's (table_delta.hpp), and its three arrays come out bit for bit: the table is keyed by the exact record
// bytes -- a hash picks a home slot and a 32-bit tag, never an answer -- and every key that occurs more than once on a side and is
// present in the snapshot is left to kjoin_resolve, the only place where the occurrence rule is applied.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string_view>
#include <vector>

#include "table_delta.hpp"

#if defined(__HIPCC__)
#define GK_KJ_HD __host__ __device__
#else
#define GK_KJ_HD
#endif

namespace gk {

// ---- records.  One side's keys in review order: a record is [u32 length][bytes], 16-byte aligned and zero-padded (the string heap's
// convention), so hashing and comparing are whole 16-byte loads; off[i] = where review i's record begins, in 16-byte units.  An empty
// key is a record of length 0.
struct alignas(16) KjUnit { uint32_t w[4]; };
struct KjPacked {
  std::vector<KjUnit> rec;
  std::vector<uint32_t> off;   // [n]
};
constexpr uint64_t KJOIN_MAX_UNITS = 0xFFFFFFFFull;   // offsets are 32 bits wide
constexpr uint32_t KJOIN_MAX_REVIEWS = 1u << 30;       // the capacity, a power of two >= 2 n, stays below 2^32

GK_KJ_HD inline uint32_t kjoin_units(uint32_t len) { return (uint32_t)(((uint64_t)len + 4u + 15u) / 16u); }

// false: the side does not fit 32-bit offsets in 16-byte units (`max_units`: a test's faked size) -- nothing is truncated, the caller
// joins on the host
template <class Key>
inline bool kjoin_pack(uint32_t n, Key&& key, KjPacked* out, uint64_t max_units = KJOIN_MAX_UNITS) {
  out->rec.clear(); out->off.clear();
  if (n > KJOIN_MAX_REVIEWS) return false;
  uint64_t units = 0;
  for (uint32_t i = 0; i < n; i++) {
    const std::string_view k = key(i);
    if (k.size() > 0xFFFFFFF0ull) return false;
    units += kjoin_units((uint32_t)k.size());
    if (units > max_units) return false;
  }
  out->rec.assign((size_t)units, KjUnit{{0u, 0u, 0u, 0u}});
  out->off.resize(n);
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; i++) {
    const std::string_view k = key(i);
    out->off[i] = (uint32_t)at;
    unsigned char* p = reinterpret_cast<unsigned char*>(out->rec.data() + at);
    const uint32_t len = (uint32_t)k.size();
    std::memcpy(p, &len, 4);
    if (len) std::memcpy(p + 4, k.data(), len);
    at += kjoin_units(len);
  }
  return true;
}
// the key of a record, as bytes
inline std::string_view kjoin_key(const KjUnit* rec) {
  return std::string_view(reinterpret_cast<const char*>(rec) + 4, rec->w[0]);
}

// ---- hash.  64 bits over the record's units (length word and padding included: equal records, equal hashes).  The low bits choose the
// home slot, the high half is the slot's tag.  A quality matter only: the join compares bytes wherever tags agree.
GK_KJ_HD inline uint64_t kjoin_hash(const KjUnit* rec, uint32_t units) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)units * 0xD6E8FEB86659FD93ull);
  for (uint32_t u = 0; u < units; u++) {
    const uint64_t a = (uint64_t)rec[u].w[0] | ((uint64_t)rec[u].w[1] << 32), b = (uint64_t)rec[u].w[2] | ((uint64_t)rec[u].w[3] << 32);
    h = (h ^ a) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
    h = (h ^ b) * 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 29;
  }
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33;
  return h;
}
// test aid (gk_debug_set "kjoin_hash_bits"): the low `bits` bits of a hash; 64 and above: all of it, 0: every key one home and one tag
GK_KJ_HD inline uint64_t kjoin_mask(uint64_t h, uint32_t bits) { return bits >= 64u ? h : bits == 0u ? 0ull : h & ((1ull << bits) - 1ull); }
GK_KJ_HD inline bool kjoin_same(const KjUnit* a, const KjUnit* b, uint32_t units) {
  for (uint32_t u = 0; u < units; u++)
    if (a[u].w[0] != b[u].w[0] || a[u].w[1] != b[u].w[1] || a[u].w[2] != b[u].w[2] || a[u].w[3] != b[u].w[3]) return false;
  return true;
}
// the table's capacity: the power of two >= 2 n_then (at least 1), so an empty slot always exists
inline uint32_t kjoin_capacity(uint32_t n_then) {
  uint64_t c = 1;
  while (c < 2ull * n_then) c <<= 1;
  return (uint32_t)c;
}
constexpr uint64_t KJOIN_EMPTY = ~0ull;   // a slot: hash high half << 32 | review; all ones: empty

struct KjoinStats {
  uint32_t n_now = 0, n_then = 0, capacity = 0;
  uint32_t host_resolved_now = 0, host_resolved_then = 0;   // the reviews kjoin_resolve settled
  uint32_t device = 0;      // 1: the device join ran, 0: the host join (delta_join over the two key orders)
  uint32_t fallback = 0;    // why not the device, when it was asked for: 0 none, 1 a side's keys do not fit, 2 the kernels' error word
  float pack_ms = 0;        // host time to pack and upload the now side's keys, when this call did (diagnostic)
};
// the kernels gave up (a probe loop ran out, an offset outside the records): the caller joins on the host and says so
struct KjoinFault : std::runtime_error { using std::runtime_error::runtime_error; };

// ---- the reviews the device leaves to the host.  flagged_now / flagged_then = bit words over the two sides: every review whose key
// occurs more than once on some side and is present in the snapshot (closed under key equality).  Each subset is sorted by (key,
// review), delta_join runs over the two subsets alone, and then_of / now_of / unmatched take its answer for exactly those reviews.
template <class KeyNow, class KeyThen>
inline void kjoin_resolve(const std::vector<uint64_t>& flagged_now, const std::vector<uint64_t>& flagged_then, uint32_t n_now, uint32_t n_then, KeyNow&& key_now,
                          KeyThen&& key_then, std::vector<uint32_t>* then_of, std::vector<uint32_t>* now_of, std::vector<uint64_t>* unmatched,
                          std::vector<uint32_t>* resolved_now = nullptr, std::vector<uint32_t>* resolved_then = nullptr) {
  std::vector<uint32_t> sub_now, sub_then;
  for (size_t w = 0; w < flagged_now.size(); w++)
    for (uint64_t m = flagged_now[w]; m; m &= m - 1ull) {
      const uint64_t r = w * 64u + (uint64_t)__builtin_ctzll(m);
      if (r < n_now) sub_now.push_back((uint32_t)r);
    }
  for (size_t w = 0; w < flagged_then.size(); w++)
    for (uint64_t m = flagged_then[w]; m; m &= m - 1ull) {
      const uint64_t p = w * 64u + (uint64_t)__builtin_ctzll(m);
      if (p < n_then) sub_then.push_back((uint32_t)p);
    }
  if (then_of->size() != n_now || now_of->size() != n_then || unmatched->size() != ((size_t)n_then + 63u) / 64u) throw std::runtime_error("kjoin_resolve: the arrays do not fit the sides");
  // (the subsets come out ascending by review, so a stable sort by key is the sort by (key, review))
  std::stable_sort(sub_now.begin(), sub_now.end(), [&](uint32_t a, uint32_t b) { return key_now(a) < key_now(b); });
  std::stable_sort(sub_then.begin(), sub_then.end(), [&](uint32_t a, uint32_t b) { return key_then(a) < key_then(b); });
  std::vector<uint32_t> ord_now(sub_now.size()), ord_then(sub_then.size()), t_of, n_of;
  for (uint32_t i = 0; i < ord_now.size(); i++) ord_now[i] = i;
  for (uint32_t i = 0; i < ord_then.size(); i++) ord_then[i] = i;
  std::vector<uint64_t> gone;
  delta_join(ord_now, [&](uint32_t i) { return key_now(sub_now[i]); }, ord_then, [&](uint32_t i) { return key_then(sub_then[i]); }, &t_of, &n_of, &gone);
  for (size_t i = 0; i < sub_now.size(); i++) (*then_of)[sub_now[i]] = t_of[i] == DELTA_NONE ? DELTA_NONE : sub_then[t_of[i]];
  for (size_t j = 0; j < sub_then.size(); j++) {
    const uint32_t p = sub_then[j];
    (*now_of)[p] = n_of[j] == DELTA_NONE ? DELTA_NONE : sub_now[n_of[j]];
    const uint64_t bit = 1ull << (p % 64u);
    if (n_of[j] == DELTA_NONE) (*unmatched)[p / 64u] |= bit; else (*unmatched)[p / 64u] &= ~bit;
  }
  if (resolved_now) *resolved_now = std::move(sub_now);
  if (resolved_then) *resolved_then = std::move(sub_then);
}

}  // namespace gk
