// TEST-ONLY CPU stand-in of dev_keys_put / dev_kjoin and the dev_tchg_align overload that takes a finished join (device.hpp; the device
// versions are gk_kjoin_build + gk_kjoin_probe + gk_kjoin_finish in kernels.hip), linked into libgkgpu_hostemu.so beside hostemu.cpp.
// Public device.hpp entries only.  The same contract in one thread: the same records, the same hash and homes (key_join.hpp), the same
// open-addressing table walked review by review, the same flagged sets and stats -- so the engine's use of the flagged sets and
// kjoin_resolve are exercised here exactly as on the device (tests/native/key_join_test.cpp checks it against delta_join).
#include <memory>
#include <stdexcept>

#include "device.hpp"

namespace gk {

struct DevKeys { std::vector<KjUnit> rec; std::vector<uint32_t> off; };
struct DevJoin { std::vector<uint32_t> then_of; uint32_t n_then = 0; };

namespace {
// the record of review i; throws what the device reports through its error word
const KjUnit* record_of(const DevKeys& k, uint32_t i, uint32_t* units) {
  const size_t o = k.off[i];
  if (o >= k.rec.size() || kjoin_units(k.rec[o].w[0]) > k.rec.size() - o) throw KjoinFault("dev_kjoin: a record lies outside the arena");
  *units = kjoin_units(k.rec[o].w[0]);
  return k.rec.data() + o;
}
}  // namespace

DevKeys* dev_keys_put(int, const KjUnit* rec, size_t units, const uint32_t* off, uint32_t n) {
  if (units > KJOIN_MAX_UNITS || n > KJOIN_MAX_REVIEWS) throw std::runtime_error("dev_keys_put: the keys do not fit 32-bit offsets");
  for (uint32_t i = 0; i < n; i++)
    if (off[i] >= units || kjoin_units(rec[off[i]].w[0]) > units - off[i]) throw std::runtime_error("dev_keys_put: a record lies outside the arena");
  std::unique_ptr<DevKeys> k(new DevKeys());
  k->rec.assign(rec, rec + units);
  k->off.assign(off, off + n);
  return k.release();
}
void dev_keys_free(DevKeys* k) { delete k; }
uint64_t dev_keys_bytes(const DevKeys* k) { return k ? (uint64_t)k->rec.size() * sizeof(KjUnit) + (uint64_t)k->off.size() * 4u : 0u; }
void dev_join_free(DevJoin* j) { delete j; }

void dev_kjoin(const DevKeys* now, const DevKeys* then, uint32_t hash_bits, const KjKeyFn& key_now, const KjKeyFn& key_then, std::vector<uint32_t>* then_of,
               std::vector<uint32_t>* now_of, std::vector<uint64_t>* unmatched, std::vector<uint64_t>* flagged_now, std::vector<uint64_t>* flagged_then, KjoinStats* stats,
               float* ms, DevJoin** keep) {
  *ms = 0;
  if (keep) *keep = nullptr;
  if (!now || !then) throw std::runtime_error("dev_kjoin: two sides' keys on one device");
  const uint32_t n_now = (uint32_t)now->off.size(), n_then = (uint32_t)then->off.size(), cap = kjoin_capacity(n_then);
  *stats = KjoinStats();
  stats->n_now = n_now; stats->n_then = n_then; stats->capacity = cap; stats->device = 1;
  then_of->assign(n_now, DELTA_NONE); now_of->assign(n_then, DELTA_NONE);
  unmatched->assign((n_then + 63u) / 64u, 0); flagged_now->assign((n_now + 63u) / 64u, 0); flagged_then->assign((n_then + 63u) / 64u, 0);
  std::vector<uint64_t> slots(cap, KJOIN_EMPTY);
  std::vector<uint8_t> dup(n_then, 0);
  std::vector<uint32_t> hits(n_then, 0), cand(n_now, DELTA_NONE);
  // the slot that holds the bytes of `rec`, or the first empty one from its home on; *found says which
  auto walk = [&](const KjUnit* rec, uint32_t units, bool* found) -> uint32_t {
    const uint64_t h = kjoin_mask(kjoin_hash(rec, units), hash_bits);
    uint32_t slot = (uint32_t)h & (cap - 1u);
    for (uint32_t step = 0; step < cap; step++, slot = (slot + 1u) & (cap - 1u)) {
      if (slots[slot] == KJOIN_EMPTY) { *found = false; return slot; }
      if ((uint32_t)(slots[slot] >> 32) != (uint32_t)(h >> 32)) continue;
      uint32_t ou = 0;
      const KjUnit* orec = record_of(*then, (uint32_t)slots[slot], &ou);
      if (ou == units && kjoin_same(rec, orec, units)) { *found = true; return slot; }
    }
    throw KjoinFault("dev_kjoin: a probe loop ran out of slots");
  };
  for (uint32_t p = 0; p < n_then; p++) {   // build
    uint32_t units = 0;
    const KjUnit* rec = record_of(*then, p, &units);
    if (rec->w[0] == 0u) continue;
    bool found = false;
    const uint32_t slot = walk(rec, units, &found);
    if (found) { dup[p] = 1; dup[(uint32_t)slots[slot]] = 1; }
    else slots[slot] = (kjoin_mask(kjoin_hash(rec, units), hash_bits) >> 32 << 32) | p;
  }
  for (uint32_t r = 0; r < n_now; r++) {   // probe
    uint32_t units = 0;
    const KjUnit* rec = record_of(*now, r, &units);
    if (rec->w[0] == 0u) continue;
    bool found = false;
    const uint32_t slot = walk(rec, units, &found);
    if (found) { cand[r] = (uint32_t)slots[slot]; hits[cand[r]]++; }
  }
  for (uint32_t r = 0; r < n_now; r++) {   // finish
    const uint32_t c = cand[r];
    if (c == DELTA_NONE) continue;
    if (hits[c] == 1u && !dup[c]) { (*then_of)[r] = c; (*now_of)[c] = r; }
    else (*flagged_now)[r / 64u] |= 1ull << (r % 64u);
  }
  for (uint32_t p = 0; p < n_then; p++) {
    if (dup[p] || hits[p] > 1u) (*flagged_then)[p / 64u] |= 1ull << (p % 64u);
    else if (hits[p] == 0u) (*unmatched)[p / 64u] |= 1ull << (p % 64u);
  }
  std::vector<uint32_t> res_now, res_then;
  kjoin_resolve(*flagged_now, *flagged_then, n_now, n_then, key_now, key_then, then_of, now_of, unmatched, &res_now, &res_then);
  stats->host_resolved_now = (uint32_t)res_now.size(); stats->host_resolved_then = (uint32_t)res_then.size();
  if (keep) {
    std::unique_ptr<DevJoin> j(new DevJoin());
    j->then_of = *then_of; j->n_then = n_then;
    *keep = j.release();
  }
}

DevAligned* dev_tchg_align(int device, const DevSnap* s, uint32_t n, const DevJoin& then_of, const std::vector<uint32_t>& row_of, const std::vector<uint64_t>* moved,
                           const std::vector<uint64_t>* only, float* ms) {
  if (then_of.then_of.size() != n) throw std::runtime_error("dev_tchg_align: the join does not fit the table");
  return dev_tchg_align(device, s, n, &then_of.then_of, row_of, moved, only, ms);
}

}  // namespace gk
