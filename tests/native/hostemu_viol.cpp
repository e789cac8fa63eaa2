// TEST-ONLY CPU stand-in of dev_viol_index / dev_viol_entries (device.hpp; the device versions are gk_viol_any + gk_viol_emit in
// kernels.hip), linked into libgkgpu_hostemu.so beside hostemu.cpp.  Plain loops over the bitmap of the table's most recent
// evaluation, which it gets through the public dev_last_viol: nothing of the emulation's internals, and no state between calls.
#include <stdexcept>
#include <string>

#include "device.hpp"

namespace gk {

// the bitmap and its words per row; throws what the device entries throw
static uint32_t viol_rows(const char* who, const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, std::vector<uint64_t>* viol) {
  const uint32_t pw = (n_reviews + 63u) / 64u;
  dev_last_viol(t, nc, viol);
  if (nc == 0 || viol->empty() || viol->size() % nc) throw std::runtime_error(std::string(who) + ": evaluate the table first");
  const uint32_t nt = (uint32_t)(viol->size() / nc);
  if (nt < pw || shown.size() < pw) throw std::runtime_error(std::string(who) + ": shown / the review count do not fit the table");
  return nt;
}

static uint64_t any_word(const std::vector<uint64_t>& viol, uint32_t nc, uint32_t nt, const std::vector<uint64_t>& shown, uint32_t n_reviews, uint32_t w) {
  uint64_t acc = 0;
  for (uint32_t r = 0; r < nc; r++) acc |= viol[(size_t)r * nt + w];
  acc &= shown[w];
  const uint32_t valid = n_reviews - w * 64u;
  return valid < 64u ? acc & ((1ull << valid) - 1ull) : acc;
}

void dev_viol_index(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, uint64_t /*shown_gen*/,
                    std::vector<uint32_t>* cnt, std::vector<uint64_t>* any) {
  cnt->clear();
  if (any) any->clear();
  std::vector<uint64_t> viol;
  const uint32_t nt = viol_rows("dev_viol_index", t, nc, n_reviews, shown, &viol), pw = (n_reviews + 63u) / 64u;
  for (uint32_t w = 0; w < pw; w++) {
    const uint64_t a = any_word(viol, nc, nt, shown, n_reviews, w);
    cnt->push_back((uint32_t)__builtin_popcountll(a));
    if (any) any->push_back(a);
  }
}

void dev_viol_entries(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, uint64_t /*shown_gen*/, uint32_t w0, uint32_t w1,
                      std::vector<uint32_t>* reviews, std::vector<uint64_t>* masks) {
  reviews->clear(); masks->clear();
  std::vector<uint64_t> viol;
  const uint32_t nt = viol_rows("dev_viol_entries", t, nc, n_reviews, shown, &viol), pw = (n_reviews + 63u) / 64u, mw = (nc + 63u) / 64u;
  if (w0 > w1 || w1 > pw) throw std::runtime_error("dev_viol_entries: the word range does not fit the table");
  for (uint32_t w = w0; w < w1; w++) {
    const uint64_t a = any_word(viol, nc, nt, shown, n_reviews, w);
    for (uint32_t l = 0; l < 64u; l++) {
      if (!((a >> l) & 1ull)) continue;
      reviews->push_back(w * 64u + l);
      const size_t at = masks->size();
      masks->resize(at + mw, 0);
      for (uint32_t r = 0; r < nc; r++)
        if ((viol[(size_t)r * nt + w] >> l) & 1ull) (*masks)[at + r / 64u] |= 1ull << (r % 64u);
    }
  }
}

}  // namespace gk
