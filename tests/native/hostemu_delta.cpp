// TEST-ONLY CPU stand-in of dev_delta_keep / dev_delta_index / dev_delta_entries / dev_delta_drop (device.hpp; the device versions are
// gk_delta_index + gk_delta_emit in kernels.hip), linked into libgkgpu_hostemu.so beside hostemu.cpp.  Public device.hpp entries only,
// nothing of the emulation's internals: the bitmap of the table's most recent evaluation comes through dev_last_viol, dev_delta_keep
// keeps a copy of it and of the mask beside the table's address (until dev_delta_drop), and the two entries are word-by-word loops
// over plain arrays (delta_index_words / delta_entries_words: tests/native/delta_stream_test.cpp checks them bit by bit).
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

#include "device.hpp"

namespace gk {

// one table on plain arrays: now / base = [nc][nt] words (base may be null: reads as zero), shown_now / shown_base = [pw] words
struct DeltaWords { const uint64_t *now, *base, *shown_now, *shown_base; uint32_t nc, nt; };

static uint64_t delta_changed_word(const DeltaWords& d, uint32_t n_reviews, uint32_t w) {
  uint64_t acc = 0;
  for (uint32_t r = 0; r < d.nc; r++) {
    const uint64_t x = d.now[(size_t)r * d.nt + w] & d.shown_now[w];
    const uint64_t y = d.base ? d.base[(size_t)r * d.nt + w] & d.shown_base[w] : 0ull;
    acc |= x ^ y;
  }
  const uint32_t valid = n_reviews - w * 64u;
  return valid < 64u ? acc & ((1ull << valid) - 1ull) : acc;
}

void delta_index_words(const DeltaWords& d, uint32_t n_reviews, std::vector<uint32_t>* cnt, std::vector<uint64_t>* changed) {
  const uint32_t pw = (n_reviews + 63u) / 64u;
  cnt->assign(pw, 0); changed->assign(pw, 0);
  for (uint32_t w = 0; w < pw; w++) {
    (*changed)[w] = delta_changed_word(d, n_reviews, w);
    (*cnt)[w] = (uint32_t)__builtin_popcountll((*changed)[w]);
  }
}

// extra: null or [w1 - w0] words of reviews that get an entry whatever the bitmaps say (bits at or beyond n_reviews are dropped)
void delta_entries_words(const DeltaWords& d, uint32_t n_reviews, uint32_t w0, uint32_t w1, const uint64_t* extra, std::vector<uint32_t>* reviews,
                         std::vector<uint64_t>* now, std::vector<uint64_t>* was) {
  reviews->clear(); now->clear(); was->clear();
  const uint32_t mw = (d.nc + 63u) / 64u;
  for (uint32_t w = w0; w < w1; w++) {
    uint64_t ch = delta_changed_word(d, n_reviews, w);
    if (extra) {
      const uint32_t valid = n_reviews - w * 64u;
      ch |= valid < 64u ? extra[w - w0] & ((1ull << valid) - 1ull) : extra[w - w0];
    }
    for (uint64_t m = ch; m; m &= m - 1ull) {
      const uint32_t l = (uint32_t)__builtin_ctzll(m);
      reviews->push_back(w * 64u + l);
      const size_t at = now->size();
      now->resize(at + mw, 0); was->resize(at + mw, 0);
      const bool sn = (d.shown_now[w] >> l) & 1ull, sb = d.base && ((d.shown_base[w] >> l) & 1ull);
      for (uint32_t r = 0; r < d.nc; r++) {
        if (sn && ((d.now[(size_t)r * d.nt + w] >> l) & 1ull)) (*now)[at + r / 64u] |= 1ull << (r % 64u);
        if (sb && ((d.base[(size_t)r * d.nt + w] >> l) & 1ull)) (*was)[at + r / 64u] |= 1ull << (r % 64u);
      }
    }
  }
}

namespace {
struct Kept { std::vector<uint64_t> base, shown; uint32_t nc = 0, nt = 0, pw = 0; };
std::mutex& kept_mu() { static std::mutex m; return m; }
std::map<const DevTable*, Kept>& kept() { static std::map<const DevTable*, Kept> m; return m; }

// the bitmap and its words per row; throws what the device entries throw
uint32_t delta_rows(const char* who, const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, std::vector<uint64_t>* viol) {
  const uint32_t pw = (n_reviews + 63u) / 64u;
  dev_last_viol(t, nc, viol);
  if (nc == 0 || viol->empty() || viol->size() % nc) throw std::runtime_error(std::string(who) + ": evaluate the table first");
  const uint32_t nt = (uint32_t)(viol->size() / nc);
  if (nt < pw || shown.size() < pw) throw std::runtime_error(std::string(who) + ": shown / the review count do not fit the table");
  return nt;
}
// the kept baseline (kept_mu held): null without use_base or when there is none
const Kept* base_of(const char* who, const DevTable* t, uint32_t nc, uint32_t nt, uint32_t pw, bool use_base) {
  if (!use_base) return nullptr;
  auto it = kept().find(t);
  if (it == kept().end()) return nullptr;
  if (it->second.nc != nc || it->second.nt != nt || it->second.pw != pw) throw std::runtime_error(std::string(who) + ": the baseline belongs to other bitmaps (dev_delta_keep)");
  return &it->second;
}
}  // namespace

void dev_delta_keep(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, uint64_t /*shown_gen*/) {
  Kept k;
  k.nc = nc; k.pw = (n_reviews + 63u) / 64u;
  k.nt = delta_rows("dev_delta_keep", t, nc, n_reviews, shown, &k.base);
  k.shown.assign(shown.begin(), shown.begin() + k.pw);
  std::lock_guard<std::mutex> l(kept_mu());
  kept()[t] = std::move(k);
}

bool dev_delta_has(const DevTable* t, uint32_t nc) {
  std::lock_guard<std::mutex> l(kept_mu());
  auto it = kept().find(t);
  return it != kept().end() && it->second.nc == nc;
}

uint64_t dev_delta_bytes(const DevTable* t) {
  std::lock_guard<std::mutex> l(kept_mu());
  auto it = kept().find(t);
  return it == kept().end() ? 0u : (uint64_t)(it->second.base.size() + it->second.shown.size()) * 8u;
}

void dev_delta_drop(const DevTable* t) {
  std::lock_guard<std::mutex> l(kept_mu());
  kept().erase(t);
}

void dev_delta_index(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, uint64_t /*shown_gen*/, bool use_base,
                     std::vector<uint32_t>* cnt, std::vector<uint64_t>* changed, float* ms) {
  cnt->clear(); changed->clear();
  *ms = 0;
  std::vector<uint64_t> viol;
  const uint32_t nt = delta_rows("dev_delta_index", t, nc, n_reviews, shown, &viol), pw = (n_reviews + 63u) / 64u;
  std::lock_guard<std::mutex> l(kept_mu());
  const Kept* k = base_of("dev_delta_index", t, nc, nt, pw, use_base);
  delta_index_words(DeltaWords{viol.data(), k ? k->base.data() : nullptr, shown.data(), k ? k->shown.data() : nullptr, nc, nt}, n_reviews, cnt, changed);
}

void dev_delta_entries(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, uint64_t /*shown_gen*/, bool use_base, uint32_t w0,
                       uint32_t w1, const std::vector<uint32_t>& off, const std::vector<uint64_t>* extra, std::vector<uint32_t>* reviews,
                       std::vector<uint64_t>* now, std::vector<uint64_t>* was, float* ms) {
  reviews->clear(); now->clear(); was->clear();
  *ms = 0;
  std::vector<uint64_t> viol;
  const uint32_t nt = delta_rows("dev_delta_entries", t, nc, n_reviews, shown, &viol), pw = (n_reviews + 63u) / 64u;
  if (w0 > w1 || w1 > pw) throw std::runtime_error("dev_delta_entries: the word range does not fit the table");
  if (off.size() != (size_t)(w1 - w0) + 1 || (extra && extra->size() != (size_t)(w1 - w0))) throw std::runtime_error("dev_delta_entries: no index for this page (dev_delta_index)");
  std::lock_guard<std::mutex> l(kept_mu());
  const Kept* k = base_of("dev_delta_entries", t, nc, nt, pw, use_base);
  delta_entries_words(DeltaWords{viol.data(), k ? k->base.data() : nullptr, shown.data(), k ? k->shown.data() : nullptr, nc, nt}, n_reviews, w0, w1,
                      extra ? extra->data() : nullptr, reviews, now, was);
  if (off.back() < off.front() || reviews->size() != (size_t)(off.back() - off.front()))
    throw std::runtime_error("dev_delta_entries: the index does not fit the bitmaps (evaluated again since dev_delta_index?)");
}

}  // namespace gk
