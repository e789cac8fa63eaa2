// TEST-ONLY CPU stand-in of dev_tviol_index / dev_tviol_entries (device.hpp; the device versions are gk_tviol_index + gk_tviol_emit in
// kernels.hip), linked into libgkgpu_hostemu.so beside hostemu.cpp.  Public device.hpp entries only, nothing of the emulation's
// internals: dev_tviol_note keeps the three bitmaps of a collected evaluation beside the table's address (until the next one or
// dev_tviol_forget) -- the emulation fills them whatever the download option says -- and the two entries are word-by-word loops over
// those copies (tviol_index_words / tviol_entries_words, on plain arrays: tests/native/table_stream_test.cpp checks them bit by bit).
#include <algorithm>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

#include "device.hpp"

namespace gk {

// one plan group on plain arrays: viol / err = [nc][nt] words, big = [nt]
struct TviolWords { const uint64_t *viol, *err, *big; uint32_t nc, nt, row0; };

static uint64_t tviol_valid(uint32_t n_reviews, uint32_t w) {
  const uint32_t left = n_reviews - w * 64u;
  return left < 64u ? (1ull << left) - 1ull : ~0ull;
}
// word w: the reviews with a bit in any row of any group, under care; *big_out = the too_big bits below n_reviews
static uint64_t tviol_any_word(const std::vector<TviolWords>& gs, uint32_t n_reviews, uint32_t w, uint64_t* big_out) {
  uint64_t acc = 0, big = 0;
  for (const TviolWords& g : gs) {
    big |= g.big[w];
    for (uint32_t r = 0; r < g.nc; r++) acc |= g.viol[(size_t)r * g.nt + w] | g.err[(size_t)r * g.nt + w];
  }
  big &= tviol_valid(n_reviews, w);
  if (big_out) *big_out = big;
  return acc & tviol_valid(n_reviews, w) & ~big;
}

void tviol_index_words(const std::vector<TviolWords>& gs, uint32_t n_reviews, std::vector<uint32_t>* cnt, std::vector<uint64_t>* any, uint64_t* beyond) {
  const uint32_t pw = (n_reviews + 63u) / 64u;
  cnt->assign(pw, 0);
  if (any) any->assign(pw, 0);
  *beyond = 0;
  if (gs.empty()) return;
  for (uint32_t w = 0; w < pw; w++) {
    uint64_t big = 0;
    const uint64_t a = tviol_any_word(gs, n_reviews, w, &big);
    (*cnt)[w] = (uint32_t)__builtin_popcountll(a);
    if (any) (*any)[w] = a;
    *beyond += (uint64_t)__builtin_popcountll(big);
  }
}

// dst |= the 64-bit piece moved to bit `bit0` of a mask of mw words
static void tviol_deposit(uint64_t* dst, uint32_t mw, uint64_t piece, uint32_t bit0) {
  const uint32_t wi = bit0 / 64u, sh = bit0 % 64u;
  if (wi < mw) dst[wi] |= piece << sh;
  if (sh && wi + 1u < mw) dst[wi + 1u] |= piece >> (64u - sh);
}

void tviol_entries_words(const std::vector<TviolWords>& gs, uint32_t n_reviews, uint32_t mw, uint32_t w0, uint32_t w1, std::vector<uint32_t>* reviews,
                         std::vector<uint64_t>* viol, std::vector<uint64_t>* err) {
  reviews->clear(); viol->clear(); err->clear();
  if (gs.empty()) return;
  for (uint32_t w = w0; w < w1; w++) {
    const uint64_t a = tviol_any_word(gs, n_reviews, w, nullptr);
    for (uint64_t m = a; m; m &= m - 1ull) {
      const uint32_t l = (uint32_t)__builtin_ctzll(m);
      reviews->push_back(w * 64u + l);
      const size_t at = viol->size();
      viol->resize(at + mw, 0); err->resize(at + mw, 0);
      for (const TviolWords& g : gs)
        for (uint32_t r0 = 0; r0 < g.nc; r0 += 64u) {   // a block of up to 64 rows: one piece per kind
          uint64_t pv = 0, pe = 0;
          for (uint32_t j = 0; j < 64u && r0 + j < g.nc; j++) {
            pv |= ((g.viol[(size_t)(r0 + j) * g.nt + w] >> l) & 1ull) << j;
            pe |= ((g.err[(size_t)(r0 + j) * g.nt + w] >> l) & 1ull) << j;
          }
          tviol_deposit(viol->data() + at, mw, pv, g.row0 + r0);
          tviol_deposit(err->data() + at, mw, pe, g.row0 + r0);
        }
    }
  }
}

namespace {
struct Kept { std::vector<uint64_t> viol, err, big; uint32_t n = 0, nc = 0, nt = 0; };
std::mutex& kept_mu() { static std::mutex m; return m; }
std::map<const DevTable*, Kept>& kept() { static std::map<const DevTable*, Kept> m; return m; }

// the kept evaluations of the sides as plain arrays (kept_mu held); throws what the device entries throw
uint32_t groups_of(const char* who, const std::vector<TviolSide>& sides, uint32_t n_reviews, std::vector<TviolWords>* gs, uint32_t* rows) {
  const uint32_t pw = (n_reviews + 63u) / 64u;
  *rows = 0;
  for (const TviolSide& s : sides) {
    if (s.nc == 0) continue;
    auto it = kept().find(s.t);
    if (it == kept().end() || it->second.nc != s.nc) throw std::runtime_error(std::string(who) + ": evaluate the table first");
    const Kept& k = it->second;
    if (k.n != n_reviews || k.nt < pw || k.viol.size() != (size_t)k.nc * k.nt || k.err.size() != k.viol.size() || k.big.size() < pw)
      throw std::runtime_error(std::string(who) + ": the review count does not fit the table");
    gs->push_back(TviolWords{k.viol.data(), k.err.data(), k.big.data(), k.nc, k.nt, s.row0});
    *rows = std::max(*rows, s.row0 + s.nc);
  }
  return pw;
}
}  // namespace

void dev_tviol_note(const DevTable* t, const EvalOut& o) {
  Kept k;
  k.n = o.n_reviews; k.nc = o.n_constraints; k.nt = o.n_tiles;
  k.viol = o.viol; k.err = o.err; k.big = o.too_big;
  std::lock_guard<std::mutex> l(kept_mu());
  kept()[t] = std::move(k);
}

void dev_tviol_forget(const DevTable* t) {
  std::lock_guard<std::mutex> l(kept_mu());
  kept().erase(t);
}

void dev_tviol_index(const std::vector<TviolSide>& sides, uint32_t n_reviews, std::vector<uint32_t>* cnt, std::vector<uint64_t>* any, uint64_t* beyond, float* ms) {
  *ms = 0;
  std::lock_guard<std::mutex> l(kept_mu());
  std::vector<TviolWords> gs;
  uint32_t rows = 0;
  groups_of("dev_tviol_index", sides, n_reviews, &gs, &rows);
  tviol_index_words(gs, n_reviews, cnt, any, beyond);
}

void dev_tviol_entries(const std::vector<TviolSide>& sides, uint32_t n_reviews, const std::vector<uint32_t>& off, uint32_t w0, uint32_t w1,
                       std::vector<uint32_t>* reviews, std::vector<uint64_t>* viol, std::vector<uint64_t>* err, float* ms) {
  *ms = 0;
  reviews->clear(); viol->clear(); err->clear();
  std::lock_guard<std::mutex> l(kept_mu());
  std::vector<TviolWords> gs;
  uint32_t rows = 0;
  const uint32_t pw = groups_of("dev_tviol_entries", sides, n_reviews, &gs, &rows);
  if (off.size() != (size_t)pw + 1) throw std::runtime_error("dev_tviol_entries: no index for this table (dev_tviol_index)");
  if (w0 > w1 || w1 > pw) throw std::runtime_error("dev_tviol_entries: the word range does not fit the table");
  tviol_entries_words(gs, n_reviews, (rows + 63u) / 64u, w0, w1, reviews, viol, err);
  if (off[w1] < off[w0] || reviews->size() != (size_t)(off[w1] - off[w0]))
    throw std::runtime_error("dev_tviol_entries: the index does not fit the bitmaps (evaluated again since dev_tviol_index?)");
}

}  // namespace gk
