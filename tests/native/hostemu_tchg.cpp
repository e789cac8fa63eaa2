// TEST-ONLY CPU stand-in of dev_snap_take / dev_tchg_align / dev_tchg_index / dev_tchg_entries (device.hpp; the device versions are
// gk_tchg_align + gk_tchg_index + gk_tchg_emit in kernels.hip), linked into libgkgpu_hostemu.so beside hostemu.cpp.  Public device.hpp
// entries only, nothing of the emulation's internals: dev_tchg_note keeps the three bitmaps of a collected evaluation beside the table's
// address (until the next one or dev_tchg_forget), and the entries are loops over plain arrays (tchg_align_words / tchg_index_words /
// tchg_entries_words: tests/native/table_delta_test.cpp checks them bit by bit).
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>

#include "device.hpp"

namespace gk {

// bitmaps in the flat layout: viol / err = [rows][pw] words (null: all zero), big = [pw] (null: zero), n reviews
struct TchgFlat { const uint64_t *viol, *err, *big; uint32_t rows, pw, n; };
// one plan group on plain arrays: viol / err = [nc][nt] words, big = [nt]
struct TchgGroup { const uint64_t *viol, *err, *big; uint32_t nc, nt, row0; };

static uint64_t tchg_valid(uint32_t n, uint32_t w) {
  const uint32_t left = n - w * 64u;
  return left < 64u ? (1ull << left) - 1ull : ~0ull;
}

// the groups' rows at their row0 in one flat layout of `rows` rows (out_viol / out_err = [rows][pw], out_big = [pw])
void tchg_flatten_words(const std::vector<TchgGroup>& gs, uint32_t rows, uint32_t pw, std::vector<uint64_t>* out_viol, std::vector<uint64_t>* out_err,
                        std::vector<uint64_t>* out_big) {
  out_viol->assign((size_t)rows * pw, 0); out_err->assign((size_t)rows * pw, 0); out_big->assign(pw, 0);
  for (const TchgGroup& g : gs) {
    for (uint32_t w = 0; w < pw; w++) (*out_big)[w] |= g.big[w];
    for (uint32_t r = 0; r < g.nc && g.row0 + r < rows; r++)
      for (uint32_t w = 0; w < pw; w++) {
        (*out_viol)[(size_t)(g.row0 + r) * pw + w] = g.viol[(size_t)r * g.nt + w];
        (*out_err)[(size_t)(g.row0 + r) * pw + w] = g.err[(size_t)r * g.nt + w];
      }
  }
}

// was_* = [rows_now][ceil(n / 64)]; then_of null: the identity
void tchg_align_words(const TchgFlat& s, uint32_t n, const uint32_t* then_of, const std::vector<uint32_t>& row_of, std::vector<uint64_t>* was_viol,
                      std::vector<uint64_t>* was_err, std::vector<uint64_t>* was_big) {
  const uint32_t pw = (n + 63u) / 64u, rows = (uint32_t)row_of.size();
  was_viol->assign((size_t)rows * pw, 0); was_err->assign((size_t)rows * pw, 0); was_big->assign(pw, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t p = then_of ? then_of[i] : i;
    if (p >= s.n) continue;
    const uint64_t bit = 1ull << (i % 64u);
    if (s.big && ((s.big[p / 64u] >> (p % 64u)) & 1ull)) (*was_big)[i / 64u] |= bit;
    for (uint32_t r = 0; r < rows; r++) {
      if (row_of[r] >= s.rows) continue;
      if (s.viol && ((s.viol[(size_t)row_of[r] * s.pw + p / 64u] >> (p % 64u)) & 1ull)) (*was_viol)[(size_t)r * pw + i / 64u] |= bit;
      if (s.err && ((s.err[(size_t)row_of[r] * s.pw + p / 64u] >> (p % 64u)) & 1ull)) (*was_err)[(size_t)r * pw + i / 64u] |= bit;
    }
  }
}

// word w of the changed reviews; now = the table's bitmaps in the flat layout (viol null: no sides), was = the aligned side
static uint64_t tchg_changed_word(const TchgFlat& now, const TchgFlat& was, const uint64_t* moved, const uint64_t* only, uint32_t w, uint64_t* big_out) {
  const uint32_t rows = was.rows;
  uint64_t acc = 0, any = 0;
  const uint64_t wb = was.big ? was.big[w] : 0ull;
  for (uint32_t r = 0; r < rows; r++) {
    const uint64_t x = now.viol ? now.viol[(size_t)r * now.pw + w] : 0ull, y = now.err ? now.err[(size_t)r * now.pw + w] : 0ull;
    const uint64_t a = was.viol ? was.viol[(size_t)r * was.pw + w] & ~wb : 0ull, b = was.err ? was.err[(size_t)r * was.pw + w] & ~wb : 0ull;
    acc |= (x ^ a) | (y ^ b);
    any |= x | y;
  }
  if (moved) acc |= moved[w] & any;
  const uint64_t big = (now.big ? now.big[w] : 0ull) & tchg_valid(was.n, w);
  if (big_out) *big_out = big;
  return acc & tchg_valid(was.n, w) & ~big & (only ? only[w] : ~0ull);
}

void tchg_index_words(const TchgFlat& now, const TchgFlat& was, const uint64_t* moved, const uint64_t* only, std::vector<uint32_t>* cnt,
                      std::vector<uint64_t>* changed, std::vector<uint64_t>* big, uint64_t* beyond) {
  const uint32_t pw = was.pw;
  cnt->assign(pw, 0); changed->assign(pw, 0); big->assign(pw, 0);
  *beyond = 0;
  for (uint32_t w = 0; w < pw; w++) {
    (*changed)[w] = tchg_changed_word(now, was, moved, only, w, &(*big)[w]);
    (*cnt)[w] = (uint32_t)__builtin_popcountll((*changed)[w]);
    *beyond += (uint64_t)__builtin_popcountll((*big)[w]);
  }
}

// drop / extra: null or [w1 - w0] words
void tchg_entries_words(const TchgFlat& now, const TchgFlat& was, const uint64_t* moved, const uint64_t* only, uint32_t w0, uint32_t w1, const uint64_t* drop,
                        const uint64_t* extra, std::vector<uint32_t>* reviews, std::vector<uint64_t>* viol, std::vector<uint64_t>* err,
                        std::vector<uint64_t>* was_viol, std::vector<uint64_t>* was_err) {
  reviews->clear(); viol->clear(); err->clear(); was_viol->clear(); was_err->clear();
  const uint32_t rows = was.rows, mw = (rows + 63u) / 64u;
  for (uint32_t w = w0; w < w1; w++) {
    uint64_t ch = tchg_changed_word(now, was, moved, only, w, nullptr);
    if (drop) ch &= ~drop[w - w0];
    if (extra) ch |= extra[w - w0] & tchg_valid(was.n, w);
    const uint64_t wb = was.big ? was.big[w] : 0ull;
    for (uint64_t m = ch; m; m &= m - 1ull) {
      const uint32_t l = (uint32_t)__builtin_ctzll(m);
      reviews->push_back(w * 64u + l);
      const size_t at = viol->size();
      viol->resize(at + mw, 0); err->resize(at + mw, 0); was_viol->resize(at + mw, 0); was_err->resize(at + mw, 0);
      for (uint32_t r = 0; r < rows; r++) {
        const uint64_t bit = 1ull << (r % 64u);
        if (now.viol && ((now.viol[(size_t)r * now.pw + w] >> l) & 1ull)) (*viol)[at + r / 64u] |= bit;
        if (now.err && ((now.err[(size_t)r * now.pw + w] >> l) & 1ull)) (*err)[at + r / 64u] |= bit;
        if ((wb >> l) & 1ull) continue;
        if (was.viol && ((was.viol[(size_t)r * was.pw + w] >> l) & 1ull)) (*was_viol)[at + r / 64u] |= bit;
        if (was.err && ((was.err[(size_t)r * was.pw + w] >> l) & 1ull)) (*was_err)[at + r / 64u] |= bit;
      }
    }
  }
}

struct DevSnap { std::vector<uint64_t> viol, err, big; uint32_t rows = 0, pw = 0, n = 0; };
struct DevAligned { std::vector<uint64_t> viol, err, big, moved, only; uint32_t rows = 0, pw = 0, n = 0; bool has_was = false, has_moved = false, has_only = false; };

namespace {
struct Kept { std::vector<uint64_t> viol, err, big; uint32_t n = 0, nc = 0, nt = 0; };
std::mutex& kept_mu() { static std::mutex m; return m; }
std::map<const DevTable*, Kept>& kept() { static std::map<const DevTable*, Kept> m; return m; }

// the sides' kept evaluations in the flat layout (kept_mu held); throws what the device entries throw
void flat_of(const char* who, const std::vector<TviolSide>& sides, uint32_t n_reviews, uint32_t min_rows, DevSnap* out) {
  const uint32_t pw = (n_reviews + 63u) / 64u;
  std::vector<TchgGroup> gs;
  uint32_t rows = min_rows;
  for (const TviolSide& s : sides) {
    if (s.nc == 0) continue;
    auto it = kept().find(s.t);
    if (it == kept().end() || it->second.nc != s.nc) throw std::runtime_error(std::string(who) + ": evaluate the table first");
    const Kept& k = it->second;
    if (k.n != n_reviews || k.nt < pw || k.viol.size() != (size_t)k.nc * k.nt || k.err.size() != k.viol.size() || k.big.size() < pw)
      throw std::runtime_error(std::string(who) + ": the review count does not fit the table");
    gs.push_back(TchgGroup{k.viol.data(), k.err.data(), k.big.data(), k.nc, k.nt, s.row0});
    rows = std::max(rows, s.row0 + s.nc);
  }
  out->rows = rows; out->pw = pw; out->n = n_reviews;
  tchg_flatten_words(gs, rows, pw, &out->viol, &out->err, &out->big);
}
TchgFlat flat_view(const DevSnap& s) { return TchgFlat{s.viol.data(), s.err.data(), s.big.data(), s.rows, s.pw, s.n}; }
TchgFlat was_view(const DevAligned& a) {
  return TchgFlat{a.has_was ? a.viol.data() : nullptr, a.has_was ? a.err.data() : nullptr, a.has_was ? a.big.data() : nullptr, a.rows, a.pw, a.n};
}
}  // namespace

void dev_tchg_note(const DevTable* t, const EvalOut& o) {
  Kept k;
  k.n = o.n_reviews; k.nc = o.n_constraints; k.nt = o.n_tiles;
  k.viol = o.viol; k.err = o.err; k.big = o.too_big;
  std::lock_guard<std::mutex> l(kept_mu());
  kept()[t] = std::move(k);
}
void dev_tchg_forget(const DevTable* t) {
  std::lock_guard<std::mutex> l(kept_mu());
  kept().erase(t);
}

DevSnap* dev_snap_take(const std::vector<TviolSide>& sides, uint32_t n_reviews) {
  std::unique_ptr<DevSnap> s(new DevSnap());
  std::lock_guard<std::mutex> l(kept_mu());
  flat_of("dev_snap_take", sides, n_reviews, 0, s.get());
  return s.release();
}
void dev_snap_free(DevSnap* s) { delete s; }
uint64_t dev_snap_bytes(const DevSnap* s) { return s ? (s->viol.size() + s->err.size() + s->big.size()) * 8u : 0u; }

DevAligned* dev_tchg_align(int, const DevSnap* s, uint32_t n, const std::vector<uint32_t>* then_of, const std::vector<uint32_t>& row_of,
                           const std::vector<uint64_t>* moved, const std::vector<uint64_t>* only, float* ms) {
  *ms = 0;
  std::unique_ptr<DevAligned> a(new DevAligned());
  a->rows = (uint32_t)row_of.size(); a->n = n; a->pw = (n + 63u) / 64u;
  if ((then_of && then_of->size() != n) || (!then_of && s && s->n != n)) throw std::runtime_error("dev_tchg_align: the join does not fit the table");
  if ((moved && moved->size() != a->pw) || (only && only->size() != a->pw)) throw std::runtime_error("dev_tchg_align: the review words do not fit the table");
  if (s) {
    for (uint32_t r : row_of) if (r != 0xFFFFFFFFu && r >= s->rows) throw std::runtime_error("dev_tchg_align: the row map does not fit the snapshot");
    if (then_of) for (uint32_t p : *then_of) if (p != 0xFFFFFFFFu && p >= s->n) throw std::runtime_error("dev_tchg_align: the join does not fit the snapshot");
    tchg_align_words(flat_view(*s), n, then_of ? then_of->data() : nullptr, row_of, &a->viol, &a->err, &a->big);
    a->has_was = true;
  }
  if (moved) { a->moved = *moved; a->has_moved = true; }
  if (only) { a->only = *only; a->has_only = true; }
  return a.release();
}
void dev_tchg_free(DevAligned* a) { delete a; }

void dev_tchg_index(const std::vector<TviolSide>& sides, uint32_t n, const DevAligned* a, std::vector<uint32_t>* cnt, std::vector<uint64_t>* changed,
                    std::vector<uint64_t>* big, uint64_t* beyond, float* ms) {
  *ms = 0;
  if (!a || a->n != n) throw std::runtime_error("dev_tchg_index: the aligned side does not fit the table");
  DevSnap now;
  TchgFlat nv{nullptr, nullptr, nullptr, a->rows, a->pw, n};
  std::lock_guard<std::mutex> l(kept_mu());
  if (!sides.empty()) {
    flat_of("dev_tchg_index", sides, n, a->rows, &now);
    if (now.rows != a->rows) throw std::runtime_error("dev_tchg_index: the rows do not fit the aligned side");
    nv = flat_view(now);
  }
  tchg_index_words(nv, was_view(*a), a->has_moved ? a->moved.data() : nullptr, a->has_only ? a->only.data() : nullptr, cnt, changed, big, beyond);
}

void dev_tchg_entries(const std::vector<TviolSide>& sides, uint32_t n, const DevAligned* a, const std::vector<uint32_t>& off, uint32_t w0, uint32_t w1,
                      const std::vector<uint64_t>& drop, const std::vector<uint64_t>& extra, std::vector<uint32_t>* reviews, std::vector<uint64_t>* viol,
                      std::vector<uint64_t>* err, std::vector<uint64_t>* was_viol, std::vector<uint64_t>* was_err, float* ms) {
  *ms = 0;
  reviews->clear(); viol->clear(); err->clear(); was_viol->clear(); was_err->clear();
  if (!a || a->n != n) throw std::runtime_error("dev_tchg_entries: the aligned side does not fit the table");
  if (w0 > w1 || w1 > a->pw) throw std::runtime_error("dev_tchg_entries: the word range does not fit the table");
  if (off.size() != (size_t)(w1 - w0) + 1 || (!drop.empty() && drop.size() != (size_t)(w1 - w0)) || (!extra.empty() && extra.size() != (size_t)(w1 - w0)))
    throw std::runtime_error("dev_tchg_entries: no index for this page (dev_tchg_index)");
  DevSnap now;
  TchgFlat nv{nullptr, nullptr, nullptr, a->rows, a->pw, n};
  std::lock_guard<std::mutex> l(kept_mu());
  if (!sides.empty()) {
    flat_of("dev_tchg_entries", sides, n, a->rows, &now);
    if (now.rows != a->rows) throw std::runtime_error("dev_tchg_entries: the rows do not fit the aligned side");
    nv = flat_view(now);
  }
  tchg_entries_words(nv, was_view(*a), a->has_moved ? a->moved.data() : nullptr, a->has_only ? a->only.data() : nullptr, w0, w1, drop.empty() ? nullptr : drop.data(),
                     extra.empty() ? nullptr : extra.data(), reviews, viol, err, was_viol, was_err);
  if (off.back() < off.front() || reviews->size() != (size_t)(off.back() - off.front()))
    throw std::runtime_error("dev_tchg_entries: the index does not fit the bitmaps (evaluated again since dev_tchg_index?)");
}

}  // namespace gk
