// TEST-ONLY CPU stand-in of the verification entries of device.hpp (the device versions: gk_verify_diff and its wrappers in kernels.hip),
// linked into libgkgpu_hostemu.so beside hostemu.cpp.  Public device.hpp entries only, nothing of the emulation's internals:
//   * dev_verify_eval evaluates through dev_eval_launch / dev_eval_finish WITH download and keeps the four bitmaps beside the table's
//     address (until the next dev_verify_eval of that table or dev_verify_forget); dev_verify_diff and dev_verify_flip are plain loops
//     over those copies.
//   * The emulation binds its code to a plan when the plan is uploaded: the generated plan source under GK_HOSTEMU_JIT=1 (the stand-in
//     of the plan-specialised kernel), else the interpreter (the stand-in of the bytecode kernel).  EvalOptions::bytecode therefore
//     selects the interpreter through the plan: dev_verify_twin uploads a twin of the plan with GK_HOSTEMU_JIT taken out of the
//     environment for the length of the upload (nullptr without the variable: the plan is interpreted already), and the engine
//     evaluates the bytecode side with the twin.  The specialised side ran iff the variable is set and the call is not a bytecode one.
//   * dev_plan_no_jit is without effect in the emulation: a quarantined plan goes on running the generated source here, with the same
//     answers; that it counts as not specialised from then on is the engine's bookkeeping.
#include <cstdlib>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

#include "device.hpp"

namespace gk {

namespace {
struct Kept { std::vector<uint64_t> v[4]; uint32_t n = 0, nc = 0; };   // [0] viol [1] err [2] match [3] too_big
std::mutex& kept_mu() { static std::mutex m; return m; }
std::map<const DevTable*, Kept>& kept() { static std::map<const DevTable*, Kept> m; return m; }
}  // namespace

// the comparison itself, on plain arrays: a[k] / b[k] = [nc][nt] words of kind k (nullptr: not compared), big_a / big_b = [nt]
void verify_diff_words(const uint64_t* const a[3], const uint64_t* const b[3], const uint64_t* big_a, const uint64_t* big_b, uint32_t nt, uint32_t nc,
                       const uint64_t* mask, uint32_t n_reviews, uint32_t cap, VerifyDiff* out) {
  const uint32_t pw = (n_reviews + 63u) / 64u;
  for (int k = 0; k < 3; k++) out->diff[k].assign(a[k] ? nc : 0, 0);
  out->diff_too_big = 0; out->entries_total = 0; out->entries.clear(); out->ms = 0;
  auto emit = [&](uint64_t x, uint64_t av, uint32_t kind, uint32_t row, uint32_t w) {
    for (uint64_t m = x; m; m &= m - 1ull) {
      const uint32_t bit = (uint32_t)__builtin_ctzll(m);
      if (out->entries_total < cap) out->entries.push_back(VerifyEntry{kind, row, w * 64u + bit, (uint32_t)((av >> bit) & 1ull)});
      out->entries_total++;
    }
  };
  for (uint32_t w = 0; w < pw; w++) {
    uint64_t valid = ~0ull;
    const uint32_t left = n_reviews - w * 64u;
    if (left < 64u) valid = (1ull << left) - 1ull;
    if (mask) valid &= mask[w];
    const uint64_t care = valid & ~(big_a[w] | big_b[w]), xb = (big_a[w] ^ big_b[w]) & valid;
    out->diff_too_big += (uint64_t)__builtin_popcountll(xb);
    emit(xb, big_a[w], VERIFY_TOO_BIG, 0, w);
    for (uint32_t k = 0; k < 3; k++) {
      if (!a[k]) continue;
      for (uint32_t r = 0; r < nc; r++) {
        const uint64_t av = a[k][(size_t)r * nt + w], x = (av ^ b[k][(size_t)r * nt + w]) & care;
        out->diff[k][r] += (uint64_t)__builtin_popcountll(x);
        emit(x, av, k, r, w);
      }
    }
  }
}

void dev_verify_eval(const DevPlan* p, const DevTable* t, const EvalOptions& opt, EvalOut* out) {
  EvalOptions o = opt;
  o.download = true;
  dev_eval_launch(p, t, o);
  dev_eval_finish(p, t, o, out);
  out->specialised = !opt.bytecode && getenv("GK_HOSTEMU_JIT") != nullptr;
  Kept k;
  k.n = out->n_reviews; k.nc = out->n_constraints;
  k.v[0] = out->viol; k.v[1] = out->err; k.v[3] = out->too_big;
  if (opt.want_match) k.v[2] = out->match;
  std::lock_guard<std::mutex> l(kept_mu());
  kept()[t] = std::move(k);
}

DevPlan* dev_verify_twin(int device, const HostPlan& fast, const HostPlan& big) {
  static std::mutex mu;   // (the environment is the process's: one twin at a time; test-only)
  std::lock_guard<std::mutex> l(mu);
  const char* j = getenv("GK_HOSTEMU_JIT");
  if (!j) return nullptr;
  const std::string keep = j;
  unsetenv("GK_HOSTEMU_JIT");
  DevPlan* p = nullptr;
  try { p = dev_plan_upload(device, fast, big); } catch (...) { setenv("GK_HOSTEMU_JIT", keep.c_str(), 1); throw; }
  setenv("GK_HOSTEMU_JIT", keep.c_str(), 1);
  return p;
}

void dev_verify_forget(const DevTable* t) {
  std::lock_guard<std::mutex> l(kept_mu());
  kept().erase(t);
}

void dev_verify_diff(const DevTable* a, const DevTable* b, uint32_t nc, uint32_t n_reviews, bool want_match, const std::vector<uint64_t>* mask,
                     uint32_t cap, VerifyDiff* out) {
  for (int k = 0; k < 3; k++) out->diff[k].assign(k < 2 || want_match ? nc : 0, 0);
  out->diff_too_big = 0; out->entries_total = 0; out->entries.clear(); out->ms = 0;
  if (nc == 0 || n_reviews == 0) return;
  std::lock_guard<std::mutex> l(kept_mu());
  auto ia = kept().find(a), ib = kept().find(b);
  if (ia == kept().end() || ib == kept().end()) throw std::runtime_error("dev_verify_diff: evaluate the table first");
  const Kept &ka = ia->second, &kb = ib->second;
  const uint32_t pw = (n_reviews + 63u) / 64u;
  if (ka.n != n_reviews || kb.n != n_reviews || (mask && mask->size() < pw)) throw std::runtime_error("dev_verify_diff: the two evaluations / the mask do not fit the table");
  for (int k = 0; k < 2; k++)
    if (ka.v[k].size() != (size_t)nc * pw || kb.v[k].size() != (size_t)nc * pw) throw std::runtime_error("dev_verify_diff: evaluate the table first");
  if (ka.v[3].size() != pw || kb.v[3].size() != pw) throw std::runtime_error("dev_verify_diff: evaluate the table first");
  if (want_match && (ka.v[2].size() != (size_t)nc * pw || kb.v[2].size() != (size_t)nc * pw)) throw std::runtime_error("dev_verify_diff: the evaluations hold no match bitmaps");
  const uint64_t* pa[3] = {ka.v[0].data(), ka.v[1].data(), want_match ? ka.v[2].data() : nullptr};
  const uint64_t* pb[3] = {kb.v[0].data(), kb.v[1].data(), want_match ? kb.v[2].data() : nullptr};
  verify_diff_words(pa, pb, ka.v[3].data(), kb.v[3].data(), pw, nc, mask ? mask->data() : nullptr, n_reviews, cap, out);
}

void dev_verify_flip(const DevTable* t, uint32_t nc, uint32_t kind, uint32_t row, uint32_t review, bool whole_word) {
  std::lock_guard<std::mutex> l(kept_mu());
  auto it = kept().find(t);
  if (it == kept().end()) throw std::runtime_error("dev_verify_flip: evaluate the table first");
  Kept& k = it->second;
  const uint32_t pw = (k.n + 63u) / 64u;
  if (kind == VERIFY_TOO_BIG) row = 0;
  if (kind > VERIFY_TOO_BIG || review >= k.n || row >= nc || k.v[kind].size() != (size_t)(kind == VERIFY_TOO_BIG ? 1u : nc) * pw)
    throw std::runtime_error("dev_verify_flip: no such bit in the table's most recent evaluation");
  k.v[kind][(size_t)row * pw + review / 64u] ^= whole_word ? ~0ull : 1ull << (review % 64u);
}

}  // namespace gk
