// The plain host alternative to gk_viol_any + gk_viol_emit, for tools/resident_violations_cost.py (built by the probe with g++ -O3,
// loaded through ctypes): every review that has a bit in any row of viol or err, with its two constraint masks, from the bitmaps a
// sweep downloads anyway.  The algorithm of tests/native/hostemu_viol.cpp, word-wise and without that file's copy of the bitmap.
#include <cstddef>
#include <cstdint>

extern "C" {

// viol, err: [nc][nt] u64; shown: [nt]; out_review: [cap]; out_viol / out_err: [cap][mw], mw = ceil(nc / 64), zeroed by the caller.
// -> the number of entries (those beyond cap are counted, not stored)
uint64_t host_viol_entries(const uint64_t* viol, const uint64_t* err, const uint64_t* shown, uint32_t nc, uint32_t nt, uint32_t n_reviews, uint64_t cap,
                           uint32_t* out_review, uint64_t* out_viol, uint64_t* out_err) {
  const uint32_t mw = (nc + 63u) / 64u, pw = (n_reviews + 63u) / 64u;
  uint64_t n = 0;
  for (uint32_t w = 0; w < pw && w < nt; w++) {
    uint64_t any = 0;
    for (uint32_t r = 0; r < nc; r++) any |= viol[(size_t)r * nt + w] | err[(size_t)r * nt + w];
    any &= shown[w];
    const uint32_t valid = n_reviews - w * 64u;
    if (valid < 64u) any &= (1ull << valid) - 1ull;
    for (uint64_t m = any; m; m &= m - 1) {
      const uint32_t l = (uint32_t)__builtin_ctzll(m);
      if (n < cap) {
        out_review[n] = w * 64u + l;
        for (uint32_t r = 0; r < nc; r++) {
          out_viol[n * mw + r / 64u] |= ((viol[(size_t)r * nt + w] >> l) & 1ull) << (r % 64u);
          out_err[n * mw + r / 64u] |= ((err[(size_t)r * nt + w] >> l) & 1ull) << (r % 64u);
        }
      }
      n++;
    }
  }
  return n;
}

}  // extern "C"
