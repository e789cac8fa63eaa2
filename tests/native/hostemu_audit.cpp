// TEST-ONLY CPU stand-in of dev_audit_select (device.hpp; the device version is gk_audit_permute + gk_audit_select in kernels.hip),
// linked into libgkgpu_hostemu.so beside hostemu.cpp.  Plain loops over the bitmap of the table's most recent evaluation, which it
// gets through the public dev_last_viol: nothing of the emulation's internals.
#include <stdexcept>

#include "device.hpp"

namespace gk {

void dev_audit_select(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint32_t>& order, const std::vector<uint32_t>& grp,
                      const std::vector<uint64_t>& shown, uint64_t /*shown_gen*/, uint32_t k, uint32_t cap,
                      std::vector<uint32_t>* pairs, std::vector<uint32_t>* idx, std::vector<uint32_t>* n, std::vector<uint32_t>* ovf) {
  pairs->assign(nc, 0); idx->assign((size_t)nc * cap, 0xFFFFFFFFu); n->assign(nc, 0); ovf->assign(nc, 0);
  const uint32_t nt = (n_reviews + 63u) / 64u;
  std::vector<uint64_t> viol;
  dev_last_viol(t, nc, &viol);
  if (viol.size() != (size_t)nc * nt) throw std::runtime_error("dev_audit_select: evaluate the table first");
  if (order.size() != n_reviews || grp.size() != n_reviews || shown.size() < nt) throw std::runtime_error("dev_audit_select: order / grp / shown do not fit the table");
  for (uint32_t c = 0; c < nc; c++) {
    uint32_t count = 0, emitted = 0, grp_k = 0;
    bool open = k != 0;   // the list still takes entries
    for (uint32_t p = 0; p < n_reviews; p++) {
      const uint32_t rev = order[p];
      if (rev >= n_reviews) continue;
      if (!((viol[(size_t)c * nt + rev / 64u] & shown[rev / 64u]) >> (rev % 64u) & 1ull)) continue;
      if (open && count >= k && grp[p] != grp_k) open = false;
      if (open) {
        if (count == k - 1u) grp_k = grp[p];
        if (emitted < cap) (*idx)[(size_t)c * cap + emitted] = rev; else (*ovf)[c] = 1;
        emitted++;
      }
      count++;
    }
    (*pairs)[c] = count;
    (*n)[c] = emitted < cap ? emitted : cap;
  }
}

}  // namespace gk
