// TEST ONLY: runs accumulator tables read from stdin through the plan source of join_form_gen.cpp (included as join_form_plan.inc):
// the staged parts (what the device runs, every share over the same words) and the monolithic function (the general form).
// in, per case:  n_mounts n_volumes  m0 m1 m2  x0 x1 x2  v0 .. v11        out, per case:  staged: j0 j1 j2 viol   monolithic: j0 j1 j2 viol
#include <cstdio>
#include <vector>

#include "vm_core.hpp"
#include "join_form_plan.inc"

struct VecAcc {
  std::vector<uint32_t>* w;
  void or_word(uint32_t i, uint32_t m) { (*w)[i] |= m; }
  void max_word(uint32_t i, uint32_t v) { if ((*w)[i] < v) (*w)[i] = v; }
  void store_word(uint32_t i, uint32_t v) { (*w)[i] = v; }
  uint32_t load(uint32_t i) const { return (*w)[i]; }
};

int main() {
  unsigned nm, nv;
  while (scanf("%u %u", &nm, &nv) == 2) {
    std::vector<uint32_t> w(21, 0u);
    w[1] = nm; w[2] = nv;
    for (int i = 0; i < 3; i++) if (scanf("%u", &w[3 + i]) != 1) return 2;
    for (int i = 0; i < 3; i++) if (scanf("%u", &w[6 + i]) != 1) return 2;
    for (int i = 0; i < 12; i++) if (scanf("%u", &w[9 + i]) != 1) return 2;
    const uint32_t bounds[gk::GK_MAX_SCOPES] = {nm, nv};
    std::vector<uint32_t> ws = w, wm = w;
    VecAcc as{&ws}, am{&wm};
    gk::Results rs = {};
    for (uint32_t st = 0; st < gk::GK_N_STAGES; st++)
      for (uint32_t k = 0; k < gk::GK_GEN_PARTS; k++) gk::jit_formula_part(st * gk::GK_GEN_PARTS + k, as, 0u, nullptr, bounds, rs, nullptr);
    gk::PlanView pv = {};
    const gk::Results rm = gk::jit_formulas(pv, am, 0u, nullptr, nullptr, bounds);
    printf("%u %u %u %u  %u %u %u %u\n", (ws[3] >> 3) & 1u, (ws[4] >> 3) & 1u, (ws[5] >> 3) & 1u, (unsigned)(rs.viol[0] & 1u),
           (wm[3] >> 3) & 1u, (wm[4] >> 3) & 1u, (wm[5] >> 3) & 1u, (unsigned)(rm.viol[0] & 1u));
  }
  return 0;
}
