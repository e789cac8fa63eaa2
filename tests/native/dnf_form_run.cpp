// TEST ONLY: runs accumulator tables read from stdin through the plan source of dnf_form_gen.cpp (included as dnf_form_plan.inc):
// the staged parts (what the device runs, every share over the same words) and the monolithic function (the general form).
// in, per case:  flags  w0 .. w21        out, per case:  staged: viol(hex) w0 .. w9    monolithic: viol(hex) w0 .. w9
#include <cstdio>
#include <vector>

#include "vm_core.hpp"
#include "dnf_form_plan.inc"

struct VecAcc {
  std::vector<uint32_t>* w;
  void or_word(uint32_t i, uint32_t m) { (*w)[i] |= m; }
  void max_word(uint32_t i, uint32_t v) { if ((*w)[i] < v) (*w)[i] = v; }
  void store_word(uint32_t i, uint32_t v) { (*w)[i] = v; }
  uint32_t load(uint32_t i) const { return (*w)[i]; }
};

int main() {
  unsigned flags;
  while (scanf("%u", &flags) == 1) {
    std::vector<uint32_t> w(22, 0u);
    for (int i = 0; i < 22; i++) if (scanf("%u", &w[i]) != 1) return 2;
    const uint32_t bounds[gk::GK_MAX_SCOPES] = {w[2], w[3]};
    std::vector<uint32_t> ws = w, wm = w;
    VecAcc as{&ws}, am{&wm};
    gk::Results rs = {};
    for (uint32_t st = 0; st < gk::GK_N_STAGES; st++)
      for (uint32_t k = 0; k < gk::GK_GEN_PARTS; k++) gk::jit_formula_part(st * gk::GK_GEN_PARTS + k, as, flags, nullptr, bounds, rs, nullptr);
    gk::PlanView pv = {};
    const gk::Results rm = gk::jit_formulas(pv, am, flags, nullptr, nullptr, bounds);
    printf("%llx", (unsigned long long)rs.viol[0]);
    for (int i = 0; i < 10; i++) printf(" %u", ws[i]);
    printf("  %llx", (unsigned long long)rm.viol[0]);
    for (int i = 0; i < 10; i++) printf(" %u", wm[i]);
    printf("\n");
  }
  return 0;
}
