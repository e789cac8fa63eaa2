// TEST ONLY: prints the plan source of a plan whose formula code comes from stdin -- tests/test_dnf_form.py writes the formulas
// (known-answer plans and seeded random ones), compiles the text with g++ and runs accumulator tables through it.
// The accumulator words of a review are fixed:
//   0, 1 global predicate words | 2, 3 element counts | 4..6 mounts (scope 0: element word + one value slot in a word of its own)
//   7..9 the mounts' value slots | 10..21 volumes (scope 1: the value id packed into the element word)
// stdin: n_viol  n_code code...  n_segs seg_ends...
// usage: dnf_form_gen <parts>      (GK_JIT_DNF=0 in the environment: the general form)
#include "codegen.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  using namespace gk;
  HostPlan p;
  p.cheap.push_back(0);
  p.scopes.push_back(Scope{4u, 7u, 2u, 3, 1, 1});
  p.scopes.push_back(Scope{10u, GK_VAL_PACKED, 3u, 12, 1, 1});
  p.cursor_scope = {0, 1};
  p.n_real_scopes = 2;
  unsigned n_viol = 0, n = 0, x = 0;
  if (scanf("%u %u", &n_viol, &n) != 2) return 2;
  for (unsigned i = 0; i < n; i++) { if (scanf("%u", &x) != 1) return 2; p.code.push_back(x); }
  if (scanf("%u", &n) != 1) return 2;
  for (unsigned i = 0; i < n; i++) { if (scanf("%u", &x) != 1) return 2; p.seg_ends.push_back(x); }
  p.n_viol = n_viol;
  p.dims.n_scopes = 2;
  p.dims.n_code = (uint32_t)p.code.size();
  p.dims.n_gwords = 2;
  p.dims.acc_words = 22;
  p.dims.n_viol = n_viol;
  fputs(generate_plan_source(p, argc > 1 ? (uint32_t)atoi(argv[1]) : 2u).c_str(), stdout);
  return 0;
}
