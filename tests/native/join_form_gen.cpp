// TEST ONLY: prints the plan source of a hand-built plan whose one formula is a value join of the shape the audit set's
// "volumeMounts x volumes" has -- tests/test_join_form.py compiles the text with g++ and runs known-answer tables through it.
//   for each mount m (scope 0: element word + one value slot in a word of its own)
//     j = some volume v (scope 1: the value id packed into the element word) with  !bit1(v) && id(v) == id(m)
//     derived bit 3 of m |= j
//   violation 0 = some mount with j
// usage: join_form_gen <parts>      (GK_JIT_JOIN=0 in the environment: the general form)
#include "codegen.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  using namespace gk;
  HostPlan p;
  p.cheap.push_back(0);
  // accumulator words of a review: 0 globals | 1, 2 element counts | 3..5 mounts | 6..8 the mounts' value slots | 9..20 volumes
  p.scopes.push_back(Scope{3u, 6u, 1u, 3, 1, 1});
  p.scopes.push_back(Scope{9u, GK_VAL_PACKED, 2u, 12, 1, 1});
  p.cursor_scope = {0, 1};
  p.n_real_scopes = 2;
  p.code = {
      finst(F_LOOP, 0, 0, 4),
      finst(F_LOOP, 1, 0, 5),
      finst(F_LDE, 6, 1, 1),
      finst(F_NOT, 6, 6),
      finst(F_VEQ, 7), 1u | (0u << 8) | (0u << 16) | (0u << 24),
      finst(F_AND, 6, 6, 7),
      finst(F_ENDLOOP, 5, 6),
      finst(F_STE, 5, 0, 3),
      finst(F_ENDLOOP, 4, 5),
      finst(F_RES, 4, 0, 0),
      finst(F_END),
  };
  p.seg_ends = {(uint32_t)p.code.size() - 1u};
  p.n_viol = 1;
  p.dims.n_scopes = 2;
  p.dims.n_code = (uint32_t)p.code.size();
  p.dims.n_gwords = 1;
  p.dims.acc_words = 21;
  p.dims.n_viol = 1;
  fputs(generate_plan_source(p, argc > 1 ? (uint32_t)atoi(argv[1]) : 2u).c_str(), stdout);
  return 0;
}
