// Plan -> HIP source: the predicate dispatch (phase 1) and the formulas (phase 2) of ONE compiled plan as straight-line
// code over the same primitives the interpreter uses (vm_core.hpp: eval_pred with a constexpr Pred folds to the single
// operation; boolean registers become locals; loops become real loops with constant LDS offsets).  kernels.hip
// compiles the result for gfx950 with hiprtc when the plan is uploaded; tests/native/hostemu.cpp can compile the same
// text with g++ to validate the generator in the GPU-less container.
// The generator in its internal headers, bottom up: formula_code.hpp reads the formula code; codegen_forms.hpp holds the analyses that
// decide which form a loop or a run takes; codegen_cut.hpp deals the formula blocks to waves; codegen_emit.hpp writes the text.  This
// file is the public interface (codegen.hpp) and the order of the text.
#include "codegen.hpp"
#include "codegen_cut.hpp"
#include "codegen_emit.hpp"

#include <cstdio>

namespace gk {

using namespace cg;

std::vector<uint32_t> jit_path_classes(const HostPlan& plan, std::vector<std::vector<Pred>>* classes) {
  // distinct predicate lists -> class ids (1-based); entry[path] = class id | GK_ENT_NEEDS_STR, 0 = no predicates
  std::vector<uint32_t> out(plan.ptab.size(), 0);
  std::map<std::string, uint32_t> ids;
  classes->clear();
  classes->push_back({});
  for (size_t i = 0; i < plan.ptab.size(); i++) {
    uint32_t ent = plan.ptab[i];
    if (!ent) continue;
    uint32_t first = ent >> 8, cnt = ent & 0xFF;
    std::string key((const char*)&plan.path_preds[first], cnt * sizeof(Pred));
    bool str = false;
    for (uint32_t j = 0; j < cnt; j++) str = str || pred_needs_str(plan.path_preds[first + j]);
    auto it = ids.find(key);
    uint32_t id;
    if (it == ids.end()) {
      id = (uint32_t)classes->size();
      ids[key] = id;
      classes->emplace_back(plan.path_preds.begin() + first, plan.path_preds.begin() + first + cnt);
    } else id = it->second;
    out[i] = id | (str ? GK_ENT_NEEDS_STR : 0u);
  }
  // CANONICAL numbering: by the predicate lists themselves, not by the order in which key paths got their ids -- the host threads
  // of the first table's ingest intern paths in whatever order they meet them, and the generated text (hence the code-object
  // cache key, on disk too) must not depend on that: the same policy set over the same objects is the same kernel in every process
  std::vector<uint32_t> renum(classes->size(), 0);
  {
    uint32_t next = 1;
    for (auto& kv : ids) renum[kv.second] = next++;   // (std::map: ascending by the lists' bytes)
    std::vector<std::vector<Pred>> sorted(classes->size());
    for (size_t c = 1; c < classes->size(); c++) sorted[renum[c]] = std::move((*classes)[c]);
    classes->swap(sorted);
  }
  for (auto& e : out) if (e) e = renum[e & ~GK_ENT_NEEDS_STR] | (e & GK_ENT_NEEDS_STR);
  return out;
}

// result slots the plan-specialised kernel keeps per 64-review half: KV violation slots, KM match slots and KM error slots, in that
// order (kernel_body.inc s_masks).  In steps of four: 4 halves x (20 + 2 x 8) slots of configs[2] fit the 256-entry chunk-list buffer
// they alias.
uint32_t jit_res_kv(const HostPlan& plan) { return std::min<uint32_t>((uint32_t)GK_MAX_VIOL, std::max<uint32_t>(4u, (plan.n_viol + 3u) / 4u * 4u)); }
uint32_t jit_res_km(const HostPlan& plan) { return std::min<uint32_t>((uint32_t)GK_MAX_RES, std::max<uint32_t>(4u, (plan.n_match + 3u) / 4u * 4u)); }
uint32_t jit_res_k(const HostPlan& plan) { return jit_res_kv(plan) + 2u * jit_res_km(plan); }   // result words per half

namespace {

void emit_preamble(std::ostream& o, const HostPlan& plan) {
  // (GK_BIT: bit 0 of a formula value; the device text defines it as an opaque copy + mask BEFORE this source -- jit_source.hpp jit_res_macros,
  //  where the reason is written down; anything else that compiles the plan source gets the plain mask)
  o << "#ifndef GK_BIT\n#define GK_BIT(b) ((b) & 1u)\n#endif\n";
  o << "namespace gk {\n";
  // the plan's constant heap as a constant-initialised array: with constexpr predicates every constant-string load has
  // a compile-time address, so the optimiser folds the bytes into immediates (no memory traffic for constants)
  o << "GK_CONST_ARRAY unsigned char gk_plan_consts[" << plan.cheap.size() << "] = {";
  for (size_t i = 0; i < plan.cheap.size(); i++) o << (i ? "," : "") << (int)plan.cheap[i];
  o << "};\n";
  // accumulator words that must start at zero: all of them (an empty value slot is id 0)
  o << "#define GK_HAS_ZERO_RANGES 1\nconstexpr uint32_t GK_N_ZERO_RANGES = 1u;\n"
    << "GK_CONST_ARRAY uint32_t gk_zero_lo[1] = {0u};\nGK_CONST_ARRAY uint32_t gk_zero_hi[1] = {" << plan.dims.acc_words << "u};\n";
  // result slots kept per 64-review half and kind (kernel_body.inc GK_RES_K), and where each scope's element count lives
  // (the element scopes only: an alias cursor's loop is bounded by its scope's count -- cursors.hpp)
  const size_t n_real = plan.n_real_scopes;
  o << "#define GK_RES_KV " << jit_res_kv(plan) << "\n#define GK_RES_KM " << jit_res_km(plan) << "\n#define GK_N_SCOPES_K " << n_real << "\n"
    << "GK_CONST_ARRAY uint32_t gk_count_off[" << std::max<size_t>(1, n_real) << "] = {";
  for (size_t i = 0; i < n_real; i++) o << (i ? "," : "") << plan.scopes[i].count_off << "u";
  if (n_real == 0) o << "0u";
  o << "};\nGK_CONST_ARRAY uint32_t gk_scope_cap[" << std::max<size_t>(1, n_real) << "] = {";
  for (size_t i = 0; i < n_real; i++) o << (i ? "," : "") << plan.scopes[i].cap << "u";
  if (n_real == 0) o << "0u";
  o << "};\n";
}

// phase 1: jit_row, the dispatch over the predicate classes
void emit_jit_row(std::ostream& o, const HostPlan& plan) {
  std::vector<std::vector<Pred>> classes;
  jit_path_classes(plan, &classes);
  // inlined into its single call site (the chunk loop): as a separate function every LDS atomic would first look the
  // dynamic-LDS base up in a table (s_getpc + s_load + full wait; seen in the gfx950 ISA) and the call frame costs scratch
  o << "template <class Acc>\nGK_HD __attribute__((always_inline)) void jit_row(Row r, uint32_t cls, StrHdr h, const uint8_t* heap, Acc acc, bool on) {\n"
    << "  const uint8_t* cheap = gk_plan_consts;\n  (void)cheap; (void)h;\n  cls = GK_UNI(cls) & ~GK_ENT_NEEDS_STR;   // one class per call: the dispatch is a scalar branch\n";
  // The dispatch: one `switch` over the class (a balanced compare tree: the AMDGPU backend has no jump tables).  Testing the classes
  // that own most chunks first, in an if / else-if chain, measured slower (profiles/r02_variants_f_hot_dispatch.log,
  // r03_variants_l_*.log: 0.1148 ms with the plain switch, 0.1164 / 0.1177 / 0.1205 with chains of 2 / 4 / 6) and went in round 5 --
  // with it the generated text stopped depending on the table's chunk statistics: one policy set, one kernel, one cache entry.
  o << "  switch (cls) {\n";
  for (size_t c = 1; c < classes.size(); c++) o << "    case " << c << ": do { " << emit_row_class(plan, classes[c]) << "    } while (false);\n    break;\n";
  o << "    default: break;\n  }\n\n}\n\n";
}

// the formula registers, and the global predicate words: read once; derived global bits (F_STG) update the register copy as well
void emit_formula_locals(std::ostream& o, const HostPlan& plan) {
  o << "  uint32_t";
  for (int i = 0; i < 64; i++) o << (i ? ", " : " ") << "b" << i << " = 0u";
  o << ";\n";
  for (uint32_t w = 0; w < plan.dims.n_gwords; w++) o << "  uint32_t g" << w << " = acc.load(" << w << "u);\n";
}

// phase 2 in one function: every formula, in the general form
void emit_jit_formulas(std::ostringstream& o, const HostPlan& plan, bool sweep) {
  o << "template <class Acc>\nGK_HD Results jit_formulas(const PlanView& pv, Acc& acc, uint32_t flags, const Row* rows, const uint8_t* heap, const uint32_t* bounds) {\n"
    << "  (void)pv; (void)rows; (void)heap; (void)flags;\n  Results res = {};\n";
  emit_formula_locals(o, plan);
  FormulaEmitter em(plan, sweep);
  em.out = &o;
  em.gen(0, plan.code.size(), false, "  ");
  o << "  return res;\n}\n\n";
}

// one part in the preloaded form.  RUNS of consecutive blocks share one set of preloaded registers; a run ends where the words it keeps
// live would exceed `pre_live` (the kernel runs at an 80-VGPR budget: everything preloaded at the top of the part spilled 19 dwords).
// A later run re-reads what an earlier one derived: the same wave's LDS operations complete in order.
void emit_preloaded_part(std::ostringstream& o, const HostPlan& plan, FormulaEmitter& em, const std::vector<Blk>& blks, const std::vector<size_t>& order) {
  const size_t pre_live = JitSwitches::pre_live();
  std::set<uint32_t> bounds_done;
  std::ostringstream run_body;
  std::set<std::pair<uint32_t, uint32_t>> run_words;
  std::map<std::string, std::string> run_vals;
  auto flush = [&]() {
    if (run_body.str().empty()) return;
    o << "      {\n";
    for (auto& we : run_words) {
      const Scope& sc = plan.scopes[we.first];
      o << "      uint32_t W" << we.first << "_" << we.second << " = acc.load(" << (sc.word_off + we.second * sc.wpe) << "u);\n";
    }
    for (auto& kv : run_vals) o << "      const uint32_t " << kv.first << " = " << kv.second << ";\n";
    o << run_body.str() << "      }\n";
    run_body.str(""); run_body.clear(); run_words.clear(); run_vals.clear();
  };
  for (size_t bi : order) {
    std::ostringstream body;
    em.out = &body; em.pre = true;
    em.begin_block();
    em.gen(blks[bi].pc0, blks[bi].pc1, true, "      ");
    em.out = &o; em.pre = false;
    for (uint32_t sidx : em.pre_bounds) if (bounds_done.insert(sidx).second) { flush(); o << "      const uint32_t ns" << sidx << " = GK_UNI(bounds[" << sidx << "]);\n"; }
    std::set<std::pair<uint32_t, uint32_t>> uw = run_words;
    uw.insert(em.pre_words.begin(), em.pre_words.end());
    std::map<std::string, std::string> uv = run_vals;
    uv.insert(em.pre_vals.begin(), em.pre_vals.end());
    if (uw.size() + uv.size() > pre_live && !run_body.str().empty()) { flush(); uw = em.pre_words; uv = em.pre_vals; }
    run_words.swap(uw); run_vals.swap(uv);
    run_body << body.str();
  }
  flush();
}

// phase 2 as the share cut deals it: jit_formula_part, one case per part
void emit_jit_formula_part(std::ostringstream& o, const HostPlan& plan, const FormulaCut& cut, uint32_t NW, bool sweep, const JitSwitches& sw) {
  o << "#define GK_HAS_STAGES 1\nconstexpr uint32_t GK_N_STAGES = " << cut.n_stages << "u;\nconstexpr uint32_t GK_GEN_PARTS = " << NW << "u;\n"
    << "#ifndef GK_RES\n#define GK_RES(kind, slot, b) do { if ((kind) == 0) res.viol[0] |= (uint64_t)(b) << (slot); else if ((kind) == 1) res.match |= (uint64_t)(b) << (slot); "
       "else if ((kind) == 2) res.err |= (uint64_t)(b) << (slot); else res.viol[(kind) - 2] |= (uint64_t)(b) << (slot); } while (0)\n#define GK_RES_PROLOGUE\n#endif\n"
       "#ifndef GK_RES_FLUSH\n#define GK_RES_FLUSH(m0, m1, m2, m3, m4, m5)\n#endif\n"
    // GK_RESC: GK_RES of a compare-valued register -- the ballot tests the whole value, no opaque copy (jit_source.hpp GK_BIT); where the
    // result words do not ride in lanes (another compiler of this text, GK_JIT_RES_LANES=0) it is GK_RES
    << (JitSwitches::dnf() && sweep ? std::string("#ifndef GK_RESC\n") + (!sw.res_lanes ? "#if 0\n" : "#if defined(GK_WRITELANE2) && defined(GK_RES_BASE)\n") +
                              "#define GK_RESC(kind, slot, b) do { const unsigned long long m_ = __ballot((b) != 0u); GK_WRITELANE2(m_, slot, gk_rl##kind, gk_rh##kind); } while (0)\n"
                              "#else\n#define GK_RESC(kind, slot, b) GK_RES(kind, slot, b)\n#endif\n#endif\n" : std::string())
    << "template <class Acc>\nGK_HD void jit_formula_part(uint32_t part, Acc& acc, uint32_t flags, const uint8_t* heap, const uint32_t* bounds, Results& res, unsigned long long* masks) {\n"
    << "  (void)heap; (void)flags; (void)bounds; (void)res; (void)masks;\n  GK_RES_PROLOGUE\n";
  emit_formula_locals(o, plan);
  o << "  switch (part) {\n";
  FormulaEmitter em(plan, sweep);
  em.out = &o;
  for (size_t p = 0; p < cut.parts.size(); p++) {
    o << "    case " << p << ": {\n";
    for (auto& rs : em.res_slots) rs = 0;
    std::vector<size_t> order = cut.parts[p];
    std::sort(order.begin(), order.end());
    if (cut.use_pre) emit_preloaded_part(o, plan, em, cut.blks, order);
    else for (size_t bi : order) { em.begin_block(); em.gen(cut.blks[bi].pc0, cut.blks[bi].pc1, true, "      "); }
    // the part's finished slots leave the wave together (jit_source.hpp jit_res_macros: lane s holds slot s's word)
    static_assert(GK_VIOL_WORDS == 4, "GK_RES_FLUSH takes the masks of six kinds");
    char fb[256];
    snprintf(fb, sizeof fb, "      GK_RES_FLUSH(0x%llxull, 0x%llxull, 0x%llxull, 0x%llxull, 0x%llxull, 0x%llxull);\n", (unsigned long long)em.res_slots[0], (unsigned long long)em.res_slots[1],
             (unsigned long long)em.res_slots[2], (unsigned long long)em.res_slots[3], (unsigned long long)em.res_slots[4], (unsigned long long)em.res_slots[5]);
    o << fb << "    } break;\n";
  }
  o << "    default: break;\n  }\n";
  for (uint32_t w = 0; w < plan.dims.n_gwords; w++) o << "  (void)g" << w << ";\n";
  o << "}\n";
}

}  // namespace

std::string generate_plan_source(const HostPlan& plan, uint32_t parts) {
  std::ostringstream o;
  const bool sweep = parts <= 2;   // row groups of 128 reviews and more: resident tables of >= 8 192 reviews (engine.cpp)
  emit_preamble(o, plan);
  emit_jit_row(o, plan);
  emit_jit_formulas(o, plan, sweep);
  const JitSwitches sw;   // (the per-call switches: read here, behind the monolithic function, as ever)
  const FormulaCut cut = cut_formula_parts(plan, parts, sweep, sw);
  emit_jit_formula_part(o, plan, cut, parts, sweep, sw);
  o << "}  // namespace gk\n";
  return o.str();
}

}  // namespace gk
