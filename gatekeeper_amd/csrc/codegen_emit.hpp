// The emitters of the plan code generator: one predicate class of phase 1 (emit_row_class), and the formulas of phase 2
// (FormulaEmitter: the state of the text being written and one method per form).  What takes which form is decided in
// codegen_forms.hpp; which block goes to which wave in codegen_cut.hpp.  Host only.
#pragma once
#include <cstring>
#include <sstream>
#include <string>

#include "chunks.hpp"
#include "codegen_forms.hpp"

namespace gk::cg {

inline std::string u(uint64_t v) { return std::to_string(v) + "u"; }
static const char* const kRel[] = {"==", "!=", "<", "<=", ">", ">="};   // CmpOp -> its operator (predicates, key and value relations)

inline std::string pred_literal(const Pred& p) {
  std::ostringstream o;
  o << "Pred{" << (int)p.op << "," << (int)p.dst << "," << (int)p.scope << "," << (int)p.level << "," << p.bit << "," << (int)p.cmp << ","
    << (int)p.ctype << "," << p.a << "u," << p.b << "u," << p.k << "ull," << p.idx << "," << p.pad << "u}";
  return o.str();
}

// ---------------------------------------------------------------------------------------------- phase 1
// One class = the predicates of one key path.  Results are gathered in one mask per destination word (a single LDS
// atomic per word, not per predicate); integer comparisons share one type test; short string equalities compare
// the packed payload; everything else goes through eval_pred with a constexpr predicate.
// -> the class's body: the class dispatch is wave-uniform and comes FIRST; the per-lane "this lane holds a row of this pass" test sits
// inside the case (around a divergent dispatch the structuriser threads every case exit through a chain of flow blocks)
inline std::string emit_row_class(const HostPlan& plan, const std::vector<Pred>& ps) {
  std::ostringstream o;
  // (a branch-free form of these bodies -- predicates as selects, every LDS atomic unconditional with a neutral operand -- measured
  //  level with this one in round 3, 0.1299 against 0.1287 ms on configs[2], profiles/r03_variants_c_*.log, and was removed in round 5)
  o << "if (on) {\n      const uint32_t t = r.meta & 7u; (void)t;\n";
  // a CARRIER class (plan.hpp T_ABSENT): the path's rows carry an element marker besides the member's own predicates, and an element
  // without the member has a row of type T_ABSENT there -- it exists for the marker alone: every other predicate of the class sees
  // "no row" (`real`), as eval_pred does
  bool mixed = false;
  for (const Pred& p : ps) if (p.op == P_PRESENT) mixed = true;
  if (mixed) o << "      const bool real = t != 7u; (void)real;\n";
  // (any other class: a T_ABSENT row may sit on its path all the same -- ANOTHER plan of the engine, or one loaded earlier, made the
  //  path a carrier -- and is no row to this class at all)
  else o << "      if (t != 7u) {\n";
  struct Group { int scope, level; bool always = false; std::vector<std::string> masks; std::vector<size_t> stores; bool present = false; };
  std::vector<Group> groups;          // element destinations by (scope, level)
  std::vector<std::string> gmasks;    // global destination words
  auto declare = [&](const std::string& name, std::vector<std::string>& list) {
    if (std::find(list.begin(), list.end(), name) == list.end()) { list.push_back(name); o << "      uint32_t " << name << " = 0u;\n"; }
  };
  auto group_of = [&](const Pred& p) -> Group& {
    for (auto& g : groups) if (g.scope == p.scope && g.level == p.level) return g;
    groups.push_back(Group{p.scope, p.level});
    return groups.back();
  };
  std::vector<std::string> target(ps.size());   // "mask |= bit" statement per predicate
  for (size_t i = 0; i < ps.size(); i++) {
    const Pred& p = ps[i];
    if (p.dst == D_GLOBAL) {
      std::string m = "mg" + std::to_string(p.bit >> 5);
      declare(m, gmasks);
      target[i] = m + " |= " + u(1u << (p.bit & 31)) + ";";
    } else {
      Group& g = group_of(p);
      if (p.op == P_STORE) { g.stores.push_back(i); g.always = true; if (p.level >= GK_LEVEL_ROOT) g.present = true; continue; }   // root scope: a store marks its element
      if (p.op == P_PRESENT) { g.present = true; g.always = true; continue; }
      std::string m = "me" + std::to_string(p.scope) + "_" + std::to_string(p.level) + "_" + std::to_string(elem_word_of_bit(p.bit));
      declare(m, g.masks);
      target[i] = m + " |= " + u(elem_mask_of_bit(p.bit)) + ";";
      if (p.op == P_DEFINED) g.always = true;
    }
  }
  // integer comparisons: one type test for all of them
  std::vector<size_t> icmp;
  for (size_t i = 0; i < ps.size(); i++) if (ps[i].op == P_CMP && ps[i].ctype == T_INT && !target[i].empty()) icmp.push_back(i);
  if (!icmp.empty()) {
    o << "      if (t == T_INT) {\n        const int64_t a = row_i64(r);\n";
    for (size_t i : icmp) o << "        if (a " << kRel[ps[i].cmp] << " " << (long long)(int64_t)ps[i].k << "ll) " << target[i] << "\n";
    o << "      } else {\n";
    for (size_t i : icmp) o << "        { constexpr Pred P = " << pred_literal(ps[i]) << "; if (eval_pred(r, P, h, heap, cheap)) " << target[i] << " }\n";
    o << "      }\n";
  }
  // predicates on components of split(trim(row, cut), sep): the split itself -- where the separators are, vm_core.hpp
  // SplitMask -- is computed ONCE per (cut, sep) of the class and shared by all of them (seven "banned tag" predicates on
  // containers[].image used to scan the string seven times, a byte per memory round trip)
  std::vector<uint32_t> split_pads;
  for (size_t i = 0; i < ps.size(); i++)
    if (!target[i].empty() && (ps[i].op == P_SPLIT_CMP || ps[i].op == P_SPLIT_COUNT || ps[i].op == P_SPLIT_PREFIX) &&
        std::find(split_pads.begin(), split_pads.end(), ps[i].pad) == split_pads.end()) split_pads.push_back(ps[i].pad);
  if (!split_pads.empty()) {
    o << "      const bool isstr = t == T_STRING;\n      const StrRef s_ = make_str(r, h, heap);\n";
    for (uint32_t pad : split_pads)
      o << "      SplitMask sm_" << pad << "; sm_" << pad << ".seps = 0ull; sm_" << pad << ".lo = 0u; sm_" << pad << ".hi = 0u; sm_" << pad << ".fast = true;\n"
        << "      if (isstr) sm_" << pad << " = split_mask(s_, (uint8_t)" << (pad >> 8) << "u, (uint8_t)" << (pad & 0xFFu) << "u);\n";
  }
  for (size_t i = 0; i < ps.size(); i++) {
    const Pred& p = ps[i];
    if (target[i].empty() || (p.op == P_CMP && p.ctype == T_INT)) continue;
    if (p.op == P_SPLIT_CMP || p.op == P_SPLIT_COUNT || p.op == P_SPLIT_PREFIX) {
      const std::string call = std::string(p.op == P_SPLIT_PREFIX ? "eval_split_prefix" : "eval_split_pred") + "(s_, sm_" + std::to_string(p.pad) + ", P, cheap)";
      o << "      { constexpr Pred P = " << pred_literal(p) << "; if (isstr && " << call << ") " << target[i] << " }\n";
      continue;
    }
    std::string cond;
    switch (p.op) {
      case P_DEFINED: cond = "true"; break;
      case P_TRUTHY: cond = "!(t == T_BOOL && r.lo == 0u)"; break;
      case P_TYPE: cond = "((" + u(p.ctype) + " >> t) & 1u) != 0u"; break;
      case P_BITS: cond = "(t == T_INT) && (((r.lo & " + u((uint32_t)p.k) + ") | (r.hi & " + u((uint32_t)(p.k >> 32)) + ")) != 0u)"; break;
      case P_COUNT_CMP: cond = std::string("(t == T_OBJECT || t == T_ARRAY) && ((int64_t)r.lo ") + kRel[p.cmp] + " " + std::to_string((long long)(int64_t)p.k) + "ll)"; break;
      case P_CMP:
        if (p.ctype == T_STRING && (p.cmp == C_EQ || p.cmp == C_NE) && p.b <= 7) {
          uint64_t bits = 0;
          for (uint32_t k = 0; k < p.b; k++) bits |= (uint64_t)plan.cheap[p.a + k] << (8 * k);
          uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32) | (p.b << 24);
          cond = std::string(p.cmp == C_NE ? "!" : "") + "((r.meta & (7u | ROW_STR_INLINE)) == (4u | ROW_STR_INLINE) && r.lo == " + u(lo) + " && r.hi == " + u(hi) + ")";
        }
        break;
      case P_STR_IN_SET: {   // all members short: compare the packed payload of an inline string row
        bool all_short = p.b > 0 && p.b <= 8;
        for (uint32_t k = 0; k < p.b && all_short; k++) {
          uint32_t len; memcpy(&len, &plan.cheap[p.a + 12 * k + 8], 4);
          if (len > 7) all_short = false;
        }
        if (!all_short) break;
        cond = "(r.meta & (7u | ROW_STR_INLINE)) == (4u | ROW_STR_INLINE) && (";
        for (uint32_t k = 0; k < p.b; k++) {
          uint32_t ea, eb, len;
          memcpy(&ea, &plan.cheap[p.a + 12 * k], 4); memcpy(&eb, &plan.cheap[p.a + 12 * k + 4], 4); memcpy(&len, &plan.cheap[p.a + 12 * k + 8], 4);
          cond += std::string(k ? " || " : "") + "(r.lo == " + u(ea) + " && r.hi == " + u(eb | (len << 24)) + ")";
        }
        cond += ")";
        break;
      }
      default: break;
    }
    if (mixed && !cond.empty()) cond = cond == "true" ? "real" : "real && (" + cond + ")";
    if (cond.empty()) o << "      { constexpr Pred P = " << pred_literal(p) << "; if (eval_pred(r, P, h, heap, cheap)) " << target[i] << " }\n";
    else if (cond == "true") o << "      " << target[i] << "\n";
    else o << "      if (" << cond << ") " << target[i] << "\n";
  }
  for (const std::string& m : gmasks) o << "      if (" << m << ") acc.or_word(" << m.substr(2) << "u, " << m << ");\n";
  for (const Group& g : groups) {
    const Scope& sc = plan.scopes[g.scope];
    std::string hit = g.always ? ((mixed && !(g.present && g.level < (int)GK_LEVEL_ROOT)) ? "real" : "true") : "";   // (only the marker's own group is written for a T_ABSENT row)
    if (!g.always) for (size_t k = 0; k < g.masks.size(); k++) hit += (k ? " | " : "") + g.masks[k];
    if (!g.always) hit = "(" + hit + ") != 0u";
    o << "      if (" << hit << ") {\n        const uint32_t ord = row_ordinal(r, " << g.level << "u);\n"
      << "        if (ord >= " << sc.cap << "u || (r.meta & ROW_ORD_OVERFLOW)) acc.or_word(0u, 1u);\n        else {\n";
    std::string extra;
    // a stored value = the row's VALUE ID (plan.hpp); a row without one (non-empty container, stale table) or with the
    // overflow id cannot be compared: the review goes beyond the limits (vm_core.hpp P_STORE)
    if (!g.stores.empty()) {
      if (mixed) o << "          const uint32_t vid = real ? row_vid(r) : 0u;\n          if (real && (vid == 0u || vid >= GK_VID_OVERFLOW)) acc.or_word(0u, 1u); else {\n";
      else o << "          const uint32_t vid = row_vid(r);\n          if (vid == 0u || vid >= GK_VID_OVERFLOW) acc.or_word(0u, 1u); else {\n";
    }
    for (size_t i : g.stores) {
      const Pred& p = ps[i];
      if (scope_packed(sc)) extra += " | (vid << " + std::to_string(ELEM_VID_SHIFT) + "u)";
      else o << "          " << (mixed ? "if (real) " : "") << "acc.store_word(" << sc.val_off << "u + ord * " << val_stride(sc.nvals) << "u + " << p.bit << "u, vid);\n";
    }
    if (g.present) {
      if (g.level > 0 && g.level < (int)GK_LEVEL_ROOT) extra += " | 1u | (row_ordinal(r, " + std::to_string(g.level - 1) + "u) << 24)";
      else extra += " | 1u";
      o << "          acc.max_word(" << sc.count_off << "u, ord + 1u);\n";
    }
    bool w0_done = false;
    for (const std::string& m : g.masks) {
      uint32_t wi = (uint32_t)atoi(m.substr(m.rfind('_') + 1).c_str());
      if (wi == 0) { o << "          acc.or_word(" << sc.word_off << "u + ord * " << (int)sc.wpe << "u, " << m << extra << ");\n"; w0_done = true; }
      else o << "          if (" << m << ") acc.or_word(" << sc.word_off << "u + ord * " << (int)sc.wpe << "u + " << wi << "u, " << m << ");\n";
    }
    if (!w0_done && !extra.empty()) o << "          acc.or_word(" << sc.word_off << "u + ord * " << (int)sc.wpe << "u, 0u" << extra << ");\n";
    if (!g.stores.empty()) o << "          }\n";
    o << "        }\n      }\n";
  }
  if (!mixed) o << "      }\n";
  o << "    }\n";
  return o.str();
}

// ---------------------------------------------------------------------------------------------- phase 2
// The text of formula code, instruction by instruction: boolean registers are locals b<r>, a loop at depth d has the element counter
// e<d>, its element's word 0 in w<d> and "this element is present (and its parent's)" in v<d>.
// PRELOADED form of the staged parts (round 5, `pre`).  The formulas are LDS-latency bound: every loop of every formula re-reads its
// scope's element words (an LDS round trip in front of a handful of bit operations; ~450 instructions took 10 k clocks per
// row group).  Here a part reads each element word it needs ONCE, up front -- all reads in flight together -- into registers
// W<scope>_<element>; loops are unrolled by the generator (every iteration a copy of the body with the element index as a
// literal; iterations beyond the wave's largest element count are skipped by a scalar branch), derived element bits update the
// register copy as well as LDS.  Used when the unrolled text stays small (codegen_cut.hpp `pre_budget` operations per plan);
// GK_JIT_PRELOAD=0 keeps the loops.
class FormulaEmitter {
 public:
  FormulaEmitter(const HostPlan& plan, bool sweep) : plan(plan), code(plan.code), sweep(sweep), dnf_on(JitSwitches::dnf()) {}

  std::ostringstream* out = nullptr;                   // where the text goes
  bool pre = false;                                    // generating the preloaded form
  std::set<std::pair<uint32_t, uint32_t>> pre_words;   // (scope, element) words the block being generated reads
  std::set<uint32_t> pre_bounds;                       // scopes whose run-time bound the block needs
  std::map<std::string, std::string> pre_vals;         // unpacked value slots: register name -> its load
  // result slots (per KIND) the staged part being generated hands to GK_RES.  Kinds: 0 = violation slots 0..63, 1 = match, 2 = error,
  // 3.. = violation slots 64.., 128.., 192.. (one kind per bank of 64: a kind's words ride in one register pair, lane = slot & 63)
  uint64_t res_slots[2 + GK_VIOL_WORDS] = {};

  // in front of every block: nothing of the block before it is open, known or wanted (the registers are reused)
  void begin_block() {
    pre_words.clear(); pre_bounds.clear(); pre_vals.clear();
    stack.clear();
    for (bool& x : cmpv) x = false;
    run_start = true;
  }

  // the instructions [pc0, pc1) at indentation `ind`.  -> true: the last of them was the F_ENDLOOP / F_ENDLOOP2 that closes an unrolled
  // copy of its loop's body (unrolled_loop below called with the body and that end)
  bool gen(size_t pc0, size_t pc1, bool staged, std::string ind) {
    std::ostringstream& o = *out;
    for (size_t pc = pc0; pc < pc1;) {
      const FIns i = decode(code[pc++]);
      const uint32_t op = i.op, a = i.a, b = i.b, c = i.c;
      // (the DNF form and the plain tests: in the unrolled parts of the sweep geometry only, as the join form)
      const bool dnf_ok = dnf_on && sweep && pre && staged;
      if (dnf_ok && stack.empty() && run_start) {
        run_start = false;
        DnfRun rn;
        if (dnf_run(plan, pc - 1, pc1, &rn)) { emit_run(rn, ind); pc = rn.at; continue; }   // (the run's F_RES / F_STG: below, as ever)
      }
      if (op == F_RES || op == F_STG) run_start = stack.empty();
      track_cmpv(i);
      // the test of a formula value: bit 0 through the opaque copy (GK_BIT), but for a compare-valued register -- it has no other bits
      const auto bit_of = [&](uint32_t r) { return dnf_ok && cmpv[r] ? "b" + std::to_string(r) + " != 0u" : "GK_BIT(b" + std::to_string(r) + ")"; };
      switch (op) {
        case F_LDG: o << ind << "b" << a << " = (g" << (global_bit(i) >> 5) << " >> " << (global_bit(i) & 31) << ") & 1u;\n"; break;
        case F_LDF: o << ind << "b" << a << " = (flags >> " << b << ") & 1u;\n"; break;
        case F_LDE: {
          const Scope& sc = plan.scopes[b];
          const int d = depth_of(b, "codegen: element load outside its loop");
          // booleans are 0/1 integers in vector registers (bitwise VALU ops), not wave masks in scalar registers
          const uint32_t sh = (uint32_t)__builtin_ctz(elem_mask_of_bit(c));
          if (elem_word_of_bit(c) == 0) o << ind << "b" << a << " = (w" << d << " >> " << sh << "u) & 1u;\n";
          else o << ind << "b" << a << " = (acc.load(" << sc.word_off << "u + e" << d << " * " << (int)sc.wpe << "u + " << elem_word_of_bit(c) << "u) >> " << sh << "u) & 1u;\n";
          break;
        }
        case F_AND: o << ind << "b" << a << " = b" << b << " & b" << c << ";\n"; break;
        case F_OR: o << ind << "b" << a << " = b" << b << " | b" << c << ";\n"; break;
        case F_NOT: o << ind << "b" << a << " = b" << b << " ^ 1u;\n"; break;
        case F_ANDN: o << ind << "b" << a << " = b" << b << " & (b" << c << " ^ 1u);\n"; break;
        case F_CONST: o << ind << "b" << a << " = " << ((b & 1) ? "1u" : "0u") << ";\n"; break;
        case F_MOV: o << ind << "b" << a << " = b" << b << ";\n"; break;
        case F_LOOP: {
          o << ind << "b" << c << " = 0u;\n";
          const size_t end = loop_end(code, pc);
          // (the join form: in the unrolled parts of the sweep geometry only -- the 64-review text of admission batches is latency-bound
          //  and stays byte for byte what it was)
          const bool conj_on = JitSwitches::conj(), join_ok = JitSwitches::join() && sweep && pre;
          const LoopClass lc = classify_loop(plan, i, pc, end, conj_on, join_ok, dnf_ok, [&](uint32_t so) { return var_of(so) >= 0; });
          if (lc.form == LoopForm::Conjunction) conjunction_loop(i, lc.cj, ind);
          else if (lc.form == LoopForm::Dnf) dnf_loop(i, lc.dl, ind);
          else if (pre && !is_alias(plan, a)) unrolled_loop(i, pc, end, staged, ind);
          else {
            // small capacities: constant trip count, fully unrolled -- the element words of absent elements are zero, so
            // they contribute nothing, and the compiler can issue all LDS reads of the nest at once
            constexpr uint64_t unroll_max = 4;
            if (plan.scopes[a].cap <= 16 && nest_of(a) <= unroll_max && !is_alias(plan, a)) constant_loop(i, ind);
            else runtime_loop(i, ind);
            ind += "    ";
            break;
          }
          pc = end + 1;
          run_start = stack.empty();
          break;
        }
        case F_ENDLOOP: case F_ENDLOOP2: {   // F_ENDLOOP2, the counting loop: a = once, b = body, c = twice
          const int d = stack.back().depth;
          if (op == F_ENDLOOP2) o << ind << "b" << c << " = b" << c << " | (b" << a << " & b" << b << " & v" << d << ");\n";
          o << ind << "b" << a << " = b" << a << " | (b" << b << " & v" << d << ");\n";
          if (pre && !stack.back().rt) { stack.pop_back(); o << ind.substr(0, ind.size() - 2) << "}\n"; return true; }
          stack.pop_back();
          run_start = stack.empty();
          for (bool& x : cmpv) x = false;   // (a run-time loop may not run at all: its registers are what they were)
          ind = ind.substr(0, ind.size() - 4);
          o << ind << "  }\n" << ind << "}\n";
          break;
        }
        case F_VEQ: {
          const SlotWord s = decode_slots(code[pc++]);
          const int da = var_of(s.sa), db = var_of(s.sb);
          if (da < 0 || db < 0) throw Unsupported("codegen: join outside its loops");
          o << ind << "b" << a << " = (uint32_t)vid_eq(" << vid(plan.scopes[s.sa], da, s.la) << ", " << vid(plan.scopes[s.sb], db, s.lb) << ");\n";
          break;
        }
        case F_STE: {
          const Scope& sc = plan.scopes[b];
          const int d = depth_of(b, "codegen: element store outside its loop");
          const int lit = lit_of(d);
          if (pre && elem_word_of_bit(c) == 0 && pre_words.count({b, (uint32_t)lit})) {
            o << ind << "if (" << bit_of(a) << ") { acc.or_word(" << sc.word_off << "u + e" << d << " * " << (int)sc.wpe << "u, " << u(elem_mask_of_bit(c)) << "); W" << b << "_" << lit << " |= " << u(elem_mask_of_bit(c)) << "; }\n";
            break;
          }
          o << ind << "if (" << bit_of(a) << ") acc.or_word(" << sc.word_off << "u + e" << d << " * " << (int)sc.wpe << "u + " << elem_word_of_bit(c) << "u, " << u(elem_mask_of_bit(c)) << ");\n";
          break;
        }
        case F_STG: {
          const uint32_t bit = global_bit(i);
          if (staged) o << ind << "if (" << bit_of(a) << ") { g" << (bit >> 5) << " |= " << u(1u << (bit & 31)) << "; acc.or_word(" << (bit >> 5) << "u, " << u(1u << (bit & 31)) << "); }\n";
          else o << ind << "if (" << bit_of(a) << ") g" << (bit >> 5) << " |= " << u(1u << (bit & 31)) << ";\n";
          break;
        }
        case F_RES: {
          const char* f = b == 0 ? "viol" : b == 1 ? "match" : "err";
          // staged parts hand the result of slot c to GK_RES: on the device one ballot turns the 64 lanes' answers into the
          // slot's bitmap word (kernel_body.inc), elsewhere it accumulates into `res` like the monolithic function
          if (staged) {
            const uint32_t kind = (b == 0 && c >= 64) ? 2u + (c >> 6) : b, lane_ = (b == 0) ? (c & 63u) : c;
            if (kind >= 2u + GK_VIOL_WORDS || lane_ >= 64u) throw Unsupported("codegen: result slot out of range");
            o << ind << (dnf_ok && cmpv[a] ? "GK_RESC(" : "GK_RES(") << kind << ", " << lane_ << ", b" << a << ");\n";
            res_slots[kind] |= 1ull << lane_;
          } else if (b == 0) o << ind << "res.viol[" << (c >> 6) << "] |= (uint64_t)b" << a << " << " << (c & 63u) << ";\n";
          else o << ind << "res." << f << " |= (uint64_t)b" << a << " << " << c << ";\n";
          break;
        }
        case F_END: pc = pc1; break;
        default: {
          if (is_vcmp(op)) {
            // F_VCMP (cursors.hpp): an ordering relation of two value ids -- ranks -- in the general form, both read as F_VEQ reads them;
            // an empty slot (0) is in no relation.  (The join and the DNF form decline a body that holds one: their xor is for equality.)
            const SlotWord s = decode_slots(code[pc++]);
            const int da = var_of(s.sa), db = var_of(s.sb);
            if (da < 0 || db < 0) throw Unsupported("codegen: value relation outside its loops");
            vid_in_place = true;
            const std::string xa = vid(plan.scopes[s.sa], da, s.la), xb = vid(plan.scopes[s.sb], db, s.lb);
            vid_in_place = false;
            o << ind << "{ const uint32_t xa_ = " << xa << ", xb_ = " << xb << "; b" << a
              << " = (uint32_t)((xa_ " << kRel[op - F_VCMP] << " xb_) & (xa_ != 0u) & (xb_ != 0u)); }\n";
            break;
          }
          if (is_kimm(op) || op == F_KEND) {
            // F_KIMM / F_KEND (cursors.hpp): the loop's element counter against a constant / against the lane's own element count of the
            // scope, which phase 1 left in the accumulators (read once per run of the preloaded form).  In an unrolled copy the counter is
            // a literal and F_KIMM folds away; an indexed loop has no other copies (unrolled_loop)
            const int d = var_of(b);
            if (d < 0) throw Unsupported("codegen: index test outside its loop");
            if (op != F_KEND) { o << ind << "b" << a << " = (uint32_t)(e" << d << " " << kRel[op - F_KIMM] << " " << c << "u);\n"; break; }
            std::string n = "acc.load(" + u(plan.scopes[b].count_off) + ")";
            if (pre) { const std::string name = "N" + std::to_string(scope_of(plan, b)); pre_vals[name] = n; n = name; }
            o << ind << "b" << a << " = (uint32_t)(e" << d << " + " << c << "u == " << n << ");\n";
            break;
          }
          if (!is_kcmp(op)) throw Unsupported("codegen: unknown formula op");
          // F_KCMP (cursors.hpp): the relation of two cursors' ordinals = of the two loops' element counters
          const int da = var_of(b), db = var_of(c);
          if (da < 0 || db < 0) throw Unsupported("codegen: key relation outside its loops");
          o << ind << "b" << a << " = (uint32_t)(e" << da << " " << kRel[op - F_KCMP] << " e" << db << ");\n";
          break;
        }
      }
    }
    return false;
  }

 private:
  const HostPlan& plan;
  const std::vector<uint32_t>& code;
  const bool sweep;    // row groups of 128 reviews and more
  const bool dnf_on;
  // scope: the loop's CURSOR (cursors.hpp; the scope table is indexed by cursor) | lit: the element index as a literal (preloaded
  // form), -1: a run-time loop variable | rt: a run-time loop inside the preloaded form (an alias cursor's loop)
  struct Loop { uint32_t scope; int depth; int lit; bool rt = false; };
  std::vector<Loop> stack;
  bool cmpv[64] = {};        // COMPARE-VALUED registers of the block being generated: built of compare results and constants only
  bool run_start = false;    // the next top-level instruction starts a run (block start, behind a loop, behind F_RES / F_STG)
  // (vid_in_place: an ordering relation reads its unpacked slots where it uses them -- one LDS read with a constant address in an unrolled
  //  copy -- instead of keeping every element's ids in registers across the part: four relations over a 16-element scope with two
  //  slots held 32 more registers live and pushed the 256-review text past its budget, 52 bytes of scratch per lane)
  bool vid_in_place = false;

  int var_of(uint32_t scope) const {
    for (size_t i = stack.size(); i-- > 0;) if (stack[i].scope == scope) return stack[i].depth;
    return -1;
  }
  int depth_of(uint32_t scope, const char* or_throw) const {
    const int d = var_of(scope);
    if (d < 0) throw Unsupported(or_throw);
    return d;
  }
  int parent_depth(const FIns& loop) const { return loop.b ? depth_of(loop.b - 1, "codegen: parent loop not open") : -1; }   // (F_LOOP b: the parent's cursor + 1)
  int lit_of(int d) const {   // the literal element index of the loop at depth d, -1: a run-time loop variable
    int lit = -1;
    for (const Loop& l : stack) if (l.depth == d) lit = l.lit;
    return lit;
  }
  uint64_t nest_of(uint32_t cursor) const {   // iterations of a loop over `cursor` here, by capacities
    uint64_t n = plan.scopes[cursor].cap;
    for (const Loop& l : stack) n *= plan.scopes[l.scope].cap;
    return n;
  }

  void track_cmpv(const FIns& i) {
    const bool cv_b = i.b < 64 && cmpv[i.b], cv_c = i.c < 64 && cmpv[i.c];   // (of the operands, before the destination -- often one of them -- changes)
    const uint32_t op = i.op;
    if (op == F_LDG || op == F_LDF || op == F_LDE) cmpv[i.a] = false;
    else if (op == F_AND || op == F_OR || op == F_ANDN) cmpv[i.a] = cv_b && cv_c;
    else if (op == F_NOT || op == F_MOV) cmpv[i.a] = cv_b;
    else if (op == F_CONST || op == F_VEQ || is_kcmp(op) || is_vcmp(op) || is_kimm(op) || op == F_KEND) cmpv[i.a] = true;
    else if (op == F_LOOP) cmpv[i.c] = true;   // (b<c> = 0u; a conjunction / join / DNF loop leaves its t_ there, any other its F_ENDLOOP decides)
    else if (op == F_ENDLOOP) cmpv[i.a] = false;   // (v<d>: an extract)
    else if (op == F_ENDLOOP2) { cmpv[i.a] = false; cmpv[i.c] = false; }
  }
  void forget_body(size_t pc, size_t end) {   // the registers the instructions [pc, end) write: not compare-valued any more
    for (size_t q = pc; q < end; q = next_ins(code, q)) for (uint32_t r : reg_use(decode(code[q])).writes) cmpv[r] = false;
  }

  // value id of slot `slot` of the element loop depth `d` is at (scope S): packed into the element word, a preloaded register, or read in place
  std::string vid(const Scope& S, int d, uint32_t slot) {
    std::ostringstream x;
    const int lit = lit_of(d);
    if (scope_packed(S)) x << "((w" << d << " >> " << ELEM_VID_SHIFT << "u) & " << GK_VID_OVERFLOW << "u)";   // word0 of the loop's current element is in a register
    else if (pre && !vid_in_place && lit >= 0) {
      const std::string name = "X" + std::to_string(&S - &plan.scopes[0]) + "_" + std::to_string(lit) + "_" + std::to_string(slot);
      pre_vals[name] = "acc.load(" + std::to_string(S.val_off + (uint32_t)lit * val_stride(S.nvals) + slot) + "u)";
      x << name;
    }
    else x << "acc.load(" << S.val_off << "u + e" << d << " * " << val_stride(S.nvals) << "u + " << slot << "u)";
    return x.str();
  }

  // a top-level run in the DNF form: one assignment of ORed masked compares of the run's word and opaque registers
  void emit_run(const DnfRun& rn, const std::string& ind) {
    const std::string wn = rn.wkey == kFlagsKey ? std::string("flags") : "g" + std::to_string(rn.wkey);
    bool all_cmp = true;
    std::string x;
    for (const DTerm& t : rn.terms) {
      std::string y;
      if (t.care) y = "(uint32_t)((" + wn + " & " + u(t.care) + ") == " + u(t.want) + ")";
      for (uint32_t k = 0; k < 64; k++) {
        if (t.opos >> k & 1ull) { y += std::string(y.empty() ? "" : " & ") + "b" + std::to_string(k); all_cmp = all_cmp && cmpv[k]; }
        if (t.oneg >> k & 1ull) { y += std::string(y.empty() ? "" : " & ") + "(b" + std::to_string(k) + " ^ 1u)"; all_cmp = all_cmp && cmpv[k]; }
      }
      if (y.empty()) y = "1u";
      x += std::string(x.empty() ? "" : " | ") + (rn.terms.size() > 1 && (t.opos || t.oneg) ? "(" + y + ")" : y);
    }
    if (x.empty()) x = "0u";
    *out << ind << "b" << rn.reg << " = " << x << ";\n";
    cmpv[rn.reg] = all_cmp;
  }

  // the frame the conjunction and the DNF loop share: the accumulated mask t_, and the join's other side -- invariant in the loop --
  // shifted to the id field once.  -> that other side's id ("" without a join)
  std::string open_compare_loop(const DJoin& dj, const std::string& ind) {
    *out << ind << "{ uint32_t t_ = 0u;\n";
    if (!dj.veq) return "";
    const std::string xo = vid(plan.scopes[dj.scope], var_of(dj.scope), dj.slot);
    *out << ind << "  const uint32_t xs_ = " << xo << " << " << ELEM_VID_SHIFT << "u;\n";
    return xo;
  }
  void close_compare_loop(uint32_t acc_reg, const std::string& xo, const std::string& ind) {
    // (vid_eq: id 0, "no value", equals nothing; and what does not fit the id field equals no packed id)
    if (!xo.empty()) *out << ind << "  b" << acc_reg << " = t_ & (uint32_t)((" << xo << " - 1u) < " << GK_VID_OVERFLOW << "u); }\n";
    else *out << ind << "  b" << acc_reg << " = t_; }\n";
  }
  static std::string parent_test(const std::string& w0, int pd) { return " & (uint32_t)((" + w0 + " >> 24) == e" + std::to_string(pd) + ")"; }

  // the conjunction form: one masked compare per element (word), accumulated as a wave mask
  void conjunction_loop(const FIns& loop, const Conj& cj, const std::string& ind) {
    std::ostringstream& o = *out;
    const uint32_t a = loop.a;
    const Scope& sc = plan.scopes[a];
    const int pd = parent_depth(loop);
    if (cj.never) return;
    const bool dyn = !(pre || (sc.cap <= 16 && nest_of(a) <= 4));
    const std::string xo = open_compare_loop(cj.dj, ind);
    auto term = [&](const std::string& w0name, uint32_t e_lit, bool have_lit, const std::string& evar) {
      std::string t;
      for (uint32_t k = 0; k < sc.wpe; k++) {
        if (!cj.care[k]) continue;
        std::string wk;
        if (k == 0) wk = w0name;
        else if (have_lit) wk = "acc.load(" + std::to_string(sc.word_off + e_lit * sc.wpe + k) + "u)";
        else wk = "acc.load(" + std::to_string(sc.word_off + k) + "u + " + evar + " * " + std::to_string((int)sc.wpe) + "u)";
        if (!t.empty()) t += " & ";   // (bitwise on purpose: `&&` is control flow -- a divergent branch per element)
        if (k == 0 && cj.dj.veq) t += "(uint32_t)(((" + wk + " ^ xs_) & " + u(cj.care[k]) + ") == " + u(cj.want[k]) + ")";
        else t += "(uint32_t)((" + wk + " & " + u(cj.care[k]) + ") == " + u(cj.want[k]) + ")";
      }
      if (loop.b) t += parent_test(w0name, pd);
      return t;
    };
    if (!dyn) {
      for (uint32_t e = 0; e < sc.cap; e++) {
        std::string w0name;
        const bool in_regs = pre && (sc.cap <= 8u || stack.empty());
        if (in_regs) { pre_words.insert({a, e}); w0name = "W" + std::to_string(a) + "_" + std::to_string(e); }
        else w0name = "acc.load(" + std::to_string(sc.word_off + e * sc.wpe) + "u)";
        o << ind << "  t_ |= " << term(w0name, e, true, "") << ";\n";
      }
    } else {
      o << ind << "  const uint32_t nq_ = GK_UNI(bounds[" << a << "]);\n"
        << ind << "  for (uint32_t eq_ = 0; eq_ < nq_; eq_++) { const uint32_t wq_ = acc.load(" << sc.word_off << "u + eq_ * " << (int)sc.wpe << "u); t_ |= " << term("wq_", 0, false, "eq_") << "; }\n";
    }
    close_compare_loop(loop.c, xo, ind);
  }

  // the DNF form: the terms' compares ORed per element
  void dnf_loop(const FIns& loop, const DnfLoop& dl, const std::string& ind) {
    std::ostringstream& o = *out;
    const uint32_t a = loop.a;
    const Scope& sc = plan.scopes[a];
    const int pd = parent_depth(loop);
    if (dl.terms.empty()) return;
    const std::string xo = open_compare_loop(dl.dj, ind);
    const bool in_regs = sc.cap <= 8u || stack.empty();
    for (uint32_t e = 0; e < sc.cap; e++) {
      std::string wn = "W" + std::to_string(a) + "_" + std::to_string(e), t;
      if (in_regs) pre_words.insert({a, e});
      else wn = "wq_";
      for (const DTerm& x : dl.terms) {
        if (!t.empty()) t += " | ";
        if (x.veq) t += "(uint32_t)(((" + wn + " ^ xs_) & " + u(x.care | kIdMask) + ") == " + u(x.want) + ")";
        else t += "(uint32_t)((" + wn + " & " + u(x.care) + ") == " + u(x.want) + ")";
      }
      if (loop.b) t = (dl.terms.size() > 1 ? "(" + t + ")" : t) + parent_test(wn, pd);
      if (in_regs) o << ind << "  t_ |= " << t << ";\n";
      else o << ind << "  { const uint32_t wq_ = acc.load(" << (sc.word_off + e * sc.wpe) << "u); t_ |= " << t << "; }\n";
    }
    close_compare_loop(loop.c, xo, ind);
  }

  // the first lines of an element's iteration: its word 0 (`w0`: where it comes from), presence, and the parent's ordinal
  // (`request`: a line between the two, the rolling read of a later element)
  void element_head(const FIns& loop, int d, const std::string& w0, const std::string& ind, const std::string& request = "") {
    *out << ind << "const uint32_t w" << d << " = " << w0 << ";\n" << request << ind << "uint32_t v" << d << " = w" << d << " & 1u;\n";
    if (loop.b) *out << ind << "v" << d << " = v" << d << " & (uint32_t)((w" << d << " >> 24) == e" << parent_depth(loop) << ");\n";
  }

  // the preloaded form of an element loop: every element a copy of the body; the loop's own F_ENDLOOP closes each copy (gen -> true)
  void unrolled_loop(const FIns& loop, size_t pc, size_t end, bool staged, const std::string& ind) {
    std::ostringstream& o = *out;
    const uint32_t a = loop.a;
    const Scope& sc = plan.scopes[a];
    const int d = (int)stack.size();
    const bool guarded = !(sc.cap <= 4 && nest_of(a) <= 4);   // small nests: every copy runs (absent elements hold zero words)
    if (guarded) pre_bounds.insert(a);
    parent_depth(loop);   // (open, or no text at all)
    // (a large scope under another loop is read where it is used -- one LDS read with a constant address per copy -- instead of
    //  being kept in registers across the whole run: 12 words of a volumes array pushed the kernel past its 80-VGPR budget)
    constexpr uint32_t pre_cap = 8u;   // (16: 10 spilled dwords and 0.1167 against 0.1080 ms; 4: 0.1090 -- profiles/r05_variants_g_preload.log)
    const bool in_regs = sc.cap <= pre_cap || stack.empty();
    // ROLLING reads of a scope that is read where it is used: every copy is a basic block of its own (the scalar guard), so a
    // read at the top of the copy is an exposed LDS round trip in front of half a dozen bit operations -- 36 of them in the
    // volumeMounts x volumes join of configs[2].  Two registers carry the words of the next two elements instead: copy e takes
    // its word from one of them and requests element e + 2 into it (copy e + 2 runs only when copy e did: the guards are
    // thresholds of one count).  Not when the body stores derived bits into this scope's words (a later copy must see them).
    bool roll = JitSwitches::roll() && !in_regs && sc.cap >= 3;
    // an INDEXED loop (codegen_forms.hpp index_range): the copies of the elements its body can hold for, read where they are used
    const IndexRange ir = index_range(plan, loop, pc, end);
    if (ir.restricted()) roll = false;
    if (roll) for (size_t q = pc; q < end; q = next_ins(code, q)) {
      const FIns qi = decode(code[q]);
      if (qi.op == F_STE && qi.b == a) { roll = false; break; }
    }
    const auto word_at = [&](uint32_t e) { return std::to_string(sc.word_off + e * sc.wpe) + "u"; };
    if (roll) o << ind << "{ uint32_t P" << d << "a = acc.load(" << word_at(0) << "), P" << d << "b = acc.load(" << word_at(1) << ");\n";
    for (uint32_t e = 0; e < sc.cap; e++) {
      if (e < ir.lo || e >= ir.hi) continue;   // (beyond the capacity the element is not in LDS, and the review has overflowed anyway)
      if (in_regs) pre_words.insert({a, e});
      o << ind << (guarded ? "if (" + std::to_string(e) + "u < ns" + std::to_string(a) + ") " : std::string()) << "{\n";
      o << ind << "  constexpr uint32_t e" << d << " = " << e << "u; (void)e" << d << ";\n";
      std::string w0 = "acc.load(" + word_at(e) + ")", request;
      if (in_regs) w0 = "W" + std::to_string(a) + "_" + std::to_string(e);
      else if (roll) {
        w0 = "P" + std::to_string(d) + ((e & 1u) ? "b" : "a");
        if (e + 2 < sc.cap) request = ind + "  " + w0 + " = acc.load(" + word_at(e + 2) + ");\n";
      }
      element_head(loop, d, w0, ind + "  ", request);
      stack.push_back({a, d, (int)e});
      gen(pc, end + 1, staged, ind + "  ");   // (its F_ENDLOOP pops the stack and closes the copy)
    }
    if (roll) o << ind << "}\n";
    forget_body(pc, end);   // (a copy that is skipped leaves the body's registers as they were)
  }

  // small capacities: constant trip count, fully unrolled by the compiler
  void constant_loop(const FIns& loop, const std::string& ind) {
    const int d = (int)stack.size();
    *out << ind << "{ _Pragma(\"unroll\")\n" << ind << "  for (uint32_t e" << d << " = 0; e" << d << " < " << plan.scopes[loop.a].cap << "u; e" << d << "++) {\n";
    open_body(loop, d, ind);
  }
  // run-time trip count (the wave's largest element count).  (Partial unrolling, so that the LDS reads of several iterations are in
  // flight together, measured slower in round 3: 0.127 / 0.140 against 0.122 ms.)
  // (an alias cursor: always this form, bounded by its scope's count -- not unrolled, not preloaded)
  void runtime_loop(const FIns& loop, const std::string& ind) {
    const int d = (int)stack.size();
    *out << ind << "{ const uint32_t n" << d << " = GK_UNI(bounds[" << scope_of(plan, loop.a) << "]);\n" << ind << "  for (uint32_t e" << d << " = 0; e" << d << " < n" << d << "; e" << d << "++) {\n";
    open_body(loop, d, ind);
  }
  void open_body(const FIns& loop, int d, const std::string& ind) {
    const Scope& sc = plan.scopes[loop.a];
    element_head(loop, d, "acc.load(" + u(sc.word_off) + " + e" + std::to_string(d) + " * " + u((uint32_t)(int)sc.wpe) + ")", ind + "    ");
    stack.push_back({loop.a, d, -1, pre});
  }
};

}  // namespace gk::cg
