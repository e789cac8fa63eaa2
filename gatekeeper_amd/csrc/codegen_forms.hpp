// The one-compare forms of phase 2 as pure analyses of the formula code: which loop bodies are conjunctions (with or without a value
// join), which bodies and top-level runs are short DNFs of one word's bits, and what they cost.  They read the plan and the code, and
// ask "is this cursor an open, non-alias loop" through a predicate; they write no text and keep no state.  The emitter
// (codegen_emit.hpp) and the share cut (codegen_cut.hpp) both decide through classify_loop / dnf_run.  Host only.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <map>
#include <set>

#include "formula_code.hpp"

namespace gk::cg {

// The generator's A/B switches.  The first group is read ONCE per process, each at its first use; the second on every call of
// generate_plan_source.
struct JitSwitches {
  static bool off(const char* name) { const char* v = getenv(name); return v && atoi(v) == 0; }
  static bool conj() { static const bool on = !off("GK_JIT_CONJ"); return on; }   // (A/B aid)
  static bool join() { static const bool on = !off("GK_JIT_JOIN"); return on; }   // (A/B aid: 0 = the text of before at sweep geometry too)
  static bool dnf() { static const bool on = !off("GK_JIT_DNF"); return on; }     // (A/B aid: 0 = the text of before at sweep geometry too)
  static bool roll() { static const bool on = !off("GK_JIT_ROLL"); return on; }   // (A/B aid)
  // (4 since round 6: at the 64-VGPR budget of four row groups per CU, and with the formulas running below the other phases'
  //  priority, short runs win -- 10 M objects 0.432 -> 0.417 ms, configs[2] 0.0470 -> 0.0462, the corpus level; 16 before:
  //  profiles/r06_variants_ae_*.log)
  static size_t pre_live() { static const size_t n = getenv("GK_JIT_PRE_LIVE") ? (size_t)std::max(1, atoi(getenv("GK_JIT_PRE_LIVE"))) : 4; return n; }   // (tuning aid, read once)
  bool preload = !off("GK_JIT_PRELOAD");
  bool res_lanes = !off("GK_JIT_RES_LANES");
  bool conj_now = !off("GK_JIT_CONJ");   // (the share cut's price of the DNF form asks on every call)
};

// the scope table is indexed by CURSOR (cursors.hpp): an alias cursor walks an element scope a second time
inline uint32_t scope_of(const HostPlan& plan, uint32_t cursor) { return cursor < plan.cursor_scope.size() ? plan.cursor_scope[cursor] : cursor; }
inline bool is_alias(const HostPlan& plan, uint32_t cursor) { return cursor >= plan.n_real_scopes; }
using OpenLoop = std::function<bool(uint32_t)>;   // is this cursor's loop open around the instruction

// CONJUNCTION bodies (round 5).  Most loops of a compiled policy set ask "does SOME element hold bits b1 & b2 & !b3 .." -- a
// conjunction of literals of the element's own words (after the string tests became dictionary bits nearly every container loop
// of the 200-template corpus has that shape).  Evaluated bit by bit that is an extract per literal, a combine per literal and two
// operations to accumulate, per element; as ONE masked compare per element word -- (w & care) == want, the element's presence bit
// among the literals, so that the zero word of an absent element fails by itself -- it is two vector operations and a scalar OR.
// -> care / want per word of the element (index = word), false when the body is anything but such a conjunction.
// JOIN bodies (sweep geometry, `join_ok`).  A value join -- "some volume is present, not of kind k, and NAMED as this mount names its
// volume" -- is such a conjunction but for one literal: an equality of value ids (F_VEQ) between the id packed into THIS loop's element
// word and a value that does not change inside the loop (a slot of an enclosing loop's element).  With X the outer id,
//   ((w ^ (X << ELEM_VID_SHIFT)) & (care | idmask << ELEM_VID_SHIFT)) == want
// tests the literals and the sixteen id bits in one compare: three vector operations per pair instead of nine.  vid_eq is false for
// id 0: equal ids are both zero or neither, so that half is ONE test of X per outer element, ANDed into the finished mask (`veq`:
// the other side of the equality).  Bits of the word above the id field (the parent ordinal) are outside the mask.
struct DJoin { bool veq = false; uint32_t scope = 0, slot = 0; };   // a body's one equality: its other side
struct Conj { std::vector<uint32_t> care, want; bool never = false; DJoin dj; };
constexpr uint32_t kVeqLit = ~0u;   // the equality among a body's literals (never negated: its negation is no masked compare)
constexpr uint32_t kIdMask = GK_VID_OVERFLOW << ELEM_VID_SHIFT;

// the one equality a join body may hold: exactly one side is this loop's element, whose id is packed into its word; the other an
// element loop that is open around this one (not a cursor of a self-join).  -> the other side, false: not such an equality
inline bool join_side(const HostPlan& plan, uint32_t scope, const SlotWord& s, const OpenLoop& open, DJoin* out) {
  if (out->veq || (s.sa == scope) == (s.sb == scope)) return false;
  const uint32_t so = s.sa == scope ? s.sb : s.sa;
  if (!scope_packed(plan.scopes[scope]) || is_alias(plan, so) || !open(so)) return false;
  out->veq = true; out->scope = so; out->slot = s.sa == scope ? s.lb : s.la;
  return true;
}

inline bool conj_body(const HostPlan& plan, uint32_t scope, size_t pc, size_t end, uint32_t result_reg, bool join_ok, const OpenLoop& open, Conj* out) {
  const std::vector<uint32_t>& code = plan.code;
  struct Lit { uint32_t bit; bool pos; };
  struct Val { int kind = 0; std::vector<Lit> lits; };   // kind 0: unknown, 1: conjunction of lits, 2: constant false, 3: constant true
  std::map<uint32_t, Val> regs;
  auto conj_and = [&](const Val& x, const Val& y) -> Val {
    Val r;
    if (x.kind == 0 || y.kind == 0) return r;
    if (x.kind == 2 || y.kind == 2) { r.kind = 2; return r; }
    if (x.kind == 3) return y;
    if (y.kind == 3) return x;
    r.kind = 1; r.lits = x.lits;
    for (const Lit& l : y.lits) {
      bool dup = false;
      for (const Lit& m : r.lits) if (m.bit == l.bit) { if (m.pos != l.pos) { r.kind = 2; r.lits.clear(); return r; } dup = true; }
      if (!dup) r.lits.push_back(l);
    }
    return r;
  };
  auto neg = [&](const Val& x) -> Val {
    Val r;
    if (x.kind == 2) r.kind = 3; else if (x.kind == 3) r.kind = 2;
    else if (x.kind == 1 && x.lits.size() == 1 && x.lits[0].bit != kVeqLit) { r.kind = 1; r.lits = {Lit{x.lits[0].bit, !x.lits[0].pos}}; }
    return r;
  };
  for (; pc < end; pc = next_ins(code, pc)) {
    const FIns i = decode(code[pc]);
    switch (i.op) {
      case F_LDE: { if (i.b != scope) return false; Val v; v.kind = 1; v.lits = {Lit{i.c, true}}; regs[i.a] = v; break; }
      case F_AND: regs[i.a] = conj_and(regs[i.b], regs[i.c]); break;
      case F_ANDN: regs[i.a] = conj_and(regs[i.b], neg(regs[i.c])); break;
      case F_NOT: regs[i.a] = neg(regs[i.b]); break;
      case F_MOV: regs[i.a] = regs[i.b]; break;
      case F_CONST: { Val v; v.kind = (i.b & 1) ? 3 : 2; regs[i.a] = v; break; }
      case F_VEQ: {
        if (!join_ok || !join_side(plan, scope, decode_slots(code[pc + 1]), open, &out->dj)) return false;
        Val v; v.kind = 1; v.lits = {Lit{kVeqLit, true}}; regs[i.a] = v;
        break;
      }
      default: return false;   // a nested loop, a join, a derived bit, a global / flag bit, a disjunction: the general form
    }
    if (regs[i.a].kind == 0) return false;
  }
  const Val& body = regs[result_reg];
  if (body.kind == 0) return false;
  const Scope& sc = plan.scopes[scope];
  out->care.assign(sc.wpe, 0u); out->want.assign(sc.wpe, 0u);
  out->care[0] = 1u; out->want[0] = 1u;   // the element is present
  if (body.kind == 2) { out->never = true; return true; }
  bool veq_used = false;
  if (body.kind == 1) for (const Lit& l : body.lits) {
    if (l.bit == kVeqLit) { veq_used = true; continue; }
    const uint32_t w = elem_word_of_bit(l.bit), m = elem_mask_of_bit(l.bit);
    if (w >= sc.wpe) return false;
    if ((out->care[w] & m) && (((out->want[w] & m) != 0) != l.pos)) { out->never = true; return true; }
    out->care[w] |= m;
    if (l.pos) out->want[w] |= m;
  }
  out->dj.veq = veq_used;   // (an equality the result does not depend on is dropped with the rest of the dead code)
  if (veq_used) {
    if (out->care[0] & kIdMask) return false;   // (a predicate bit inside the id field: not a layout this form knows)
    out->care[0] |= kIdMask;
  }
  return true;
}

// DNF form (sweep geometry, `dnf_ok`).  What conj_body refuses because of a disjunction -- "a container that drops none of the
// capabilities, or adds one": bit1 & !(bit2 & !bit3 & !bit4) -- and the top-level formulas over the bits of ONE word (a global
// predicate word g<k>, or the review flags) are short disjunctions of conjunctions of literals of that word: each term one masked
// compare (w & care) == want, the terms ORed.  The compiler keeps compare results as wave masks, so the ORs are scalar operations; and
// a value built of compares only has no higher bits, so its test needs no opaque copy (GK_BIT: FormulaEmitter::cmpv).  A term may also
// hold registers the run did not compute -- finished loop results -- as opaque literals (`opos` / `oneg`: ANDed outside the compare),
// and, in a loop body, the body's one value-id equality (`veq`: the join form's xor, in every term or in none).
struct DTerm { uint32_t care = 0, want = 0; uint64_t opos = 0, oneg = 0; bool veq = false; };
struct DVal { bool ok = false; std::vector<DTerm> t; };   // ok: known | no term: false | a term without literals: true
constexpr size_t kDnfCap = 8;   // terms a value may have, intermediate values included (a cap of 4 refuses "bit1 and one of five", twice in configs[2])
inline bool d_implies(const DTerm& y, const DTerm& x) {   // every literal of x is a literal of y: y | x == x
  return (x.care & ~y.care) == 0 && ((y.want ^ x.want) & x.care) == 0 && (x.opos & ~y.opos) == 0 && (x.oneg & ~y.oneg) == 0 && (!x.veq || y.veq);
}
inline bool d_norm(DVal* v) {   // duplicates merged, absorbed terms dropped; false: more terms than the cap
  std::vector<DTerm> out;
  for (const DTerm& y : v->t) {
    bool drop = false;
    for (const DTerm& x : out) if (d_implies(y, x)) { drop = true; break; }
    if (drop) continue;
    out.erase(std::remove_if(out.begin(), out.end(), [&](const DTerm& x) { return d_implies(x, y); }), out.end());
    out.push_back(y);
  }
  v->t.swap(out);
  if (v->t.size() > kDnfCap) { v->ok = false; v->t.clear(); }
  return v->ok;
}
inline DVal d_or(const DVal& x, const DVal& y) {
  DVal r;
  if (!x.ok || !y.ok) return r;
  r.ok = true; r.t = x.t; r.t.insert(r.t.end(), y.t.begin(), y.t.end());
  d_norm(&r);
  return r;
}
inline DVal d_and(const DVal& x, const DVal& y) {
  DVal r;
  if (!x.ok || !y.ok) return r;
  r.ok = true;
  for (const DTerm& p : x.t) for (const DTerm& q : y.t) {
    if (((p.want ^ q.want) & p.care & q.care) || (p.opos & q.oneg) || (p.oneg & q.opos)) continue;   // a contradictory term
    DTerm m;
    m.care = p.care | q.care; m.want = p.want | q.want; m.opos = p.opos | q.opos; m.oneg = p.oneg | q.oneg; m.veq = p.veq || q.veq;
    r.t.push_back(m);
    if (r.t.size() > 4 * kDnfCap && !d_norm(&r)) return r;
  }
  d_norm(&r);
  return r;
}
inline DVal d_not(const DVal& x) {   // De Morgan: the product over the terms of "one of its literals fails"
  DVal r;
  if (!x.ok) return r;
  r.ok = true; r.t.push_back(DTerm{});
  for (const DTerm& p : x.t) {
    DVal alt; alt.ok = true;
    if (p.veq) return DVal{};   // (the negation of an equality of ids is no masked compare)
    for (uint32_t k = 0; k < 32; k++) if (p.care >> k & 1u) { DTerm l; l.care = 1u << k; l.want = ~p.want & (1u << k); alt.t.push_back(l); }
    for (uint32_t k = 0; k < 64; k++) {
      if (p.opos >> k & 1ull) { DTerm l; l.oneg = 1ull << k; alt.t.push_back(l); }
      if (p.oneg >> k & 1ull) { DTerm l; l.opos = 1ull << k; alt.t.push_back(l); }
    }
    r = d_and(r, alt);
    if (!r.ok) return r;
  }
  return r;
}
// the straight-line instructions [pc, end) over literals of one word -> the value of every register.  loop_scope >= 0: a loop body
// (literals: bits of word 0 of that loop's element; `join`: one value-id equality allowed, its other side an open loop's element --
// `open`); -1: a top-level run (literals: bits of one global word or of the flags -- *wkey: which, -1 none yet; registers read before
// the run writes them are opaque literals).  *bitops: what the same instructions cost bit by bit (an extract / a connective: 1)
constexpr int kFlagsKey = 1 << 20;
inline bool dnf_eval(const HostPlan& plan, int loop_scope, size_t pc, size_t end, bool join, const OpenLoop& open, std::map<uint32_t, DVal>* regs,
                     int* wkey, DJoin* dj, uint32_t* bitops) {
  const std::vector<uint32_t>& code = plan.code;
  const auto rd = [&](uint32_t r) -> DVal {
    auto it = regs->find(r);
    if (it != regs->end()) return it->second;
    DVal v;
    if (loop_scope < 0 && r < 64) { v.ok = true; DTerm l; l.opos = 1ull << r; v.t.push_back(l); }
    return v;
  };
  const auto lit = [&](int key, uint32_t mask) -> DVal {
    DVal v;
    if (*wkey >= 0 && *wkey != key) return v;
    *wkey = key;
    v.ok = true; DTerm l; l.care = mask; l.want = mask; v.t.push_back(l);
    return v;
  };
  for (; pc < end; pc = next_ins(code, pc)) {
    const FIns i = decode(code[pc]);
    DVal v;
    switch (i.op) {
      case F_LDG: if (loop_scope >= 0) return false; v = lit((int)(global_bit(i) >> 5), 1u << (global_bit(i) & 31)); break;
      case F_LDF: if (loop_scope >= 0 || i.b >= 32) return false; v = lit(kFlagsKey, 1u << i.b); break;
      case F_LDE: if (loop_scope < 0 || i.b != (uint32_t)loop_scope || elem_word_of_bit(i.c) != 0) return false; v = lit(0, elem_mask_of_bit(i.c)); break;
      case F_AND: v = d_and(rd(i.b), rd(i.c)); break;
      case F_OR: v = d_or(rd(i.b), rd(i.c)); break;
      case F_ANDN: v = d_and(rd(i.b), d_not(rd(i.c))); break;
      case F_NOT: v = d_not(rd(i.b)); break;
      case F_MOV: v = rd(i.b); (*bitops)--; break;
      case F_CONST: v.ok = true; if (i.b & 1) v.t.push_back(DTerm{}); (*bitops)--; break;
      case F_VEQ: {
        if (loop_scope < 0 || !join || !join_side(plan, (uint32_t)loop_scope, decode_slots(code[pc + 1]), open, dj)) return false;
        v.ok = true; DTerm l; l.veq = true; v.t.push_back(l);
        (*bitops) += 8;   // (an extract, two compares and three combines, and the other side's extract, as the share cut counts them)
        break;
      }
      default: return false;
    }
    (*bitops)++;
    if (!v.ok) return false;
    (*regs)[i.a] = v;
  }
  return true;
}
inline uint32_t dnf_cost(const std::vector<DTerm>& t) {   // operations of the form: 2 per compare (3 with the join's xor), the opaque literals' ANDs and negations, the ORs
  uint32_t n = 0;
  for (const DTerm& x : t) n += ((x.care || x.veq) ? (x.veq ? 3u : 2u) : 0u) + (uint32_t)__builtin_popcountll(x.opos) + 2u * (uint32_t)__builtin_popcountll(x.oneg);
  return n + (t.empty() ? 0u : (uint32_t)t.size() - 1u);
}
// a loop body as a DNF of the loop's element word 0, the presence bit in every term.  false: not such a body, or no cheaper than bit by bit
struct DnfLoop { std::vector<DTerm> terms; DJoin dj; uint32_t cost = 0; };
inline bool dnf_body(const HostPlan& plan, uint32_t scope, size_t pc, size_t end, uint32_t result_reg, bool join, const OpenLoop& open, DnfLoop* out) {
  std::map<uint32_t, DVal> regs;
  int wkey = -1;
  uint32_t bitops = 0;
  if (plan.scopes[scope].wpe == 0 || !dnf_eval(plan, (int)scope, pc, end, join, open, &regs, &wkey, &out->dj, &bitops)) return false;
  auto it = regs.find(result_reg);
  if (it == regs.end() || !it->second.ok) return false;
  DVal present; present.ok = true; { DTerm l; l.care = 1u; l.want = 1u; present.t.push_back(l); }
  const DVal body = d_and(it->second, present);
  if (!body.ok) return false;
  size_t n_veq = 0;
  for (const DTerm& x : body.t) { if (x.veq) n_veq++; if (out->dj.veq && (x.care & kIdMask)) return false; }
  if (n_veq != 0 && n_veq != body.t.size()) return false;   // (the id-0 test of the join is one AND behind the ORs: the equality is in every term or in none)
  out->dj.veq = n_veq != 0;
  out->terms = body.t;
  out->cost = dnf_cost(body.t);
  return out->cost < bitops;
}
// a top-level run: the straight-line instructions from pc up to the first F_RES / F_STG, over the bits of one word and opaque
// registers; every register it writes but the result is dead behind it (to the end of the block).  -> the index of that F_RES / F_STG
struct DnfRun { std::vector<DTerm> terms; int wkey = -1; size_t at = 0; uint32_t reg = 0, cost = 0; };
inline bool dnf_run(const HostPlan& plan, size_t pc, size_t pc1, DnfRun* out) {
  const std::vector<uint32_t>& code = plan.code;
  size_t q = pc;
  for (; q < pc1; q++) {
    const uint32_t qop = code[q] & 0xFF;
    if (qop == F_RES || qop == F_STG) break;
    if (qop != F_LDG && qop != F_LDF && qop != F_AND && qop != F_OR && qop != F_ANDN && qop != F_NOT && qop != F_MOV && qop != F_CONST) return false;
  }
  if (q >= pc1 || q == pc) return false;
  std::map<uint32_t, DVal> regs;
  DJoin dj;
  uint32_t bitops = 0;
  out->wkey = -1;
  if (!dnf_eval(plan, -1, pc, q, false, [](uint32_t) { return false; }, &regs, &out->wkey, &dj, &bitops)) return false;
  out->at = q; out->reg = decode(code[q]).a;
  auto it = regs.find(out->reg);
  if (it == regs.end() || !it->second.ok || out->wkey < 0) return false;
  // liveness: a register the run writes, other than its result, that is read behind the run before it is written again: the general form.
  // The scan is linear to the end of the block and takes a write inside a later loop body for a write.  That rests on two properties of
  // the formula code (lower.cpp): a block is self-contained -- no register is carried from one block into another, only derived bits
  // through F_STE / F_STG -- and a register is only read where every path to the read has written it (a loop's body registers are
  // written in the body before they are read there; behind the loop only its accumulators, written by F_LOOP itself, are read).  So a
  // read behind a copy or a loop that did not run never looks for a value of before the loop, the run's temporaries least of all.
  std::set<uint32_t> pending;
  for (auto& kv : regs) if (kv.first != out->reg) pending.insert(kv.first);   // (the result register is assigned by the form)
  for (size_t r = q + 1; r < pc1 && !pending.empty(); r = next_ins(code, r)) {
    const FIns i = decode(code[r]);
    if (i.op == F_END) break;
    const RegUse use = reg_use(i);
    if (!use.known) return false;
    for (uint32_t x : use.reads) if (pending.count(x)) return false;
    for (uint32_t x : use.writes) pending.erase(x);
  }
  out->terms = it->second.t;
  out->cost = dnf_cost(out->terms);
  return out->cost < bitops;
}

// a loop both one-compare forms can take at all: an element loop (no alias cursor) of at most 16 elements that ends in a plain F_ENDLOOP on its own accumulator
inline bool form_loop(const HostPlan& plan, uint32_t scope, uint32_t acc_reg, size_t end) {
  const FIns e = decode(plan.code[end]);
  return !is_alias(plan, scope) && e.op == F_ENDLOOP && e.a == acc_reg && plan.scopes[scope].cap <= 16;
}

// THE place that decides a loop's form.  loop: the F_LOOP; [pc, end): its body, code[end] its end.  conj_on: GK_JIT_CONJ | join_ok: a
// body may hold one value-id equality | dnf_ok: what conj_body refuses may be a DNF.  The emitter and the share cut both ask here; what
// each passes is written down at its call.
enum class LoopForm { General, Conjunction, Dnf };
struct LoopClass { LoopForm form = LoopForm::General; Conj cj; DnfLoop dl; };
inline LoopClass classify_loop(const HostPlan& plan, const FIns& loop, size_t pc, size_t end, bool conj_on, bool join_ok, bool dnf_ok, const OpenLoop& open) {
  LoopClass lc;
  if (!conj_on || !form_loop(plan, loop.a, loop.c, end)) return lc;
  const uint32_t body_reg = decode(plan.code[end]).b;
  if (conj_body(plan, loop.a, pc, end, body_reg, join_ok, open, &lc.cj)) lc.form = LoopForm::Conjunction;
  else if (dnf_ok && dnf_body(plan, loop.a, pc, end, body_reg, join_ok, open, &lc.dl)) lc.form = LoopForm::Dnf;
  return lc;
}

// INDEXED loops.  `cs[0]` is an iteration whose body's top-level conjunction ties the loop's own ordinal to a constant (F_KIMM ==, < or
// <= on the loop's primary cursor, cursors.hpp): every other element fails the body whatever it holds.  In the unrolled form only the
// copies of the elements [lo, hi) are written -- one copy for `== k` -- where the general form writes one per element of the capacity.
// Sound because a skipped copy would add nothing: its body is false, so F_ENDLOOP / F_ENDLOOP2 accumulate nothing, and a body that
// stores a derived bit or a result (F_STE / F_STG / F_RES) is declined.  `!=`, `>`, `>=`, F_KEND (the count is the lane's own) and alias
// cursors keep every copy.  The conjunction, join and DNF forms decline a body that holds one of these ops (conj_body / dnf_eval).
struct IndexRange { uint32_t lo = 0, hi = ~0u; bool restricted() const { return lo != 0 || hi != ~0u; } };
inline IndexRange index_range(const HostPlan& plan, const FIns& loop, size_t pc, size_t end) {
  IndexRange r;
  const std::vector<uint32_t>& code = plan.code;
  if (is_alias(plan, loop.a)) return r;
  bool has = false;
  struct At { size_t pc; int depth; };
  std::vector<At> ins;
  int depth = 0;
  for (size_t q = pc; q < end; q = next_ins(code, q)) {
    const uint32_t op = code[q] & 0xFF;
    if (op == F_STE || op == F_STG || op == F_RES) return r;
    if (op == F_ENDLOOP || op == F_ENDLOOP2) depth--;
    ins.push_back({q, depth});
    if (op == F_LOOP) depth++;
    if (is_kimm(op)) has = true;
  }
  if (!has) return r;
  // the conjuncts of register `reg` as it stands in front of instruction index `before`: through the ANDs and moves of the body's top level
  const std::function<void(uint32_t, size_t)> visit = [&](uint32_t reg, size_t before) {
    for (size_t k = before; k-- > 0;) {
      const FIns i = decode(code[ins[k].pc]);
      const RegUse use = reg_use(i);
      if (std::find(use.writes.begin(), use.writes.end(), reg) == use.writes.end()) continue;
      if (ins[k].depth != 0 || i.op == F_LOOP) return;   // (the result of a nested loop: a conjunct of its own)
      if (i.op == F_AND) { visit(i.b, k); visit(i.c, k); }
      else if (i.op == F_MOV) visit(i.b, k);
      else if (is_kimm(i.op) && i.b == loop.a) {
        const uint32_t rel = i.op - F_KIMM;
        if (rel == C_EQ) { r.lo = std::max(r.lo, i.c); r.hi = std::min(r.hi, i.c + 1u); }
        else if (rel == C_LT) r.hi = std::min(r.hi, i.c);
        else if (rel == C_LE) r.hi = std::min(r.hi, i.c + 1u);
      }
      return;
    }
  };
  visit(decode(code[end]).b, ins.size());
  return r;
}
// copies of a loop's body in the unrolled form
inline uint32_t unrolled_copies(const HostPlan& plan, const FIns& loop, size_t pc, size_t end) {
  const uint32_t cap = plan.scopes[loop.a].cap;
  const IndexRange r = index_range(plan, loop, pc, end);
  const uint32_t hi = std::min(r.hi, cap);
  return r.lo < hi ? hi - r.lo : 0u;
}

// The share cut's own, LOOSER recogniser of a join body (it sets the scan's `join_until`): a plain loop over a packed scope whose body is
// own-word literals, connectives and exactly one F_VEQ.  It does not look at the equality's sides -- whether one is this loop's element
// and the other an open loop's -- and so takes a few bodies conj_body refuses; their F_VEQ is then priced as part of the element's one
// compare all the same.
inline bool loose_join_body(const HostPlan& plan, uint32_t cursor, size_t pc, size_t end) {
  const std::vector<uint32_t>& code = plan.code;
  if (is_alias(plan, cursor) || (code[end] & 0xFF) != F_ENDLOOP || !scope_packed(plan.scopes[cursor])) return false;
  size_t n_veq = 0;
  for (size_t q = pc; q < end; q = next_ins(code, q)) {
    const uint32_t qop = code[q] & 0xFF;
    if (qop == F_VEQ) n_veq++;
    else if (qop != F_LDE && qop != F_AND && qop != F_ANDN && qop != F_NOT && qop != F_MOV && qop != F_CONST) return false;   // (an ordering relation among them: the general form)
  }
  return n_veq == 1;
}

}  // namespace gk::cg
