// The SHARE CUT of phase 2: the formulas cut into self-contained blocks and dealt to the waves that share one 64-review half.  Blocks of
// one STAGE are independent (they only read bits written by earlier stages); part = stage * NW + wave-within-half.  A pure function of
// the plan, the geometry and the switches: it prices blocks, orders them by their derived bits, places and balances them, and decides
// whether the parts are generated in the unrolled, preloaded form.  It emits nothing.  Host only.
#pragma once
#include "codegen_forms.hpp"

namespace gk::cg {

struct Blk { size_t pc0, pc1; uint32_t stage; uint64_t cost; std::vector<uint64_t> writes, reads; };
struct FormulaCut { std::vector<Blk> blks; std::vector<std::vector<size_t>> parts; uint32_t n_stages = 0; bool use_pre = false; };

constexpr uint64_t kLoopWeight = 3;   // cost of a loop body relative to straight-line code

// cost, derived-bit reads / writes and stage of every block
inline std::vector<Blk> price_blocks(const HostPlan& plan, bool sweep, const JitSwitches& sw) {
  const std::vector<uint32_t>& code = plan.code;
  std::vector<Blk> blks;
  size_t prev = 0;
  for (uint32_t e : plan.seg_ends) { blks.push_back({prev, e, 0, 0, {}, {}}); prev = e; }
  const bool join_cost = JitSwitches::join() && sweep && sw.preload;
  size_t join_until = 0;   // end of the join-form body the scan is in
  // ... and a run or a body that takes the DNF form costs its compares and ORs: the instructions it replaces are free (`free_until`).
  // The scan asks classify_loop / dnf_run, as the emitter will, over a loop stack of its own.  What it passes differs from what the emitter
  // passes, on purpose or at least with the generated text resting on it:
  //  - the cut is made before `use_pre` is known, so it prices the forms whether or not the parts will be unrolled.  A plan whose unrolled
  //    text exceeds `pre_budget` keeps its loops, takes neither form, and is then cut with the forms' prices -- a balance a little off,
  //    never a wrong result.  (The plans in the tree -- configs[1], [2] and the one-plan corpus -- are all within the budget.)
  //  - join_ok is TRUE whatever GK_JIT_JOIN says (the emitter: the switch, at sweep geometry, in the unrolled form)
  //  - its stack entries carry the literal element 0 and the scan's own depth (no analysis reads either: `open` asks for the cursor alone)
  //  - `rs`, the emitter's run_start, becomes true behind a loop closed at depth 1 -- read before the scan pops its stack
  const bool dnf_price = JitSwitches::dnf() && join_cost && sw.conj_now;
  size_t free_until = 0;
  std::map<uint64_t, size_t> writer;   // derived bit -> block
  std::vector<uint32_t> stack;         // the cursors of the open loops
  std::vector<uint64_t> wstack;        // the weight each open loop multiplied the body's cost by
  const OpenLoop open = [&](uint32_t cursor) { return std::find(stack.begin(), stack.end(), cursor) != stack.end(); };
  for (size_t bi = 0; bi < blks.size(); bi++) {
    Blk& B = blks[bi];
    uint64_t weight = 1;
    bool rs = true;   // a run starts at the block's first instruction, behind F_RES / F_STG and behind a loop, at top level
    stack.clear(); wstack.clear();
    for (size_t pc = B.pc0; pc < B.pc1;) {
      const FIns i = decode(code[pc++]);
      const uint32_t op = i.op;
      const bool loop_close = op == F_ENDLOOP || op == F_ENDLOOP2;
      if (dnf_price && stack.empty() && rs && pc > free_until) {
        DnfRun rn;
        if (dnf_run(plan, pc - 1, B.pc1, &rn)) { B.cost += rn.cost; free_until = rn.at; }
      }
      rs = false;
      if (dnf_price && (op == F_RES || op == F_STG || loop_close)) rs = stack.size() <= (loop_close ? 1u : 0u);
      if (dnf_price && op == F_LOOP) {
        const size_t end = loop_end(code, pc);
        if (pc > free_until) {
          const LoopClass lc = classify_loop(plan, i, pc, end, /*conj_on (in dnf_price)*/ true, /*join_ok*/ true, /*dnf_ok*/ true, open);
          if (lc.form == LoopForm::Dnf) { B.cost += (uint64_t)lc.dl.cost * weight * kLoopWeight; free_until = end; }
        }
        stack.push_back(i.a);
      }
      if (dnf_price && loop_close && !stack.empty()) stack.pop_back();
      const bool paid = pc <= free_until && op != F_LOOP && !loop_close;   // part of a form that is already paid for
      if (paid) { if (has_slot_word(op)) pc++; }
      else if (has_slot_word(op)) { pc++; B.cost += (op == F_VEQ && pc < join_until ? 2 : 12) * weight; }   // (in a join-form body: part of the element's one compare)
      else if (op == F_LOOP) {
        // (an INDEXED loop -- `cs[0]`, codegen_forms.hpp index_range -- is one copy of its body: straight-line code)
        const size_t body_end = loop_end(code, pc);
        const uint64_t mult = sw.preload && index_range(plan, i, pc, body_end).restricted() && unrolled_copies(plan, i, pc, body_end) <= 1u ? 1 : kLoopWeight;
        B.cost += 4 * weight; weight *= mult; wstack.push_back(mult);
        // the share cut at sweep geometry gives a join its real cost: a body of own-word literals and one equality becomes one masked
        // compare per element (conj_body), where the general form pays an extract, two compares and three combines for the equality
        if (join_cost) { const size_t end = loop_end(code, pc); if (loose_join_body(plan, i.a, pc, end)) join_until = end; }
      }
      else if (loop_close) { weight /= wstack.empty() ? kLoopWeight : wstack.back(); if (!wstack.empty()) wstack.pop_back(); B.cost += (op == F_ENDLOOP2 ? 2 : 1) * weight; }
      else B.cost += weight;
      if (op == F_STG) B.writes.push_back(1ull << 40 | global_bit(i));
      if (op == F_STE) B.writes.push_back(2ull << 40 | (uint64_t)scope_of(plan, i.b) << 16 | i.c);   // (derived element bits belong to the scope, whichever cursor reads them)
      if (op == F_LDG) B.reads.push_back(1ull << 40 | global_bit(i));
      if (op == F_LDE) B.reads.push_back(2ull << 40 | (uint64_t)scope_of(plan, i.b) << 16 | i.c);
    }
    for (uint64_t r : B.reads) { auto it = writer.find(r); if (it != writer.end() && it->second != bi) B.stage = std::max(B.stage, blks[it->second].stage + 1); }
    for (uint64_t w : B.writes) writer[w] = bi;
  }
  return blks;
}

inline uint32_t lightest(const std::vector<uint64_t>& load) {
  uint32_t w = 0;
  for (uint32_t k = 1; k < load.size(); k++) if (load[k] < load[w]) w = k;
  return w;
}
// block ids, heaviest first (ties in block order)
inline void by_cost(const std::vector<Blk>& blks, std::vector<size_t>* ids) {
  std::stable_sort(ids->begin(), ids->end(), [&](size_t x, size_t y) { return blks[x].cost > blks[y].cost; });
}

// CHAINS (round 3).  A block of a later stage only waits for the blocks that write the derived bits it reads.  When those
// run on the SAME wave, program order is all it needs (lane = review in every block: a wave reads back what its own lanes
// OR-ed into LDS): such a block is appended to its producers' share of stage 0.  Producers that sit in another share
// are DUPLICATED into this one when they are cheap (derived bits are ORs: writing one twice is harmless).  If every later
// block can be placed that way the formulas take ONE stage -- one barrier and one call per item instead of one per level
// of derived bits (configs[2]: three stages, the last two a dozen lines each, profiles/r03_*).  Otherwise: stages as before.
// -> false: not every block could be placed
inline bool chain_blocks(const std::vector<Blk>& blks, uint32_t NW, std::vector<std::vector<size_t>>* parts) {
  std::vector<std::vector<size_t>> deps(blks.size());   // direct producers
  {
    std::map<uint64_t, size_t> w2;
    for (size_t bi = 0; bi < blks.size(); bi++) {
      for (uint64_t r : blks[bi].reads) { auto it = w2.find(r); if (it != w2.end() && it->second != bi) deps[bi].push_back(it->second); }
      for (uint64_t w : blks[bi].writes) w2[w] = bi;
    }
  }
  std::vector<std::vector<size_t>> closure(blks.size());   // transitive producers, ascending
  for (size_t bi = 0; bi < blks.size(); bi++) {
    std::vector<size_t> c;
    for (size_t d : deps[bi]) { c.push_back(d); c.insert(c.end(), closure[d].begin(), closure[d].end()); }
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    closure[bi] = c;
  }
  std::vector<std::vector<bool>> in_part(NW, std::vector<bool>(blks.size(), false));
  std::vector<uint64_t> load(NW, 0);
  uint64_t total = 0, dup_total = 0;
  for (auto& B : blks) total += B.cost;
  bool chained = false;
  // (a) FAMILIES: blocks connected by derived bits go to one share as a whole (no duplicates), heaviest family to the
  //     lightest share -- as long as no family outweighs a fair share by much
  {
    std::vector<size_t> root(blks.size());
    for (size_t i = 0; i < blks.size(); i++) root[i] = i;
    auto find = [&](size_t x) { while (root[x] != x) x = root[x] = root[root[x]]; return x; };
    for (size_t bi = 0; bi < blks.size(); bi++) for (size_t d : deps[bi]) root[find(bi)] = find(d);
    std::map<size_t, uint64_t> fam_cost;
    for (size_t bi = 0; bi < blks.size(); bi++) fam_cost[find(bi)] += blks[bi].cost;
    uint64_t biggest = 0;
    for (auto& kv : fam_cost) biggest = std::max(biggest, kv.second);
    if (biggest * NW <= total + total / 8) {
      std::vector<size_t> fams;
      for (auto& kv : fam_cost) fams.push_back(kv.first);
      std::stable_sort(fams.begin(), fams.end(), [&](size_t x, size_t y) { return fam_cost[x] > fam_cost[y]; });
      for (size_t f : fams) {
        const uint32_t w = lightest(load);
        load[w] += fam_cost[f];
        for (size_t bi = 0; bi < blks.size(); bi++) if (find(bi) == f) in_part[w][bi] = true;
      }
      chained = true;
    }
  }
  // (b) a family too heavy for one share: stage-0 blocks dealt as the staged form deals them; a later block joins the share
  //     that holds most of its producers, the missing ones are duplicated if that is cheap
  if (!chained) {
    std::vector<size_t> ids;
    for (size_t bi = 0; bi < blks.size(); bi++) if (blks[bi].stage == 0) ids.push_back(bi);
    by_cost(blks, &ids);
    for (size_t bi : ids) {
      const uint32_t w = lightest(load);
      load[w] += blks[bi].cost;
      in_part[w][bi] = true;
    }
    const uint64_t dup_max = std::max<uint64_t>(64, total / NW / 8);   // duplicated cost allowed per block
    chained = true;
    for (size_t bi = 0; bi < blks.size() && chained; bi++) {
      if (blks[bi].stage == 0) continue;
      uint32_t best = NW;
      uint64_t best_extra = 0;
      for (uint32_t k = 0; k < NW; k++) {
        uint64_t extra = 0;
        for (size_t d : closure[bi]) if (!in_part[k][d]) extra += blks[d].cost;
        if (extra > dup_max) continue;
        if (best == NW || extra + load[k] < best_extra + load[best]) { best = k; best_extra = extra; }
      }
      if (best == NW) { chained = false; break; }
      for (size_t d : closure[bi]) in_part[best][d] = true;
      in_part[best][bi] = true;
      load[best] += best_extra + blks[bi].cost;
      dup_total += best_extra;
    }
    if (chained && dup_total > total / 4) chained = false;   // (duplicates are work done twice)
  }
  if (chained) {
    parts->assign(NW, {});
    for (uint32_t k = 0; k < NW; k++) for (size_t bi = 0; bi < blks.size(); bi++) if (in_part[k][bi]) (*parts)[k].push_back(bi);
  }
  return chained;
}

// operations of [pc, pc1) after unrolling every loop by its scope's capacity
inline uint64_t unrolled_ops(const HostPlan& plan, size_t pc, size_t pc1) {
  uint64_t n = 0;
  while (pc < pc1) {
    const FIns i = decode(plan.code[pc]);
    if (has_slot_word(i.op)) { pc += 2; n += 2; continue; }
    if (i.op == F_LOOP) { const size_t end = loop_end(plan.code, pc + 1); n += (uint64_t)unrolled_copies(plan, i, pc + 1, end) * (4 + unrolled_ops(plan, pc + 1, end)); pc = end + 1; continue; }
    n++; pc++;
  }
  return n;
}

// NW: waves that share the formulas of one 64-review half
inline FormulaCut cut_formula_parts(const HostPlan& plan, uint32_t NW, bool sweep, const JitSwitches& sw) {
  FormulaCut cut;
  cut.blks = price_blocks(plan, sweep, sw);
  const std::vector<Blk>& blks = cut.blks;
  for (auto& B : blks) cut.n_stages = std::max(cut.n_stages, B.stage + 1);
  if (cut.n_stages > 1 && chain_blocks(blks, NW, &cut.parts)) cut.n_stages = 1;
  else {
    cut.parts.assign((size_t)cut.n_stages * NW, {});
    for (uint32_t st = 0; st < cut.n_stages; st++) {   // greedy balance: heaviest block to the lightest wave
      std::vector<size_t> ids;
      for (size_t bi = 0; bi < blks.size(); bi++) if (blks[bi].stage == st) ids.push_back(bi);
      by_cost(blks, &ids);
      std::vector<uint64_t> load(NW, 0);
      for (size_t bi : ids) {
        const uint32_t w = lightest(load);
        load[w] += blks[bi].cost;
        cut.parts[(size_t)st * NW + w].push_back(bi);
      }
    }
  }
  // the preloaded form when its unrolled text stays small: operations after unrolling, summed over the parts
  cut.use_pre = sw.preload;
  if (cut.use_pre) {
    constexpr size_t pre_budget = 12000;   // (100 000 -- every part of the corpus plans unrolled -- measured slower: 0.6045 against 0.5141 ms summed over the groups)
    uint64_t total = 0;
    for (auto& part : cut.parts) for (size_t bi : part) total += unrolled_ops(plan, blks[bi].pc0, blks[bi].pc1);
    for (const Scope& sc : plan.scopes) if (sc.cap > 16) total = ~0ull;   // (large capacities keep their loops)
    if (total > pre_budget) cut.use_pre = false;
  }
  return cut;
}

}  // namespace gk::cg
