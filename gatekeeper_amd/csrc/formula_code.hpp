// Reader of the formula code (plan.hpp F_*, cursors.hpp) for the plan code generator (codegen.cpp): one decoded instruction, the extra
// word of the value-slot ops, the end of a loop, and which registers an instruction reads and writes.  Host only: not part of the
// text hiprtc compiles.
#pragma once
#include "cursors.hpp"
#include "lower.hpp"

namespace gk::cg {

struct FIns { uint32_t op, a, b, c; };
inline FIns decode(uint32_t w) { return {w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF, w >> 24}; }
inline uint32_t global_bit(const FIns& i) { return i.b | (i.c << 8); }   // F_LDG / F_STG

// the word behind F_VEQ / F_VCMP: value slot `la` of cursor `sa` against slot `lb` of cursor `sb`
struct SlotWord { uint32_t sa, la, sb, lb; };
inline SlotWord decode_slots(uint32_t x) { return {x & 0xFF, (x >> 8) & 0xFF, (x >> 16) & 0xFF, x >> 24}; }

// index of the instruction behind the one at pc (steps over the slot word)
inline size_t next_ins(const std::vector<uint32_t>& code, size_t pc) { return pc + (has_slot_word(code[pc] & 0xFF) ? 2 : 1); }

// pc: first instruction of a loop body -> the index of its F_ENDLOOP / F_ENDLOOP2
inline size_t loop_end(const std::vector<uint32_t>& code, size_t pc) {
  for (int depth = 0;; pc = next_ins(code, pc)) {
    const uint32_t op = code[pc] & 0xFF;
    if (op == F_LOOP) depth++;
    if (op == F_ENDLOOP || op == F_ENDLOOP2) { if (depth == 0) return pc; depth--; }
    if (op == F_END) throw Unsupported("codegen: loop without an end");
  }
}

// the formula registers an instruction reads and writes (F_LOOP zeroes its accumulator; the value-slot ops and the key relations read
// no register).  known: false for an op this table does not list
struct RegUse { std::vector<uint32_t> reads, writes; bool known = true; };
inline RegUse reg_use(const FIns& i) {
  RegUse r;
  switch (i.op) {
    case F_LDG: case F_LDF: case F_LDE: case F_CONST: case F_VEQ: r.writes = {i.a}; break;
    case F_AND: case F_OR: case F_ANDN: r.reads = {i.b, i.c}; r.writes = {i.a}; break;
    case F_NOT: case F_MOV: r.reads = {i.b}; r.writes = {i.a}; break;
    case F_LOOP: r.writes = {i.c}; break;
    case F_ENDLOOP: r.reads = {i.a, i.b}; r.writes = {i.a}; break;
    case F_ENDLOOP2: r.reads = {i.a, i.b, i.c}; r.writes = {i.a, i.c}; break;
    case F_RES: case F_STE: case F_STG: r.reads = {i.a}; break;
    case F_END: break;
    default: if (is_vcmp(i.op) || is_kcmp(i.op) || is_kimm(i.op) || i.op == F_KEND) r.writes = {i.a}; else r.known = false;
  }
  return r;
}

}  // namespace gk::cg
