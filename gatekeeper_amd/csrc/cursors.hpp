// LOOP CURSORS (self-joins).  Shared by the lowering, the code generator and the bytecode interpreter.
//
// The formula ops that walk or address elements -- F_LOOP (a, and the parent b - 1), F_ENDLOOP / F_ENDLOOP2, F_LDE / F_STE (b) and
// F_VEQ's extra word -- name a CURSOR, not a scope: the plan's Scope table is indexed by cursor.  Cursor s below the number of element
// scopes is scope s's PRIMARY cursor (a plan without a self-join has no other).  The entries behind them are ALIAS cursors, each a
// copy of its scope's entry -- the same element words, the same count, hence the same loop bound --, for a second loop over a scope
// whose first loop is still open (`a := cs[_]; b := cs[_]`, lower.cpp Lowerer::open_cursor): the inner loop walks the elements with
// a counter of its own instead of resetting the outer loop's.  Scopes and aliases share the GK_MAX_SCOPES ids.
//
// This header and vm_cursors.inc are not part of the text handed to hiprtc (jit_source.hpp strips the includes): the generated
// plan code evaluates the relations itself (codegen.cpp), and the text of a plan without a self-join stays what it was.
#pragma once
#include <cstdint>

#include "plan.hpp"

namespace gk {

// F_KCMP + CmpOp (one word):  a = (ordinal of cursor b) <CmpOp> (ordinal of cursor c).  Ordinals are array indices: a relation between
// the keys of two array iterations (`c[i]; c[j]; i != j`, pe.hpp Atom::KEYREL).
constexpr uint32_t F_KCMP = 18;
constexpr uint32_t F_KCMP_LAST = F_KCMP + C_GE;
inline constexpr bool is_kcmp(uint32_t op) { return op >= F_KCMP && op <= F_KCMP_LAST; }

// F_VCMP + CmpOp (C_LT .. C_GE; followed by F_VEQ's extra word):  a = (value slot A) <CmpOp> (value slot B) under Rego's total order,
// false when either slot is empty.  The slots hold value ids as for F_VEQ; the ids of a table flattened with an ORDERED value pattern in
// the registry are RANKS -- id(a) < id(b) iff a < b within the review (flatten.cpp Flattener::rank_review) -- so the relation is one
// unsigned compare of the two ids.  `==` / `!=` between two review values stay F_VEQ.
constexpr uint32_t F_VCMP = 24;
inline constexpr bool is_vcmp(uint32_t op) { return op >= F_VCMP + C_LT && op <= F_VCMP + C_GE; }
// the ops that carry F_VEQ's extra word: every scan of the formula code steps over it
inline constexpr bool has_slot_word(uint32_t op) { return op == F_VEQ || is_vcmp(op); }

// F_KIMM + CmpOp (one word):  a = (ordinal of cursor b) <CmpOp> c, with c an 8-bit constant: the index of an array element against a
// number (`cs[0]`, `cs[i]; i > 0`, pe.hpp Atom::KEYCMP).  Only on the cursors of top-level scopes, whose ordinals are the indices.
constexpr uint32_t F_KIMM = 30;
inline constexpr bool is_kimm(uint32_t op) { return op >= F_KIMM && op <= F_KIMM + C_GE; }
// F_KEND (one word):  a = (ordinal of cursor b) + c == the element count of cursor b's scope: element c from the end (`cs[count(cs) - c]`).
constexpr uint32_t F_KEND = 36;

}  // namespace gk
