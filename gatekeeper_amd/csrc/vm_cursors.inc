      // (cursors.hpp) F_KCMP + CmpOp: reg a = ordinal of cursor b <CmpOp> ordinal of cursor c
      case F_KCMP + C_EQ: case F_KCMP + C_NE: case F_KCMP + C_LT: case F_KCMP + C_LE: case F_KCMP + C_GT: case F_KCMP + C_GE: {
        const uint32_t i = cur[b], j = cur[c], rel = op - F_KCMP;
        const bool v = rel == C_EQ ? i == j : rel == C_NE ? i != j : rel == C_LT ? i < j : rel == C_LE ? i <= j : rel == C_GT ? i > j : i >= j;
        B = (B & ~(1ull << a)) | ((uint64_t)v << a);
        break;
      }
      // (cursors.hpp) F_VCMP + CmpOp: reg a = value slot <CmpOp> value slot, both ids read as F_VEQ reads them; the ids are ranks
      case F_VCMP + C_LT: case F_VCMP + C_LE: case F_VCMP + C_GT: case F_VCMP + C_GE: {
        const uint32_t x = GK_UNI(code[pc++]), rel = op - F_VCMP;
        const uint32_t sa = x & 0xFF, la = (x >> 8) & 0xFF, sb = (x >> 16) & 0xFF, lb = x >> 24;
        const Scope& A = pv.scopes[sa];
        const Scope& Bs = pv.scopes[sb];
        const uint32_t ia = scope_packed(A) ? (acc.load(A.word_off + cur[sa] * A.wpe) >> ELEM_VID_SHIFT) & GK_VID_OVERFLOW
                                            : acc.load(A.val_off + cur[sa] * val_stride(A.nvals) + la);
        const uint32_t ib = scope_packed(Bs) ? (acc.load(Bs.word_off + cur[sb] * Bs.wpe) >> ELEM_VID_SHIFT) & GK_VID_OVERFLOW
                                             : acc.load(Bs.val_off + cur[sb] * val_stride(Bs.nvals) + lb);
        const bool r = rel == C_LT ? ia < ib : rel == C_LE ? ia <= ib : rel == C_GT ? ia > ib : ia >= ib;
        const bool v = r & (ia != 0u) & (ib != 0u);
        B = (B & ~(1ull << a)) | ((uint64_t)v << a);
        break;
      }
      // (cursors.hpp) F_KIMM + CmpOp: reg a = ordinal of cursor b <CmpOp> the constant c
      case F_KIMM + C_EQ: case F_KIMM + C_NE: case F_KIMM + C_LT: case F_KIMM + C_LE: case F_KIMM + C_GT: case F_KIMM + C_GE: {
        const uint32_t i = cur[b], rel = op - F_KIMM;
        const bool v = rel == C_EQ ? i == c : rel == C_NE ? i != c : rel == C_LT ? i < c : rel == C_LE ? i <= c : rel == C_GT ? i > c : i >= c;
        B = (B & ~(1ull << a)) | ((uint64_t)v << a);
        break;
      }
      // (cursors.hpp) F_KEND: reg a = ordinal of cursor b + c == the element count of its scope (the review's own: max ordinal + 1)
      case F_KEND: {
        const bool v = cur[b] + c == acc.load(pv.scopes[b].count_off);
        B = (B & ~(1ull << a)) | ((uint64_t)v << a);
        break;
      }
