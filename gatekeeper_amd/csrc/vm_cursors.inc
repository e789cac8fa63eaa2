      // (cursors.hpp) F_KCMP + CmpOp: reg a = ordinal of cursor b <CmpOp> ordinal of cursor c
      case F_KCMP + C_EQ: case F_KCMP + C_NE: case F_KCMP + C_LT: case F_KCMP + C_LE: case F_KCMP + C_GT: case F_KCMP + C_GE: {
        const uint32_t i = cur[b], j = cur[c], rel = op - F_KCMP;
        const bool v = rel == C_EQ ? i == j : rel == C_NE ? i != j : rel == C_LT ? i < j : rel == C_LE ? i <= j : rel == C_GT ? i > j : i >= j;
        B = (B & ~(1ull << a)) | ((uint64_t)v << a);
        break;
      }
