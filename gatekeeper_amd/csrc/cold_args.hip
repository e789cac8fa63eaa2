// COLD LAUNCH ARGUMENTS of the plan-specialised sweep kernel (gk_jit_tiles at sweep geometry): the stage text that embed_sources.py
// splices into kernel_body.inc to make the COLD-ARGS variant (kKernelBodyCold / kKernelBodyRwCold; COLD_HOOKS there name the anchors).
// kernel_body.inc itself stays as it is: the bytecode build, the kernel emulator, gk_jit_big and the texts of small tables include it.
//
// Why: the kernel has no scalars to spare (57 spilled to vector lanes at the 64-VGPR budget of configs[2]).  A launch argument is a
// scalar from the prologue to its last use, and the arguments that only the per-item TAIL reads -- the output pointers, n_tiles, slots,
// the list and flag arrays of the next item's requests -- were live across phase 1 and the formulas, where they were spilled, and came
// back in the tail through v_readlane chains with wait states, at priority 3, once per row group and wave.  Here such an argument is no
// function-lifetime value: the stage that uses it reads it from the KERNEL-ARGUMENT SEGMENT (scalar loads through the scalar cache; the
// segment pointer is two scalars the ABI provides anyway).  The kernel's parameter list does not change, so neither does the launch.
// The segment pointer is made opaque once per item: otherwise the loads are hoisted out of the group loop and spilled again.
//
// A section starts at a line `//== name` and ends at the next one.
//== args
// The parameter list of gk_jit_tiles as one struct: the kernel-argument segment holds the parameters in this order, each at its natural
// alignment, which is how a struct lays them out.  tests/test_cold_args_text.py compares every offset the text reads with the `.offset`
// the code object's own metadata records for that argument; kernels.hip includes this section and builds its launch from the same struct.
struct GkTilesArgs {
  PlanView pv;
  const Row* rows;
  const StrHdr* shdr;
  const ChunkDesc* lists;
  uint32_t capg;
  const uint32_t* rflags;
  const uint8_t* heap;
  uint32_t n_reviews, n_tiles;
  const ConstraintSlot* slots;
  OutPtrs out;
  uint32_t dbg, rpp;
#if defined(GK_RW_K) || defined(GK_ARGS_WITH_RW)
  const uint32_t* rwords;   // (the review-words variant's two trailing parameters)
  uint32_t rw_stride;
#endif
};
//== device
typedef const __attribute__((address_space(4))) uint8_t* gk_kargs_t;
template <typename T>
__device__ inline T gk_karg(gk_kargs_t ka, uint32_t off) { return *reinterpret_cast<const __attribute__((address_space(4))) T*>(ka + off); }
#define GK_KARG(ka, field) gk_karg<decltype(((GkTilesArgs*)0)->field)>((ka), (uint32_t)__builtin_offsetof(GkTilesArgs, field))
#define GK_KARGS(ka) gk_kargs_t ka = (gk_kargs_t)__builtin_amdgcn_kernarg_segment_ptr(); asm volatile("" : "+s"(ka))
//== carried
  // the arrays of the next item's requests (entry_of / flags_of): from the parameters in the prologue, from the argument segment in
  // every tail -- assigned there right in front of their only uses, so nothing of them is live across phase 1 and the formulas
  const ChunkDesc* lists_c = lists;
  const uint32_t* rflags_c = rflags;
//== tail_head
    // the tail's cold arguments, requested in front of the flag ballots: they travel (lgkmcnt) while the ballots issue
    GK_KARGS(ka);
    lists_c = GK_KARG(ka, lists);
    rflags_c = GK_KARG(ka, rflags);
    const uint32_t n_tiles_now = GK_KARG(ka, n_tiles);
    uint64_t* const o_viol = GK_KARG(ka, out.viol);
    uint64_t* const o_err = GK_KARG(ka, out.err);
    uint64_t* const o_match = GK_KARG(ka, out.match);
    uint64_t* const o_overflow = GK_KARG(ka, out.overflow);
    uint64_t* const o_too_big = GK_KARG(ka, out.too_big);
    uint32_t* const o_list = GK_KARG(ka, out.list);
    uint32_t* const o_list_count = GK_KARG(ka, out.list_count);
    const uint32_t o_list_capacity = GK_KARG(ka, out.list_capacity);
    const uint32_t nc_now = GK_KARG(ka, pv.dims.n_constraints);
//== tail
    constexpr uint32_t OUT_B = GK_PARTS_K > 1 ? 1u : 0u;
    if (wave_on && (part == 0 || part == OUT_B)) {
      const uint32_t word = tile * GK_HALVES_K + pass * halves_per_pass + half;     // the half's bitmap word
      const bool do_v = part == 0, do_e = part == OUT_B;
      if (do_e && lane == 0 && word < n_tiles_now) {
        o_overflow[word] = ovf_mask;
        if (ovf_mask) atomicAdd(&o_list_count[1], (uint32_t)__popcll(ovf_mask));
        o_too_big[word] = refused;   // every half writes its word: no clearing pass; the big variant ORs into it later
      }
      // lane s: the words of match / error slot s and of violation slots s, 64 + s, ... (one register pair per bank of 64 violation slots:
      // a plan with up to 64 distinct violation formulas has one)
      const uint32_t sl = lane < (uint32_t)GK_RES_KM ? lane : 0u;
      const unsigned long long wm = hm[GK_RES_KV + sl];
      const unsigned long long we = do_e ? hm[GK_RES_KV + GK_RES_KM + sl] : 0ull;
      unsigned long long wv[GK_RES_BANKS_K];
#pragma unroll
      for (uint32_t bk = 0; bk < (uint32_t)GK_RES_BANKS_K; bk++) wv[bk] = do_v ? hm[bk * 64u + lane < (uint32_t)GK_RES_KV ? bk * 64u + lane : 0u] : 0ull;
      const uint32_t nc = GK_DBG(64u) ? 0u : nc_now;
      // one batch of 64 constraints: lane c of the batch = constraint cb + c, slw = its (violation slot | match slot << 16)
      auto emit = [&](uint32_t cb, uint32_t slw) {
        const uint32_t c = cb + lane;
        const int sv = (int)(slw & 0xFFFFu), sm = (int)(slw >> 16);
        const unsigned long long m = (((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(wm >> 32), sm) << 32) | (uint32_t)__shfl((int)(uint32_t)wm, sm)) | prem;
        const bool mine = c < nc && word < n_tiles_now;
        if (do_v) {
          unsigned long long v = 0ull;
#pragma unroll
          for (uint32_t bk = 0; bk < (uint32_t)GK_RES_BANKS_K; bk++) {
            const unsigned long long x = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(wv[bk] >> 32), sv & 63) << 32) | (uint32_t)__shfl((int)(uint32_t)wv[bk], sv & 63);
            if (GK_RES_BANKS_K == 1 || (uint32_t)(sv >> 6) == bk) v = x;
          }
          const unsigned long long vw = m & v & usable;
          if (mine) {
            o_viol[(size_t)c * n_tiles_now + word] = vw;
            if (vw && o_list_capacity) {
              // compacted (constraint, review) list: per-constraint totals come from gk_count_rows over the finished bitmap
              const uint32_t n = (uint32_t)__popcll(vw);
              uint32_t q = atomicAdd(&o_list_count[0], n);
              for (unsigned long long w = vw; w; w &= w - 1ull, q++)
                if (q < o_list_capacity) { o_list[2 * q] = c; o_list[2 * q + 1] = r0 + rev_lo + half * GK_TILE + (uint32_t)__builtin_ctzll(w); }
            }
          }
#ifdef GK_TOT_K
          GK_LDS_ADD(&s_tot[lane + (mine ? cb : 0u)], (uint32_t)__popcll(mine ? vw : 0ull));
#endif
        }
        if (do_e) {
          const unsigned long long e = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(we >> 32), sm) << 32) | (uint32_t)__shfl((int)(uint32_t)we, sm);
          const unsigned long long ew = e & usable & ~prem, mw = m & usable;
          if (mine) {
            o_err[(size_t)c * n_tiles_now + word] = ew;
            if (o_match) o_match[(size_t)c * n_tiles_now + word] = mw;
          }
        }
      };
      // the first batch takes its slots from LDS (no vector load on the usual path: it would have to wait for the rows requested
      // above -- loads return in order); further batches read theirs, and only they touch the slots pointer
      uint32_t lane_o = lane;   // (opaque: a hoisted, spilled LDS address would come back through a load)
      GK_OPAQUE_V1(lane_o);
      if (nc) emit(0u, s_slw[lane_o]);
      for (uint32_t cb = GK_TILE; cb < nc; cb += GK_TILE) {
        const ConstraintSlot* const slots_c = GK_KARG(ka, slots);   // (read here: a plan of up to 64 constraints never asks for it)
        uint32_t slw = 0;
        if (cb + lane < nc) slw = *reinterpret_cast<const uint32_t*>(&slots_c[cb + lane]);
        emit(cb, slw);
      }
    }
//== epilogue
  __syncthreads();   // every output wave's adds are in
  {
    GK_KARGS(ka);
    uint32_t* const o_partial = GK_KARG(ka, out.partial);
#pragma unroll
    for (uint32_t q = threadIdx.x; q < (uint32_t)GK_TOT_K; q += GK_BLOCK_K) o_partial[(size_t)blockIdx.x * GK_TOT_K + q] = s_tot[q];
  }
#endif
