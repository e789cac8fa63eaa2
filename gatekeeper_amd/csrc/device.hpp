// Device backend interface between the host engine (engine.cpp) and the HIP kernels (kernels.hip).
// The product library links kernels.hip.  tests/native/hostemu.cpp implements the same interface on the CPU for
// the build container's GPU-less unit tests ONLY (libgkgpu_hostemu.so; never loaded by the product path).
#pragma once
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

#include "flatten.hpp"
#include "key_join.hpp"
#include "lower.hpp"
#include "verify_merge.hpp"

namespace gk {

struct DevTable;
struct DevPlan;

struct EvalOptions {
  bool download = true;      // copy bitmaps / list back to the host
  bool want_match = false;   // also produce the match-only bitmap
  uint32_t list_capacity = 0;   // max violation-list entries (0 = no list)
  bool shard = false;           // results go to the shard slot prepared by dev_shard_setup (bitmap stride = the largest shard's)
  bool detached = false;        // (kernels.hip, internal) an enqueue-only pass that dev_eval_finish never collects: see dev_shard_enqueue
  bool kernel_only = false;     // GK_EVAL_KERNEL_ONLY: no totals kernel behind the dominant one (back-to-back timing of that kernel)
  bool time_each = false;       // GK_EVAL_TIME_EACH: an event pair around EVERY launch (isolated kernel durations) instead of one around all pending ones
  bool timed = true;            // the launches up to the collecting call are bracketed by one event pair (kernel_ms / fast_kernel_ms); false: an
                                //   enqueue-only sweep nobody asked the duration of records no event -- the collecting call then reports 0
  bool jit_wait = true;         // wait for the plan-specialised build of the dominant kernel; false (admission batches): never
                                //   block -- the bytecode kernel serves until the background build has been loaded
  bool bytecode = false;        // the ahead-of-time bytecode kernel whatever the plan says: never asks for the plan-specialised build and neither
                                //   reads nor leaves any cached launch state (the reference side of dev_verify_diff)
};

struct EvalOut {
  uint32_t n_reviews = 0, n_constraints = 0, n_tiles = 0;
  std::vector<uint64_t> viol;     // [n_constraints][n_tiles]  bit r%64 of word r/64: constraint matched AND violated
  std::vector<uint64_t> err;      // [n_constraints][n_tiles]  Matcher.Match returned an error (autoreject)
  std::vector<uint64_t> match;    // [n_constraints][n_tiles]  (only if want_match)
  std::vector<uint64_t> too_big;  // [n_tiles] reviews that exceed engine limits even in the large variant
  std::vector<uint32_t> counts;   // [n_constraints] violating reviews per constraint
  std::vector<uint32_t> list;     // pairs (constraint, review) -- compacted violation list
  uint32_t list_total = 0;        // entries the kernel wanted to emit (may exceed capacity)
  uint32_t n_overflow = 0;        // reviews re-run in the large-capacity variant
  float kernel_ms = 0;            // device time of the evaluation kernels (HIP events on the launch stream)
  float fast_kernel_ms = 0;       // average duration of the dominant (LDS) kernel per launch since the last finish
  uint32_t n_launches = 0;        // launches averaged in fast_kernel_ms
  uint32_t lds_bytes = 0;         // accumulator LDS per workgroup of the dominant kernel's most recent launch
  uint64_t list_bytes = 0;        // chunk lists the dominant kernel reads per launch (chunks.hpp)
  uint64_t rw_bytes = 0;          // review words the most recent launch read instead of rw_rows rows (rw_hdr_rows of them with their string headers) of
  uint64_t rw_rows = 0, rw_hdr_rows = 0;   //   the plan's all-global predicate classes (review_words.hpp); 0: the sweep walked every class
  uint64_t kernel_hash = 0;       // FNV-64 of the plan-specialised kernel's source text (0: the bytecode kernel ran)
  bool specialised = false;       // the plan-specialised code evaluated the most recent launch (the CPU stand-in: the generated plan source)
  const void *d_viol = nullptr, *d_err = nullptr, *d_counts = nullptr;   // device-resident results (valid until the table's next launch)
};

std::string dev_init(int device);                       // "" on success, else error text
int dev_count();
// A table goes to the device in PARTS: every host thread uploads the part it flattened as soon as it is done
// (dev_part_upload: thread-safe, overlaps the other threads' flattening and their transfers); dev_table_assemble then
// places the parts one after the other in the table's arrays ON THE DEVICE, relocating the rows' heap offsets there -- the
// host never merges the gigabytes.  `meta` carries what is global: tile_idx, slot_path, rflags, n_reviews.
struct DevPart;
DevPart* dev_part_upload(int device, HostTable& part);   // releases the part's host arrays (rows / shdr / heap)
void dev_part_free(DevPart* p);
DevTable* dev_table_assemble(int device, std::vector<DevPart*>& parts, const HostTable& meta);   // consumes the parts
void dev_table_free(DevTable* t);
// A second handle on the same resident table with its own result buffers and path binding (plan groups beyond the
// first evaluate through views); freeing a view leaves the table's arrays alone.  Free views before the table.
DevTable* dev_table_view(DevTable* base);
uint64_t dev_table_bytes(const DevTable* t);
DevPlan* dev_plan_upload(int device, const HostPlan& fast, const HostPlan& big);
void dev_plan_free(DevPlan* p);
// this plan is served by the bytecode kernel only from now on (the small one-sweep-per-audit plans of the RESULT totals; a plan group that
// gk_table_verify quarantined).  Tables drop whatever launch state they cached for the plan: call it while no evaluation of the plan runs.
void dev_plan_no_jit(DevPlan* p);
void dev_eval(const DevPlan* p, const DevTable* t, const EvalOptions& opt, EvalOut* out);   // launch + finish; throws std::runtime_error
// first-k violating reviews per bitmap row in `order` (reviews sorted by object key; grp = dense key rank, ties equal);
// uses the bitmaps of the table's most recent evaluation.  idx: [nc][cap], n: [nc], ovf: [nc]
void dev_topk(const DevTable* t, uint32_t nc, const std::vector<uint32_t>& order, const std::vector<uint32_t>& grp, uint32_t k, uint32_t cap,
              std::vector<uint32_t>* idx, std::vector<uint32_t>* n, std::vector<uint32_t>* ovf);
// resident-set audit lists: dev_topk's selection (same tie rule, cap and overflow flag) restricted to the reviews whose bit is set in
// `shown` (one bit per review), plus the masked pair total of every bitmap row from the same pass.  The mask stays on the device beside
// the table (views share it) and is uploaded again only when `shown_gen` differs from the generation it went up under; order / grp
// go up once per table.  pairs: [nc], idx: [nc][cap], n: [nc], ovf: [nc]
void dev_audit_select(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint32_t>& order, const std::vector<uint32_t>& grp,
                      const std::vector<uint64_t>& shown, uint64_t shown_gen, uint32_t k, uint32_t cap,
                      std::vector<uint32_t>* pairs, std::vector<uint32_t>* idx, std::vector<uint32_t>* n, std::vector<uint32_t>* ovf);
// resident-set violation stream: every review that is set in `shown` and has a bit in at least one row of the most recent evaluation's
// violation bitmap, with the rows it has them in.  dev_viol_index: cnt[w] = such reviews in bitmap word w (pw = ceil(n_reviews / 64)
// words; `any`, when asked for, the reviews themselves as a bit word -- for a caller that merges further sources per word); it leaves
// the prefix sum of cnt beside the table.  dev_viol_entries: the entries of the words [w0, w1) -- reviews ascending, masks
// [entries][ceil(nc / 64)], bit r = row r -- placed by that prefix sum; it throws when the index belongs to another evaluation or mask.
// The mask is dev_audit_select's device copy (same shown_gen rule).
void dev_viol_index(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, uint64_t shown_gen,
                    std::vector<uint32_t>* cnt, std::vector<uint64_t>* any = nullptr);
void dev_viol_entries(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, uint64_t shown_gen, uint32_t w0, uint32_t w1,
                      std::vector<uint32_t>* reviews, std::vector<uint64_t>* masks);
// resident-set changes stream (gk_resident_changes): what differs between the most recent evaluation's violation bitmap read under `shown`
// and the BASELINE of the table (view) -- a copy of that bitmap and of the mask it was read under, made by dev_delta_keep (device to
// device, allocated at the first call) and held beside the table until dev_delta_drop or the table goes away.  A review that is not set
// in a side's mask counts as all zero on that side.  Without use_base, or when the table has no baseline, the baseline reads as zero
// (no buffer is filled for that); a baseline of another row count or layout makes both entries throw.  dev_delta_has: a baseline for
// `nc` rows of this table is there; dev_delta_bytes: what it holds on the device.
// dev_delta_index: changed[w] = the reviews of bitmap word w with a differing bit in at least one row, cnt[w] = their number.
// dev_delta_entries: the entries of the words [w0, w1), reviews ascending, `now` / `was` = [entries][ceil(nc / 64)] masks of the two
// sides, bit r = row r.  `off` is the page's slice [w1 - w0 + 1] of the exclusive prefix sum that places the entries (the caller keeps
// the index); `extra`, when given, [w1 - w0] words of reviews that get an entry whatever this table's bitmaps say -- a caller that
// merges several sources per word passes the merged words, so that every source emits the same reviews.  It throws when the index does
// not fit the bitmaps.  *ms: HIP-event time of the call's kernels (the CPU stand-in: 0).  The mask is dev_audit_select's device copy.
void dev_delta_keep(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, uint64_t shown_gen);
bool dev_delta_has(const DevTable* t, uint32_t nc);
uint64_t dev_delta_bytes(const DevTable* t);
void dev_delta_drop(const DevTable* t);
void dev_delta_index(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, uint64_t shown_gen, bool use_base,
                     std::vector<uint32_t>* cnt, std::vector<uint64_t>* changed, float* ms);
void dev_delta_entries(const DevTable* t, uint32_t nc, uint32_t n_reviews, const std::vector<uint64_t>& shown, uint64_t shown_gen, bool use_base, uint32_t w0,
                       uint32_t w1, const std::vector<uint32_t>& off, const std::vector<uint64_t>* extra, std::vector<uint32_t>* reviews,
                       std::vector<uint64_t>* now, std::vector<uint64_t>* was, float* ms);
// table violation stream (gk_table_violations): every review with a bit in at least one row of the violation OR the autoreject bitmap of
// the most recent evaluation, over ALL plan groups at once.  A side is what one group evaluated into (the table or a view of it), its
// rows and its first row among all constraints; sides without rows are skipped.  Reviews with a too_big bit in any side are masked
// (their device bits are unspecified) and counted in *beyond.  dev_tviol_index: cnt[w] = entries of bitmap word w ([ceil(n_reviews /
// 64)]; `any`, when asked for, the reviews themselves).  dev_tviol_entries: the entries of the words [w0, w1), reviews ascending, masks
// [entries][ceil(total rows / 64)] with bit row0 + r = row r of the side; `off` = the exclusive prefix sum of cnt ([words + 1], the
// caller keeps it) places them, and the call throws when it does not fit the bitmaps.  Both throw while launches of a side are still to
// be collected.  *ms: HIP-event time of the call's kernels (the CPU stand-in: 0).
struct TviolSide { const DevTable* t = nullptr; uint32_t nc = 0, row0 = 0; };
void dev_tviol_index(const std::vector<TviolSide>& sides, uint32_t n_reviews, std::vector<uint32_t>* cnt, std::vector<uint64_t>* any, uint64_t* beyond, float* ms);
void dev_tviol_entries(const std::vector<TviolSide>& sides, uint32_t n_reviews, const std::vector<uint32_t>& off, uint32_t w0, uint32_t w1,
                       std::vector<uint32_t>* reviews, std::vector<uint64_t>* viol, std::vector<uint64_t>* err, float* ms);
// what a collected evaluation of `t` answered, for a backend that cannot read its result buffers back later (the CPU stand-in keeps the
// three bitmaps beside the table's address; the device reads its own buffers and does nothing here) / the table (view) is going away
void dev_tviol_note(const DevTable* t, const EvalOut& o);
void dev_tviol_forget(const DevTable* t);
// table changes stream (gk_table_snapshot / gk_table_changes): one list-based audit cycle's answer compared with a kept earlier one.
// dev_snap_take copies what dev_tviol_index would read -- the bitmaps of all sides, device to device -- into ONE flat layout,
// viol / err = [rows][pw] with every side's rows at its row0 (rows = the largest row0 + nc, pw = ceil(n_reviews / 64)), plus the OR of
// the sides' too_big words; the snapshot owns its memory (device pool) and outlives the table.
// dev_tchg_align lines a snapshot up with a table of `n` reviews: was_viol / was_err = [rows_now][ceil(n / 64)] where bit i of row r is
// bit then_of[i] of the snapshot's row row_of[r] (then_of[i] / row_of[r] == 0xFFFFFFFF: zero; then_of == nullptr: the identity over the
// snapshot's own reviews, n = its count), and was_big likewise from the snapshot's too_big words.  A null snapshot aligns to all zero
// without buffers.  `moved` (reviews whose version differs) and `only` (the reviews the side is about; none: all) are [ceil(n / 64)]
// words the aligned side keeps with it.  The caller owns the result (dev_tchg_free) and keeps it for the life of a stream.
// dev_tchg_index: changed[w] = the reviews of word w with (viol ^ was_viol) | (err ^ was_err) != 0 in some row, the was side read under
// NOT was_big, or that are in `moved` and have a bit now; all under care = below n, in `only`, NOT in any side's too_big.  big[w] = the
// sides' too_big bits below n, *beyond their number.  Without sides the now side reads as zero (the gone reviews of a snapshot).
// dev_tchg_entries: the entries of the words [w0, w1) -- reviews ascending, four masks [entries][ceil(rows_now / 64)], bit r = row r of
// the table now -- of the reviews (changed & ~drop) | extra; drop / extra: [w1 - w0] words or empty.  `off` = the page's slice
// [w1 - w0 + 1] of the exclusive prefix sum over those words; the call throws when it does not fit the bitmaps.  The now masks of a
// review with a too_big bit are unspecified.  *ms: HIP-event time of the call's kernels (the CPU stand-in: 0).
struct DevSnap;
struct DevAligned;
DevSnap* dev_snap_take(const std::vector<TviolSide>& sides, uint32_t n_reviews);
void dev_snap_free(DevSnap* s);
uint64_t dev_snap_bytes(const DevSnap* s);
DevAligned* dev_tchg_align(int device, const DevSnap* s, uint32_t n, const std::vector<uint32_t>* then_of, const std::vector<uint32_t>& row_of,
                           const std::vector<uint64_t>* moved, const std::vector<uint64_t>* only, float* ms);
void dev_tchg_free(DevAligned* a);
void dev_tchg_index(const std::vector<TviolSide>& sides, uint32_t n, const DevAligned* a, std::vector<uint32_t>* cnt, std::vector<uint64_t>* changed,
                    std::vector<uint64_t>* big, uint64_t* beyond, float* ms);
void dev_tchg_entries(const std::vector<TviolSide>& sides, uint32_t n, const DevAligned* a, const std::vector<uint32_t>& off, uint32_t w0, uint32_t w1,
                      const std::vector<uint64_t>& drop, const std::vector<uint64_t>& extra, std::vector<uint32_t>* reviews, std::vector<uint64_t>* viol,
                      std::vector<uint64_t>* err, std::vector<uint64_t>* was_viol, std::vector<uint64_t>* was_err, float* ms);
// as dev_tviol_note / dev_tviol_forget, for the CPU stand-in of the entries above (the device does nothing here)
void dev_tchg_note(const DevTable* t, const EvalOut& o);
void dev_tchg_forget(const DevTable* t);
// ---- the key join of a changes stream on the device (GK_CHANGES_DEVICE_JOIN, gk_table_join; key_join.hpp holds the pure part).
// dev_keys_put: one side's packed key records and their offsets (kjoin_pack) on the device; the holder owns its memory (device pool) as
// a DevSnap does and outlives whatever the keys were packed from.
// dev_kjoin: delta_join's three arrays, bit for bit, from an exact hash join of the two sides' records -- gk_kjoin_build over the
// snapshot's reviews, gk_kjoin_probe over the table's, gk_kjoin_finish over both, back to back on one stream; hashes are masked to
// `hash_bits` bits (kjoin_mask).  What the kernels cannot pair without the occurrence rule -- every review whose key occurs more than
// once on some side and is present in the snapshot -- comes back as flagged_now / flagged_then bit words and is settled by
// kjoin_resolve on the host (key_now / key_then are asked for those reviews only); unmatched takes their bits from there.  It throws
// KjoinFault when the kernels set their error word (a probe loop that ran out of slots, a record outside the arena): nothing of the
// answer is used then.  *keep, when asked for, holds then_of as it stands on the device, the flagged reviews patched, for the
// dev_tchg_align overload below (no second upload); the caller frees it (dev_join_free).  *ms: HIP-event time of the three kernels
// (the CPU stand-in: 0).
struct DevKeys;
struct DevJoin;
// (a side's key accessor: a plain function with its context -- it is called from sort comparators)
struct KjKeyFn {
  std::string_view (*fn)(const void* ctx, uint32_t review);
  const void* ctx;
  std::string_view operator()(uint32_t review) const { return fn(ctx, review); }
};
DevKeys* dev_keys_put(int device, const KjUnit* rec, size_t units, const uint32_t* off, uint32_t n);
void dev_keys_free(DevKeys* k);
uint64_t dev_keys_bytes(const DevKeys* k);
void dev_kjoin(const DevKeys* now, const DevKeys* then, uint32_t hash_bits, const KjKeyFn& key_now, const KjKeyFn& key_then, std::vector<uint32_t>* then_of,
               std::vector<uint32_t>* now_of, std::vector<uint64_t>* unmatched, std::vector<uint64_t>* flagged_now, std::vector<uint64_t>* flagged_then, KjoinStats* stats,
               float* ms, DevJoin** keep = nullptr);
void dev_join_free(DevJoin* j);
// dev_tchg_align with then_of taken from a finished dev_kjoin (n = its now side's reviews)
DevAligned* dev_tchg_align(int device, const DevSnap* s, uint32_t n, const DevJoin& then_of, const std::vector<uint32_t>& row_of, const std::vector<uint64_t>* moved,
                           const std::vector<uint64_t>* only, float* ms);
// the violation bitmap [nc][n_tiles] of the table's most recent evaluation (device -> host copy)
void dev_last_viol(const DevTable* t, uint32_t nc, std::vector<uint64_t>* viol);
// ---- the plan-specialised kernel checked against the bytecode kernel (gk_table_verify).
// dev_verify_eval: one side of a verification -- dev_eval_launch + dev_eval_finish without download; what it leaves beside the table (view)
// is what dev_verify_diff and dev_verify_flip work on (the device: the table's result buffers themselves).  out->specialised says whether
// the plan-specialised code ran.  dev_verify_twin: the plan the bytecode side evaluates -- nullptr where EvalOptions::bytecode selects the
// bytecode kernel of the plan itself (the device); a backend that binds its code to the plan at upload (the CPU stand-in) uploads a twin
// without the specialised code, which the caller keeps and frees with dev_plan_free.  dev_verify_forget: the table (view) is going away.
void dev_verify_eval(const DevPlan* p, const DevTable* t, const EvalOptions& opt, EvalOut* out);
DevPlan* dev_verify_twin(int device, const HostPlan& fast, const HostPlan& big);
void dev_verify_forget(const DevTable* t);
// dev_verify_diff: `a` holds the finished evaluation of one plan group on the specialised path, `b` -- a view of the same table -- the
// finished evaluation of the same plan with EvalOptions::bytecode; both by dev_verify_eval, same nc and want_match.  Compared are the bits of the reviews below n_reviews that NEITHER side left
// beyond the device's limits (too_big; their bits are unspecified) and, with `mask` (one bit per review, [ceil(n_reviews / 64)] words),
// that are set in it.  The two too_big words are compared as a kind of their own (row 0).
// (VerifyEntry / VerifyDiff: verify_merge.hpp)
void dev_verify_diff(const DevTable* a, const DevTable* b, uint32_t nc, uint32_t n_reviews, bool want_match, const std::vector<uint64_t>* mask,
                     uint32_t cap, VerifyDiff* out);
// test aid (gk_debug_set "verify_flip"): toggle bit `review` -- with whole_word all 64 bits of its word -- of row `row` of the `kind`
// bitmap of the table's (view's) most recent evaluation
void dev_verify_flip(const DevTable* t, uint32_t nc, uint32_t kind, uint32_t row, uint32_t review, bool whole_word);
// ---- multi-GPU exchange step of a sharded sweep: one communicator per engine (= per GPU / rank)
struct DevComm;
bool dev_comm_unique_id(char id[128], std::string* err);                                  // rank 0: ncclGetUniqueId
DevComm* dev_comm_init(int device, const char id[128], int rank, int world, std::string* err);   // ncclCommInitRank (RCCL over xGMI)
void dev_comm_free(DevComm* c);
int dev_comm_rank(const DevComm* c);
int dev_comm_world(const DevComm* c);
bool dev_comm_query(const DevComm* c, int* rank, int* world, std::string* err);   // ncclCommUserRank / ncclCommCount of the live communicator
// A table evaluated as one SHARD: its violation bitmap and counts live in this rank's slot of an all-gather buffer
// ([world] x ([nc][stride_tiles] u64 | tail | pad), tail below), stride_tiles = the largest shard's words per row.
struct ShardInfo {
  uint32_t stride_tiles = 0;            // bitmap words per row in every slot
  uint64_t slot_bytes = 0;
  std::vector<uint32_t> shard_reviews;  // [world]
};
void dev_shard_setup(DevTable* t, DevComm* c, uint32_t nc, ShardInfo* info);   // collective: exchanges the shard sizes
// after a finished local evaluation of the shard (dev_eval): the slot's tail <- counts, ONE in-place all-gather of the slots,
// int64 totals <- sums over the gathered tails, on the evaluation stream; then synchronises and copies what was asked for to
// the host.  Slot: [nc][stride_tiles] u64 bitmap | [nc] u32 violating pairs | [nc] u32 autoreject pairs | u64 beyond | u64 not evaluated | pad.
// totals: [nc] violating pairs | [nc] autoreject pairs (match errors) | reviews beyond the engine's limits | reviews not
// evaluated (`not_evaluated` of this rank: rejected by HandleReview when the table was built), each summed over ALL shards --
// what the gathered violation bitmaps cannot say, so that a sharded audit fails closed like the single-GPU one.
// totals == nullptr: ENQUEUE ONLY -- counts, all-gather and totals go onto the stream behind the launches of
// dev_eval_launch and the call returns without waiting (back-to-back sweeps; the collecting call comes last)
void dev_shard_exchange(DevTable* t, DevComm* c, uint32_t nc, uint64_t not_evaluated, std::vector<int64_t>* totals,
                        std::vector<uint64_t>* gathered /* may be null */, const void** d_gathered);
// the exchange step of the most recent COLLECTING dev_shard_exchange of this table (enqueue-only passes are not timed): duration of the
// all-gather alone (events around it on its stream; 0 when no collecting exchange ran), the bytes this rank RECEIVES in it
// ((world - 1) x slot), and whether consecutive enqueue-only passes overlap their exchange with the next sweep
struct ShardExchangeStats { float exchange_ms = 0; uint64_t inbound_bytes = 0; bool overlap = false; };
ShardExchangeStats dev_shard_exchange_stats(const DevTable* t, const DevComm* c);
// one enqueue-only sweep + exchange step of a resident shard (launch + exchange; captured into a graph from the second pass on)
void dev_shard_enqueue(const DevPlan* p, DevTable* t, DevComm* c, const EvalOptions& opt, uint32_t nc, uint64_t not_evaluated, bool allow_graph);
// the answer of the most recent enqueue-only pass, without sweeping again; false when there is none or when that pass left
// reviews to the large-capacity re-run (which only a collecting sweep does)
bool dev_shard_collect(DevTable* t, DevComm* c, uint32_t nc, std::vector<int64_t>* totals, std::vector<uint64_t>* gathered, const void** d_gathered);
// Plan-specialised builds of the dominant kernel run in the background for admission batches (kernels.hip jit_for): wait for
// every build in flight / code-object cache counters (hits = builds served without hiprtc)
void dev_jit_quiesce();
void dev_jit_cache_stats(uint64_t* hits, uint64_t* compiles);
void dev_jit_cache_drop_memory();        // forget the code objects held in memory; the disk cache stays (what a restarted process sees)
const char* dev_jit_cache_dir();         // "" = no disk cache
void dev_jit_prefetch(const DevPlan* p, const DevTable* t);   // start the build this (plan, table) will ask for; never waits
void dev_eval_launch(const DevPlan* p, const DevTable* t, const EvalOptions& opt);          // asynchronous on the default stream
void dev_eval_finish(const DevPlan* p, const DevTable* t, const EvalOptions& opt, EvalOut* out);   // sync, overflow re-run, download

}  // namespace gk
