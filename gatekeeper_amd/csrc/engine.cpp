// Host engine + C ABI (include/gkgpu.h).  Holds templates, constraints, the path dictionary, the Namespace cache
// and data.inventory; builds the device plan lazily; flattens reviews into HBM-resident tables; launches the HIP
// kernels through device.hpp; renders messages for the sparse violating pairs.
//
// Mirrors the state a reference drivers.Driver keeps (pkg/drivers/k8scel/driver.go:60-160) plus the target handler
// pieces that sit on the hot path (pkg/target/target.go:81-179, matcher.go:21-93, ns_cache.go:15-87).
#include <atomic>
#include <cstring>
#include <dirent.h>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <thread>
#include <map>
#include <set>
#include <unordered_map>
#include <unordered_set>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <sstream>

#include "../../include/gkgpu.h"
#include "audit_merge.hpp"
#include "codegen.hpp"
#include "device.hpp"
#include "flatten.hpp"
#include "lower.hpp"
#include "pe.hpp"
#include "regex.hpp"
#include "review_words.hpp"
#include "verify_merge.hpp"
#include "table_stream.hpp"
#include "viol_stream.hpp"
#include "delta_stream.hpp"
#include "table_delta.hpp"

using namespace gk;

static std::atomic<int64_t> g_debug_verify_flip{-1};   // gk_debug_set("verify_flip", v): fault injection for gk_table_verify (gkgpu.h)
static std::atomic<uint32_t> g_debug_kjoin_hash_bits{64};   // gk_debug_set("kjoin_hash_bits", b): the device key join masks its hashes to b bits (gkgpu.h)
static std::atomic<bool> g_debug_keep_slot_index{false};   // gk_debug_set("keep_slot_index", 1): tables created from now on keep the host copy of their slot index (gk_table_review_words)
static std::atomic<int> g_debug_group_max{0};   // gk_debug_set("group_max", n): plan groups of at most n constraints (0 = as many as fit)
namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

std::string lower_str(std::string s) { for (auto& c : s) if (c >= 'A' && c <= 'Z') c += 32; return s; }

struct ConstraintRec {
  uint32_t id;
  std::string kind, name;
  Value object, params, match;
  FP viol;
  MatchFormulas mf;
  std::shared_ptr<const PreparedConstraint> prep;   // simplified / folded once (lower.hpp), reused by every plan build
  // RESULT totals (gk_table_totals): "this review may yield MORE THAN ONE result" (Template::compile_multi) with the same match
  // formulas, lowered into the totals plans; null = not lowerable: every violating pair of the constraint is rendered
  std::shared_ptr<const PreparedConstraint> multi_prep;
  bool multi_ready = false;   // multi_prep is what it will be (possibly null); false: derived by the first gk_table_totals that needs it
                              //   (half of a K8sContainerLimits AddConstraint went into a formula only the audit's RESULT totals read)
  // RESULT COUNTS on the device (round 4; Template::count_forms): rows whose true values sum to the review's number of results
  // + a flag "cannot tell" (rendered).  `cforms` is derived with the violation formula (one evaluation of the template) so that
  // the message-key paths are registered with the flattener at AddConstraint; `count_rows` / `count_flag` are the prepared,
  // trial-lowered forms (first gk_table_totals; empty = this constraint is served by multi_prep as in round 3)
  std::shared_ptr<const Template::CountForms> cforms;
  std::vector<Pattern> count_reads;   // the paths the counting forms' atoms name (publish_read_set: pruned tables must hold their rows)
  std::vector<std::shared_ptr<const PreparedConstraint>> count_rows;
  std::shared_ptr<const PreparedConstraint> count_flag;
  bool count_ready = false;
  // referential template (reads data.inventory): compiled against a snapshot of the synced objects, again whenever they change
  // (refresh_referential); `broken`: why the current inventory does not compile -- every evaluation then fails (GK_ERR_UNSUPPORTED)
  bool referential = false;
  std::string broken;
  bool alive = true;
};

// ---- host-side matcher: only used to produce the exact autoreject message for pairs the device flagged -----------
// pkg/mutation/match/match.go:32-258, pkg/target/matcher.go:44-71
bool wildcard_matches(const std::string& w, const std::string& c) {
  bool pre = !w.empty() && w.front() == '*', suf = !w.empty() && w.back() == '*';
  if (pre && suf) { std::string in = w.substr(1); if (!in.empty() && in.back() == '*') in.pop_back(); return c.find(in) != std::string::npos; }
  if (pre) { std::string s = w.substr(1); return c.size() >= s.size() && c.compare(c.size() - s.size(), s.size(), s) == 0; }
  if (suf) { std::string p = w.substr(0, w.size() - 1); return c.compare(0, p.size(), p) == 0; }
  return w == c;
}

std::string selector_error(const Value& sel) { return selector_error_text(sel); }

// IsNamespaceExcluded for one review (excluder.go:96-105).  Bare objects: the object itself (audit).  AdmissionRequests:
// the webhook's view, common.go:149-189 -- oldObject on DELETE else object, its namespace overwritten by request.namespace;
// an object that does not decode is an error there, which the handler logs and then reviews the request anyway.
bool excluder_matches(const std::vector<std::string>& pats, const std::string& ns);
bool review_excluded(const std::vector<std::string>& pats, int kind, const Value& body) {
  if (!body.is_object()) return false;
  const Value* obj = &body;
  std::string ns;
  if (kind == GK_REVIEW_ADMISSION_REQUEST) {
    const Value* op = body.get("operation");
    const bool del = op && op->is_string() && op->str() == "DELETE";
    obj = body.get(del ? "oldObject" : "object");
    const Value* k = obj && obj->is_object() ? obj->get("kind") : nullptr;
    if (!k || !k->is_string() || k->str().empty()) return false;
    const Value* rns = body.get("namespace");
    if (rns && rns->is_string()) ns = rns->str();
  } else {
    ns = obj_string(*obj, "metadata", "namespace");
  }
  if (obj_is_namespace(*obj)) return excluder_matches(pats, obj_string(*obj, "metadata", "name"));
  return excluder_matches(pats, ns);
}

// exactOrWildcardMatch (excluder.go:120-128)
bool excluder_matches(const std::vector<std::string>& pats, const std::string& ns) {
  for (auto& w : pats) if (wildcard_matches(w, ns)) return true;
  return false;
}

// error text of match.Matches for one candidate object, "" if none (subset: the error sources of match.go)
std::string candidate_error(const Value& m, const Value& obj, const Value& ns, int source, bool* matched) {
  *matched = false;
  std::string g, v, k;
  obj_gvk(obj, &g, &v, &k);
  bool is_ns = k == "Namespace" && g.empty();
  std::string name = obj_string(obj, "metadata", "name"), nsfield = obj_string(obj, "metadata", "namespace");
  auto strs = [](const Value* l) { std::vector<std::string> o; if (l && l->is_array()) for (auto& x : l->items()) if (x.is_string()) o.push_back(x.str()); return o; };
  // kinds
  const Value* kinds = m.get("kinds");
  if (kinds && kinds->is_array() && kinds->size()) {
    bool any = false;
    for (auto& kk : kinds->items()) {
      auto ks = strs(kk.get("kinds")), gs = strs(kk.get("apiGroups"));
      auto has = [](const std::vector<std::string>& l, const std::string& x) { return l.empty() || std::find(l.begin(), l.end(), "*") != l.end() || std::find(l.begin(), l.end(), x) != l.end(); };
      if (has(ks, k) && has(gs, g)) any = true;
    }
    if (!any) return "";
  }
  std::string scope = obj_string(m, "scope");
  bool has_ns = !nsfield.empty() || ns.defined();
  if (scope == "Cluster" && !(is_ns || !has_ns)) return "";
  if (scope == "Namespaced" && !(!is_ns && has_ns)) return "";
  bool has_nsname = true;
  std::string nsname;
  if (is_ns) nsname = name; else if (ns.defined()) nsname = obj_string(ns, "metadata", "name"); else if (!nsfield.empty()) nsname = nsfield; else has_nsname = false;
  auto nss = strs(m.get("namespaces"));
  if (!nss.empty() && has_nsname) { bool any = false; for (auto& w : nss) if (wildcard_matches(w, nsname)) any = true; if (!any) return ""; }
  auto ex = strs(m.get("excludedNamespaces"));
  if (!ex.empty() && has_nsname) for (auto& w : ex) if (wildcard_matches(w, nsname)) return "";
  const Value* ls = m.get("labelSelector");
  if (ls && ls->is_object()) { std::string e = selector_error(*ls); if (!e.empty()) return e; }
  // (label selector truth is decided on the device; for error text we only need to know whether evaluation continues,
  //  which the device already established by flagging this pair)
  const Value* nsel = m.get("namespaceSelector");
  if (nsel && nsel->is_object() && !(!is_ns && !ns.defined() && nsfield.empty())) {
    std::string e = selector_error(*nsel);
    if (!e.empty()) return e;
    if (!is_ns && !ns.defined()) return "namespace selector for namespace-scoped object but missing Namespace";
  }
  std::string src = obj_string(m, "source");
  if (src.empty()) src = "All";
  if (src != "All" && src != "Original" && src != "Generated") return "invalid source field \"" + src + "\"";
  if (source == SRC_EMPTY && src != "All") return "source field not specified for resource " + name;
  if (src != "All" && source == SRC_INVALID) return "invalid source field";
  *matched = true;
  return "";
}

std::string autoreject_message(const Value& match, const ReviewDoc& doc) {
  const Value* obj = doc.request.get("object");
  const Value* old = doc.request.get("oldObject");
  // gkReviewToObject (matcher.go:73-93): object first, then oldObject; the raw bytes are echoed (here: compact,
  // key-sorted JSON of the parsed document)
  if (obj && obj->is_object() && obj_string(*obj, "kind").empty())
    return "unable to match constraints: invalid request object: failed to unmarshal gkReview object " + to_json(*obj);
  if (old && old->is_object() && obj_string(*old, "kind").empty())
    return "unable to match constraints: invalid request object: failed to unmarshal gkReview oldObject " + to_json(*old);
  bool any = false;
  for (const Value* c : {obj, old}) {
    if (!c || !c->is_object()) continue;
    any = true;
    bool matched;
    std::string e = candidate_error(match, *c, doc.match_ns, doc.source, &matched);
    if (!e.empty())
      return "unable to match constraints: error matching the requested object: " + obj_string(*c, "metadata", "name") +
             " :failed to run Match criteria: " + e;
    if (matched) break;
  }
  if (!any) return "unable to match constraints: invalid request object: neither object nor old object are defined";
  return "unable to match constraints: error matching the requested object";
}

}  // namespace

// Persistent host workers for table builds.  A 64k-review batch gives each of 128 threads ~3 ms of flattening: spawning and
// joining the threads per table cost more than the work (round 2: 4.6x on 256 threads).  The pool is process-wide and sized
// to the hardware; run(n, fn) executes fn(0..n-1) on the workers and the caller, returns when all are done.  Concurrent
// run() calls (the batcher's workers) are served one after the other.
class HostWorkers {
 public:
  static HostWorkers& get() { static HostWorkers w; return w; }
  void run(size_t n, const std::function<void(size_t)>& fn) {
    if (n <= 1) { if (n) fn(0); return; }
    std::lock_guard<std::mutex> serial(run_mu_);
    {
      std::lock_guard<std::mutex> l(mu_);
      while (threads_.size() + 1 < n && threads_.size() < max_) threads_.emplace_back([this] { loop(); });
      fn_ = &fn; n_ = n; next_ = 0; done_ = 0; gen_++;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> l(mu_);
    done_cv_.wait(l, [&] { return done_ == n_; });
    fn_ = nullptr;
  }
  ~HostWorkers() {
    { std::lock_guard<std::mutex> l(mu_); stop_ = true; }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
  }
 private:
  HostWorkers() : max_(std::max<size_t>(1, std::thread::hardware_concurrency())) {}   // (a ceiling: callers ask for host_cpus() workers unless GK_HOST_THREADS says otherwise)
  void work() {
    for (;;) {
      size_t i;
      const std::function<void(size_t)>* fn;
      {
        std::lock_guard<std::mutex> l(mu_);
        if (!fn_ || next_ >= n_) return;
        i = next_++;
        fn = fn_;
      }
      (*fn)(i);
      std::lock_guard<std::mutex> l(mu_);
      if (++done_ == n_) done_cv_.notify_all();
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return stop_ || (gen_ != seen && fn_ && next_ < n_); });
        if (stop_) return;
        seen = gen_;
      }
      work();
    }
  }
  std::mutex mu_, run_mu_;
  std::condition_variable cv_, done_cv_;
  std::vector<std::thread> threads_;
  const std::function<void(size_t)>* fn_ = nullptr;
  size_t n_ = 0, next_ = 0, done_ = 0, max_;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

static std::atomic<uint64_t> g_engine_uid{1};
struct gk_engine {
  const uint64_t uid = g_engine_uid++;   // (per-thread caches are keyed by it: an address may be reused by a later engine)
  gk_opts opts{};
  std::set<std::string> disabled_builtins{"http.send"};   // rego.DisableBuiltins (gk_opts.disabled_builtins; the deployment's default)
  PathDict dict;
  DictRegistry dict_reg;     // leaf-local expressions of the loaded constraints (dexpr.hpp): evaluated by the flattener
  NsCache ns_cache;
  std::shared_mutex mu;   // templates / constraints / inventory
  std::map<std::string, std::shared_ptr<Template>> templates;   // lower(kind)
  std::vector<ConstraintRec> constraints;
  // data.inventory (pkg/target/target.go:40-79 ProcessData: namespace/<ns>/<gv>/<Kind>/<name>, cluster/<gv>/<Kind>/<name>).  Kept only
  // while a loaded constraint's template reads it (inv_tracking): inv_store mirrors gk_data_put / gk_data_remove, `inventory` is
  // the document built from it (generation inv_built), and the referential constraints are compiled against it as a CONSTANT --
  // again whenever it changes (inv_gen vs inv_compiled; refresh_referential, called by ensure_plan).
  Value inventory = Value::object({});
  bool inv_tracking = false;
  std::map<std::string, std::pair<std::vector<std::string>, std::string>> inv_store;   // key -> (path, JSON text)
  uint64_t inv_gen = 1, inv_built = 0, inv_compiled = 0;
  int next_quant = 0;
  // process excluder (pkg/controller/config/process/excluder.go): process -> namespace wildcards, replaced as a whole
  // from the Config resource's spec.match; `excluder_gen` lets resident chunks notice a change (guarded by mu)
  std::map<std::string, std::vector<std::string>> excluder;
  uint64_t excluder_gen = 1;
  // plan cache
  // Plans are read by every evaluation and replaced when the policy set (or the path dictionary) changes.  Evaluations of
  // DIFFERENT tables run side by side -- each holds plan_rw shared for as long as its launches use the plan (the batcher's
  // workers, a streamed batch being evaluated while the next one is uploaded) --; whoever replaces or walks the plans
  // takes it exclusively.  plan_gate is a turnstile in front of the shared side, so that a waiting writer is not starved by
  // a steady stream of readers; variants_mu guards the table-specialised variants, which evaluations create on demand.
  std::shared_mutex plan_rw;
  std::mutex plan_gate, variants_mu;
  // POLICY EPOCH: Driver.Query holds the driver's read lock for the whole call and AddTemplate / AddConstraint / Remove* its write
  // lock (pkg/drivers/k8scel/driver.go:61,131,140,168-169) -- a query never sees a policy set change between its two halves.  Here
  // an admission batch is flattened for the policy set loaded now (a pruned table) and evaluated a moment later: the batcher holds
  // this lock shared around the two steps, the four policy mutators take it exclusively (policy_gate: the turnstile that keeps a
  // waiting writer from being starved by back-to-back batches).  Nothing else takes it, so it nests with no other lock order.
  std::shared_mutex policy_rw;
  std::mutex policy_gate;
  bool plan_dirty = true;
  uint64_t plan_gen = 0;   // bumped whenever the device plan (and with it every variant) is rebuilt
  // A plan holds a limited number of distinct violation / match formulas (one result bit each) and element scopes.  A constraint
  // set that does not fit one plan is split into PLAN GROUPS: `groups` holds one entry per group, groups[0] the primary plan, never
  // empty once ensure_plan has run (an empty policy set is one group without constraints).  The groups are evaluated over the same
  // table, each into its own side of it (gk_table::Side: result buffers + path binding), and their bitmap rows are appended in list
  // order, so callers see one [n_constraints][n_tiles] answer.  Behind unique_ptr: tables cache `const HostPlan*` into a group.
  struct Group { HostPlan fast, big; DevPlan* dev = nullptr; std::vector<uint32_t> ids; std::vector<uint8_t> roles; };   // ids: bitmap row -> constraint id; roles: totals groups only (TR_*)
  std::vector<std::unique_ptr<Group>> groups;
  // table-specialised variants of a group's fast plan (GK_TABLE_RESIDENT): same formulas, element capacities = what the
  // table's largest arrays need, so the per-review LDS footprint (hence occupancy) fits the data
  struct Variant { HostPlan fast; DevPlan* dev = nullptr; };
  std::map<std::pair<size_t, std::vector<uint16_t>>, std::unique_ptr<Variant>> variants;   // key: (plan group, capacities)
  // plan groups (0 = the primary plan) that gk_table_verify took off the plan-specialised kernel (GK_VERIFY_QUARANTINE): every DevPlan of
  // such a group -- the base plan, its table-sized variants, their re-uploads when the dictionary grows -- is served by the bytecode kernel
  // until the policy set is compiled again.  Written under plan_rw exclusively.
  std::set<size_t> quarantined;
  // plans of the "more than one result" formulas (ConstraintRec::multi_prep), evaluated by gk_table_totals only; built on its
  // first call after a policy change (totals_gen = the plan generation they belong to; guarded by totals_mu, plan_rw shared)
  std::vector<std::unique_ptr<Group>> totals_groups;
  uint64_t totals_gen = ~0ull;
  std::mutex totals_mu;
  std::string last_dump;
  DevComm* comm = nullptr;   // multi-GPU exchange (gk_comm_init)
  // ---- resident set (row f2): every object synced through gk_data_put, flattened in HBM in chunks
  struct ResObj {
    std::vector<std::string> path;
    std::string key, json, ns;        // ns: the namespace the object lives in ("" = cluster scoped)
    bool is_namespace = false, alive = true;
    uint32_t chunk = UINT32_MAX, slot = 0;
  };
  struct ResChunk {
    gk_table* table = nullptr;
    std::vector<uint32_t> obj_of_slot;
    std::vector<uint64_t> live;       // bit per slot: still the current version of a live object
    std::vector<uint64_t> shown;      // live AND NOT excluded from the audit process by the excluder generation `excl_gen`
    uint64_t excl_gen = 0;
    uint64_t shown_gen = 0;           // moves whenever the contents of `shown` change (the device copy follows it: dev_audit_select)
    // gk_resident_audit's autoreject side, kept while the evaluation (err_plan_gen) and the mask (err_shown_gen) stay as they are: per bitmap
    // row the shown pairs whose Matcher.Match failed, and the slots of the first err_k of them in key order (+ the key ties of the last)
    std::vector<uint64_t> err_pairs;
    std::vector<std::vector<uint32_t>> err_slots;
    uint64_t err_plan_gen = 0, err_shown_gen = 0;
    uint32_t err_k = 0;
    // gk_resident_violations' index, kept like the err_* fields while the evaluation (vs_plan_gen) and the mask (vs_shown_gen) stand:
    // vs_prefix = exclusive prefix sum of the entries per bitmap word over ALL sources (device bits of every plan group, autoreject
    // bits, host-evaluated violations); vs_host_slots = the shown slots that have an autoreject bit or a host-evaluated violation, ascending
    std::vector<uint64_t> vs_prefix;
    std::vector<uint32_t> vs_host_slots;
    uint64_t vs_plan_gen = 0, vs_shown_gen = 0;
    // gk_resident_changes.  The BASELINE of the chunk (cs_has_base: the chunk existed when the last changes stream was handed out
    // completely): the device keeps a copy of every plan group's violation bitmap and of the shown mask beside the group's side
    // (dev_delta_keep); here the mask's host copy and the pairs no device bitmap carries -- autoreject pairs, violating pairs the host
    // evaluator completed -- as sorted (slot, row) lists under that mask.  The index of the stream (kept like vs_*, and while the
    // baseline cs_base_gen and the reset state cs_reset it was built against stand): cs_changed = the slots with an entry per bitmap
    // word over ALL sources, cs_prefix its exclusive prefix sum, cs_now_* = the pairs as they are now, cs_merged = an entry may come
    // from more than one source (several plan groups, host pairs that differ): every group then emits the merged words' slots.
    bool cs_has_base = false;
    std::vector<uint64_t> cs_base_shown;
    std::vector<std::pair<uint32_t, uint32_t>> cs_base_err, cs_base_hviol, cs_now_err, cs_now_hviol;
    std::vector<uint64_t> cs_prefix, cs_changed;
    bool cs_merged = false, cs_reset = false;
    uint64_t cs_plan_gen = 0, cs_shown_gen = 0, cs_base_gen = 0;
    gk_eval_out* ev = nullptr;       // bitmaps of the chunk's most recent evaluation
    uint64_t plan_gen = 0;            // ... and the plan generation they belong to
    uint64_t n_live = 0;
  };
  struct Resident {
    std::mutex mu;
    std::vector<ResObj> objs;
    std::unordered_map<std::string, uint32_t> by_key;
    std::unordered_map<std::string, std::vector<uint32_t>> by_ns;   // namespace -> objects living in it
    std::unordered_map<uint64_t, uint32_t> by_text;                 // hash of the JSON text -> object (gk_query's shortcut)
    std::vector<uint32_t> pending;                                   // objects to (re)flatten at the next sweep
    std::vector<ResChunk> chunks;
    bool swept = false;               // bitmaps are current (no put / remove / policy change since the last sweep)
    uint64_t n_live = 0, n_dead_slots = 0, flattened_total = 0;
    // gk_resident_violations: set_gen moves with every put / remove that changes the set, compactions with every time the chunks are
    // flattened again; vs_* is the state the stream generation vs_gen (0: no stream yet) was handed out for
    uint64_t set_gen = 0, compactions = 0;
    uint32_t vs_gen = 0;
    uint64_t vs_set_gen = 0, vs_compactions = 0, vs_plan_gen = 0, vs_excl_gen = 0;
    // gk_resident_changes: stream generation fields of its own (the two streams do not invalidate each other), the reset state of the
    // stream cs_gen stands for, and the baseline: cs_base_gen counts the commits (0: none yet), cs_base_compactions / cs_base_ids say
    // what it is comparable with (ids: per plan group the constraint ids in bitmap-row order)
    uint32_t cs_gen = 0;
    uint64_t cs_set_gen = 0, cs_compactions = 0, cs_plan_gen = 0, cs_excl_gen = 0;
    bool cs_reset = false;
    uint64_t cs_base_gen = 0, cs_base_compactions = 0, cs_stream_base_gen = 0;
    std::vector<std::vector<uint32_t>> cs_base_ids;
  } resident;
  // ---- admission micro-batcher (gk_query): concurrent single-review calls coalesced into one table + one launch
  struct BatchResult;   // one evaluated batch: table + bitmaps, shared by its requests until the last one has rendered
  struct Request {
    const gk_review_in* in = nullptr;
    bool pre_matched = false;               // GK_QUERY_PRE_MATCHED: the review's RF_PREMATCHED bit in the batch's table
    std::chrono::steady_clock::time_point arrived;
    int status = GK_OK;
    std::string error;
    std::shared_ptr<BatchResult> batch;   // results are rendered by the CALLER's thread from its column of the bitmaps
    uint32_t index = 0;
    uint32_t batch_size = 0;
    double queue_us = 0, device_us = 0;
    bool done = false;
    std::condition_variable cv;
  };
  struct Batcher {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Request*> queue;
    std::vector<std::thread> workers;   // each takes whole batches: one flattens while another's launch is on the device
    bool running = false, stop = false;
    gk_batch_opts opts{64, 200, 0, 0};
    uint64_t batches = 0, reviews = 0;
  } batcher;
};

struct gk_table {
  gk_engine* eng;
  DevTable* dev = nullptr;
  HostTable host;               // rows/heap released after upload unless needed
  std::vector<ReviewDoc> docs;  // GK_TABLE_KEEP_DOCS
  std::vector<gk_review_in> texts;   // GK_TABLE_KEEP_TEXT: where each review's JSON lives (caller-owned text)
  std::shared_ptr<void> owned_text;  // gk_table_create_spool: the table owns the spooled text its `texts` point into
  std::vector<std::string> review_errors;
  uint64_t n_rejected = ~0ull;              // non-empty review_errors (counted by the first sharded sweep)
  uint64_t dir_bytes = 0, n_rows = 0;      // review-flag bytes (read by every launch); rows in the table
  std::vector<uint32_t> path_rows;          // rows per path: which rows a plan reads
  std::vector<uint32_t> path_max;           // per element path: largest array of one review
  // What the table keeps per plan group (gk_engine::groups), indexed like it.  sides[0] is there from the start and evaluates into the
  // table itself; a further side is a view of the table (shares the device arrays of `dev`), made by whoever first needs it
  // (table_sides).  Sides only grow in number and go with the table.
  struct Side {
    DevTable* dev = nullptr;                // what the group evaluates into: `dev` of the table (side 0) or a view of it
    ShardInfo shard;                        // sharded sweeps: slot layout agreed with the other ranks
    DevTable* vview = nullptr;              // the bytecode side of gk_table_verify (created by its first call)
    DevPlan* vtwin = nullptr;               // ... and the plan it evaluates where the backend wants a plan of its own for it (dev_verify_twin;
    uint64_t vtwin_gen = 0;                 //     nullptr on the device), of plan generation vtwin_gen
    DevPlan* plan = nullptr;                // the plan this table runs the group on (plan_for_group), of plan generation cached_gen ...
    const HostPlan* host = nullptr;         // ... and its host form
  };
  std::vector<Side> sides;
  std::vector<DevTable*> tviews;            // one per totals plan group (gk_table_totals)
  bool resident = false;
  bool any_prematched = false;              // some review carries RF_PREMATCHED (host.rflags says which)
  uint64_t cached_gen = 0;                  // plan generation the sides' plan choices belong to
  std::vector<uint32_t> slot_path;          // path of each slot of the table's row-group index
  // per review: group \0 version \0 kind \0 namespace \0 name (audit order, manager.go:118-138) -- the bytes in one arena per host
  // thread's part, (offset, length) per review: a std::string per review was a malloc and a free per review
  std::vector<std::string> key_arena;
  std::vector<std::pair<uint32_t, uint32_t>> key_span;
  size_t key_per_part = 1;
  std::string_view obj_key(size_t i) const { const auto& sp = key_span[i]; return std::string_view(key_arena[i / key_per_part].data() + sp.first, sp.second); }
  std::vector<uint32_t> order, grp;         // reviews sorted by obj_keys / dense rank with ties equal (built by the first gk_table_topk)
  uint32_t last_nc = 0;
  std::vector<uint32_t> last_ids;
  // Reviews that may end up beyond the device's limits (RF_TOO_BIG / RF_REFUSE / RF_HOST_CAND at flatten time): their text is kept
  // whatever the table's flags, so that gk_table_eval can evaluate them on the host (complete_on_host) instead of refusing them
  struct OwnedReview {
    int32_t kind = 0, source = 0;
    std::string json, ns, nsobj, op;
    bool has_ns = false, has_nsobj = false, has_op = false;
    gk_review_in in() const {
      gk_review_in r{};
      r.kind = kind; r.source = source; r.json = json.data(); r.json_len = json.size();
      r.namespace_json = has_ns ? ns.data() : nullptr; r.namespace_len = has_ns ? ns.size() : 0;
      r.ns_object_json = has_nsobj ? nsobj.data() : nullptr; r.ns_object_len = has_nsobj ? nsobj.size() : 0;
      r.operation = has_op ? op.c_str() : nullptr;
      return r;
    }
  };
  std::map<uint32_t, OwnedReview> big_texts;
  std::mutex big_mu;
  // (row, review) pairs the host evaluation of the most recent gk_table_eval added: violations / autoreject errors the device
  // bitmaps do not hold (gk_table_totals and gk_table_topk read those)
  // (stamped with the constraint-id list of that evaluation: a reader whose own list differs -- a policy change renumbered the rows --
  //  drops them; host_mu orders the evaluation that writes them and the totals / top-k calls that read them)
  std::vector<std::pair<uint32_t, uint32_t>> host_viol, host_err;
  std::vector<uint32_t> host_ids;
  std::mutex host_mu;
  // gk_table_violations.  ts_gen, the stream generation, moves with every launch that writes the table's result buffers (table_results_move:
  // evaluation, verification, a sharded sweep): a cursor carries it.  The host evaluation stamps what it publishes -- host_done, the
  // reviews it answered, beside host_viol / host_err -- with the generation of ITS evaluation (host_gen): the stream of a later
  // evaluation that did not complete on the host (GK_EVAL_NO_DOWNLOAD) reads none of them.  eval_plan_gen: the plan generation the
  // bitmaps belong to (0: never collected); ts_pending: GK_EVAL_ASYNC launches wait to be collected.  The index is kept while ts_gen
  // stands (ts_index_gen): ts_prefix over all entries (table_stream.hpp), ts_dev_off over the device's alone (places its entries).
  uint32_t ts_gen = 0, host_gen = 0, ts_index_gen = 0;
  uint64_t eval_plan_gen = 0, ts_beyond = 0;
  bool ts_pending = false;
  std::vector<uint32_t> host_done, ts_dev_off;
  std::vector<uint64_t> ts_prefix;
  // gk_table_changes: the state of the stream begun by the last call with cursor 0, valid while ts_gen stands (tc.gen) -- per side
  // (0: the table's reviews, 1: the snapshot's gone ones) what the device lined up (freed when the result buffers move or the table
  // goes), the index (table_delta.hpp), the host-known reviews and what the device is told of them
  struct Changes {
    uint32_t gen = 0, flags = 0;            // (flags: as given at cursor 0)
    uint64_t snap_serial = 0;               // the snapshot the stream compares with (0: none, a reset stream)
    DevAligned* aligned[2] = {nullptr, nullptr};
    uint32_t n[2] = {0, 0};
    std::vector<uint64_t> prefix[2], drop[2], extra[2], moved;
    DeltaKnownMap known[2];
    std::vector<uint32_t> then_of;
    uint64_t beyond = 0;
    bool joined = false;                    // the stream has a snapshot: `join` says how the two sides were joined (gk_table_changes_join)
    KjoinStats join;
    float join_ms = 0;
  } tc;
  // the table's keys as packed records on the device (key_join.hpp), put there by the first device join and kept with the table;
  // keys_unfit: they do not fit 32-bit offsets, every join of this table runs on the host
  DevKeys* dkeys = nullptr;
  bool keys_unfit = false;
  std::mutex keys_mu;
  uint32_t n_reviews = 0;
  uint32_t rpt = GK_RPT_MIN;                // reviews per row group of this table
  uint64_t dict_gen = 0;                    // generation of the dictionary-predicate registry the rows were flattened under
  bool pruned = false;                      // GK_TABLE_PRUNED: rows of the registry's read set only ...
  uint64_t reads_gen = 0;                   // ... as it was when the table was built (DictRegistry::reads_gen)
  uint64_t shard_gen = 0;                   // plan generation the sides' shard layouts were agreed for
  gk_table_stats stats{};
};

namespace {

Value set_in(const Value& root, const std::vector<std::string>& path, size_t i, const Value* leaf) {
  // returns a copy of root with path[i..] set to *leaf (or removed when leaf == nullptr)
  ValuePairs p = root.is_object() ? root.pairs() : ValuePairs{};
  Value key = Value::string(path[i]);
  ValuePairs out;
  bool done = false;
  for (auto& kv : p) {
    if (kv.first == key) {
      done = true;
      if (i + 1 == path.size()) { if (leaf) out.emplace_back(key, *leaf); }
      else out.emplace_back(key, set_in(kv.second, path, i + 1, leaf));
    } else out.push_back(kv);
  }
  if (!done && leaf) {
    if (i + 1 == path.size()) out.emplace_back(key, *leaf);
    else out.emplace_back(key, set_in(Value::object({}), path, i + 1, leaf));
  }
  return Value::object(out);
}

PlanCaps default_caps(const gk_engine* e) {
  PlanCaps caps;
  for (int i = 0; i < 3; i++) if (e->opts.elem_cap[i]) caps.level_cap[i] = e->opts.elem_cap[i];
  return caps;
}

// ---- plan groups: the engine's list (gk_engine::groups), a table's sides of them (gk_table::sides).  Every entry point that works
// group by group goes through these; all of them want plan_rw held (shared suffices).

// (the first group's answer is taken over as it is, the others' rows are appended)
template <class T> void append(std::vector<T>& to, std::vector<T>&& from) {
  if (to.empty()) to = std::move(from); else to.insert(to.end(), from.begin(), from.end());
}

// the constraint id of every bitmap row: the groups' ids in list order
std::vector<uint32_t> all_ids(const gk_engine* e) {
  std::vector<uint32_t> ids;
  for (auto& g : e->groups) ids.insert(ids.end(), g->ids.begin(), g->ids.end());
  return ids;
}

// a side of the table for every plan group there is now
void table_sides(const gk_engine* e, gk_table* t) {
  while (t->sides.size() < e->groups.size()) { gk_table::Side s; s.dev = dev_table_view(t->dev); t->sides.push_back(s); }
}

// a launch is about to write the table's result buffers (or a collecting call to finish them): gk_table_violations' stream generation
// moves, so that no cursor handed out before is answered from the new bitmaps
void table_changes_drop(gk_table* t) {
  for (DevAligned*& a : t->tc.aligned) { dev_tchg_free(a); a = nullptr; }
  t->tc = gk_table::Changes();
}
void table_results_move(gk_table* t) { t->ts_gen = viol_next_gen(t->ts_gen); if (t->tc.gen || t->tc.aligned[0] || t->tc.aligned[1]) table_changes_drop(t); }

// One plan group as seen from one table: the engine's group `grp` (its base plan: grp.dev), the table's side of it (what it evaluates
// into: side.dev; the plan this table runs it on, once table_plans chose it: side.plan), its number of bitmap rows and its first row
// among all constraints.  each_group visits, in row order, the groups present on BOTH the engine and the table: a table that has not
// been evaluated under this many groups simply lacks the later sides, the walk ends there, and the callers' size checks turn the short
// answer into "evaluate the table first".
struct GroupAt { size_t g; const gk_engine::Group& grp; gk_table::Side& side; uint32_t nc, row0; };
template <class F> void each_group(const gk_engine* e, gk_table* t, F&& f) {
  uint32_t row0 = 0;
  for (size_t g = 0; g < e->groups.size() && g < t->sides.size(); g++) {
    const uint32_t nc = (uint32_t)e->groups[g]->ids.size();
    f(GroupAt{g, *e->groups[g], t->sides[g], nc, row0});
    row0 += nc;
  }
}

// The plan one table runs one group on, kept in the group's side while the plan generation stands (per launch: no rescan).  Resident
// tables (audit sets evaluated again and again) get a variant whose element capacities are what the table's largest arrays need: fewer
// accumulator words per review -> more tiles resident per CU, and reviews that would overflow the default capacities stay on the LDS
// kernel; every group has variants of its own (key: group, capacities).  Any other table runs the group's base plan.  Caller holds
// plan_rw (shared suffices) and variants_mu; ensure_plan and table_sides ran.
DevPlan* plan_for_group(gk_engine* e, gk_table* t, size_t group) {
  const gk_engine::Group& G = *e->groups[group];
  gk_table::Side& S = t->sides[group];
  if (t->cached_gen != e->plan_gen) { for (gk_table::Side& s : t->sides) { s.plan = nullptr; s.host = nullptr; } t->cached_gen = e->plan_gen; }
  if (S.plan) return S.plan;
  const HostPlan& base = G.fast;
  S.plan = G.dev; S.host = &base;
  if (!t->resident || base.scopes.empty()) return S.plan;
  std::vector<uint16_t> caps(base.scopes.size(), 1);
  for (size_t p = 0; p < base.ptab.size(); p++) {
    uint32_t ent = base.ptab[p];
    for (uint32_t j = 0; j < (ent & 0xFF); j++) {
      const Pred& pr = base.path_preds[(ent >> 8) + j];
      if (pr.op != P_PRESENT || pr.dst != D_ELEM) continue;
      uint32_t need = p < t->path_max.size() ? t->path_max[p] : 0;
      // (the marker rides on a member of the element -- plan.hpp T_ABSENT: the element count is the element path's, its parent)
      if (const PathDict::Info in = e->dict.info((uint32_t)p); !in.is_elem && in.parent < t->path_max.size()) need = std::max(need, t->path_max[in.parent]);
      if (need > caps[pr.scope]) caps[pr.scope] = (uint16_t)std::min<uint32_t>(need, 255);
    }
  }
  static const uint16_t steps[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 255};
  for (auto& c : caps) for (uint16_t s : steps) if (s >= c) { c = s; break; }
  const std::pair<size_t, std::vector<uint16_t>> key(group, caps);
  auto it = e->variants.find(key);
  if (it == e->variants.end()) {
    std::unique_ptr<gk_engine::Variant> v(new gk_engine::Variant());
    try {
      PlanBuilder pb(&e->dict, &e->dict_reg);
      for (uint32_t id : G.ids) pb.add_constraint(e->constraints[id].prep);
      PlanCaps pc = default_caps(e);
      pc.scope_cap = caps;
      v->fast = pb.build(pc);
      if (v->fast.scopes.size() != base.scopes.size()) throw std::runtime_error("scope layout changed");
      v->dev = dev_plan_upload(e->opts.device, v->fast, G.big);
      if (e->quarantined.count(group)) dev_plan_no_jit(v->dev);
    } catch (const std::exception&) { v->dev = nullptr; }   // e.g. LDS limit: the default plan serves the table
    it = e->variants.emplace(key, std::move(v)).first;
  }
  if (it->second->dev) { S.plan = it->second->dev; S.host = &it->second->fast; }
  return S.plan;
}

// the table's side of every plan group and the plan it runs the group on: what an entry point that evaluates every group calls first
void table_plans(gk_engine* e, gk_table* t) {
  table_sides(e, t);
  std::lock_guard<std::mutex> vl(e->variants_mu);
  for (size_t g = 0; g < e->groups.size(); g++) plan_for_group(e, t, g);
}

// Why a table cannot be evaluated under the registry as it is now (nullptr: it can): rows the plans read were not made when it was flattened
const char* table_stale(const gk_engine* e, const gk_table* t) {
  if (t->dict_gen != e->dict_reg.gen())
    return "the table was flattened before a constraint with dictionary predicates was added (its <leaf>.$d rows are missing): create it again";
  if (t->pruned && t->reads_gen != e->dict_reg.reads_gen())
    return "the pruned table was flattened before a constraint that reads other key paths was added (GK_TABLE_PRUNED): create it again";
  return nullptr;
}

void refresh_referential(gk_engine* e);
// The READ SET of pruned tables (GK_TABLE_PRUNED; flatten.hpp DictRegistry::set_reads): every path pattern some plan has a predicate
// on -- all plan groups, both capacities -- plus the paths the constraints' counting forms name (their plans are built at the
// first gk_table_totals, after the tables).  Caller holds plan_rw exclusively and mu shared (ensure_plan).
void publish_read_set(gk_engine* e) {
  std::vector<Pattern> pats;
  auto take = [&](const HostPlan& hp) { pats.insert(pats.end(), hp.pred_patterns.begin(), hp.pred_patterns.end()); };
  for (auto& g : e->groups) { take(g->fast); take(g->big); }
  for (auto& c : e->constraints) if (c.alive) pats.insert(pats.end(), c.count_reads.begin(), c.count_reads.end());
  e->dict_reg.set_reads(pats);
}

// the plans are what the policy set and the path dictionary ask for (caller holds plan_rw and mu, shared suffices)
bool plan_current(const gk_engine* e) {
  if (e->plan_dirty || e->groups.empty() || e->groups[0]->fast.dict_size != e->dict.size()) return false;
  for (auto& g : e->groups) if (!g->dev) return false;
  return true;
}

void ensure_plan(gk_engine* e) {
  refresh_referential(e);   // referential constraints follow the synced inventory (no-op unless one is loaded and it changed)
  {   // the usual case: nothing changed -- decided without keeping other evaluations out
    std::shared_lock<std::shared_mutex> pl(e->plan_rw);
    std::shared_lock<std::shared_mutex> rl(e->mu);
    if (plan_current(e)) return;
  }
  std::lock_guard<std::mutex> gate(e->plan_gate);
  std::unique_lock<std::shared_mutex> l(e->plan_rw);
  std::shared_lock<std::shared_mutex> rl(e->mu);
  if (plan_current(e)) return;
  for (auto& v : e->variants) dev_plan_free(v.second->dev);
  e->variants.clear();
  PlanCaps bigcaps;
  bigcaps.level_cap[0] = bigcaps.level_cap[1] = bigcaps.level_cap[2] = 256;
  if (e->plan_dirty || e->groups.empty()) {
    std::vector<const ConstraintRec*> alive;
    for (auto& c : e->constraints) if (c.alive) alive.push_back(&c);
    for (auto* c : alive) if (!c->broken.empty()) throw Unsupported(c->broken);   // (a referential constraint the current inventory does not compile for)
    // groups of constraints that fit one plan: everything if possible, else chunks of <= GK_MAX_VIOL constraints (a constraint
    // contributes one violation and one match formula), halved further while a chunk still does not lower.  The new list replaces the
    // old one when all of it is built.
    std::vector<std::unique_ptr<gk_engine::Group>> next;
    auto build = [&](const std::vector<const ConstraintRec*>& g) {
      std::unique_ptr<gk_engine::Group> grp(new gk_engine::Group());
      PlanBuilder pb(&e->dict, &e->dict_reg);
      for (auto* c : g) { pb.add_constraint(c->prep); grp->ids.push_back(c->id); }
      grp->fast = pb.build(default_caps(e));
      grp->big = pb.build(bigcaps);
      next.push_back(std::move(grp));
    };
    std::function<void(const std::vector<const ConstraintRec*>&)> place = [&](const std::vector<const ConstraintRec*>& g) {
      // (test / tuning aid, gk_debug_set("group_max", n): no plan group of more than n constraints -- the several-group machinery,
      //  which a set of more than 256 distinct violation formulas still takes, stays testable with a small corpus)
      if (const int forced = g_debug_group_max.load(); forced > 0 && g.size() > (size_t)forced) {
        for (size_t i = 0; i < g.size(); i += (size_t)forced)
          place(std::vector<const ConstraintRec*>(g.begin() + i, g.begin() + std::min(g.size(), i + (size_t)forced)));
        return;
      }
      try { build(g); }
      catch (const Unsupported& u) {
        if (g.size() == 1 && g[0]->referential)   // (its formula follows the synced objects: say so -- the same words refresh_referential uses)
          throw Unsupported(std::string("referential constraint ") + g[0]->kind + "/" + g[0]->name + " does not compile against the synced inventory: " + u.what());
        if (g.size() <= 1) throw;
        size_t cap = GK_MAX_VIOL;   // (a constraint contributes at most one violation formula; round 6: 256 slots per plan, 64 before)
        if (const char* gm = getenv("GK_GROUP_MAX")) cap = (size_t)std::max(1, std::min((int)GK_MAX_VIOL, atoi(gm)));   // tuning aid: smaller plan groups (smaller code objects, fewer accumulator words, more walks of the table)
        size_t half = g.size() > cap ? cap : g.size() / 2;
        for (size_t i = 0; i < g.size(); i += half)
          place(std::vector<const ConstraintRec*>(g.begin() + i, g.begin() + std::min(g.size(), i + half)));
      }
    };
    place(alive);
    if (next.empty()) build({});   // (an empty policy set: one group without constraints)
    for (auto& g : e->groups) dev_plan_free(g->dev);
    e->groups = std::move(next);
    e->quarantined.clear();   // (new plans, new generated text: specialised afresh, to be verified afresh)
  } else {
    try {
      for (auto& g : e->groups) { g->fast.resolve_paths(e->dict); g->big.resolve_paths(e->dict); }
    } catch (const Unsupported& u) {
      // the plan was built before the table's key paths were known and does not fit them: with a referential constraint loaded
      // that is its unrolled inventory (one predicate per synced value on the joined path) -- say so
      for (auto& c : e->constraints) if (c.alive && c.referential)
        throw Unsupported(std::string("referential constraint ") + c.kind + "/" + c.name + " does not compile against the synced inventory: " + u.what());
      throw;
    }
  }
  for (auto& g : e->groups) {
    if (g->dev) { dev_plan_free(g->dev); g->dev = nullptr; }
    g->dev = dev_plan_upload(e->opts.device, g->fast, g->big);
  }
  for (size_t g : e->quarantined) if (g < e->groups.size()) dev_plan_no_jit(e->groups[g]->dev);
  e->plan_gen++;
  e->plan_dirty = false;
  publish_read_set(e);
}

Value parse_opt(const char* p, size_t n) { return (p && n) ? parse_json(p, n) : Value(); }

// thresholds per counted iteration: "at least k elements fire", k = 2 .. GK_COUNT_KMAX (one more flags the review); GK_COUNT_KMAX=0
// switches the device-side result counting off (round 3's "more than one result?" decision serves alone)
enum : uint8_t { TR_MULTI = 0, TR_FLAG = 1, TR_COUNT = 2 };   // what a row of a totals plan answers (gk_engine::Group::roles)
int count_kmax() { return getenv("GK_COUNT_KMAX") ? atoi(getenv("GK_COUNT_KMAX")) : 4; }   // (read per call: a test switches it within one process)

// The counting forms of a constraint from the evaluation that gave its violation formula; registers the message-key paths with
// the flattener (caller holds mu exclusively: a new key path makes the tables flattened so far stale, like a new value path)
std::shared_ptr<const Template::CountForms> derive_count_forms(gk_engine* e, const Template::CountInfo& ci, const MatchFormulas& mf, FP* merged_viol = nullptr,
                                                                 std::vector<Pattern>* reads = nullptr) {
  if (reads) reads->clear();
  if (count_kmax() < 2) return nullptr;
  try {
    const auto tf0 = std::chrono::steady_clock::now();
    auto cf = std::make_shared<Template::CountForms>(Template::count_forms(ci, count_kmax()));
    if (getenv("GK_DEBUG_LOAD")) fprintf(stderr, "[gkgpu load]   count_forms %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - tf0).count());
    if (merged_viol && cf->viol && ci.br.size() > 8) *merged_viol = cf->viol;   // (a constraint with many unrolled alternatives: the merged form is the smaller formula)
    if (!cf->ok) return nullptr;
    // What the counting plans will read must be registered NOW, before tables are flattened: the merged bodies of the counted
    // branches fold their leaf-local parts into dictionary expressions of their own (the violation formula folds the union of
    // all alternatives).  One trial lowering of every branch's plain row and of the flag, against the live registry; the
    // threshold rows repeat those bodies.  A form that does not lower: no counting for this constraint (round 3's answer serves).
    // What the counting plans will read must be registered NOW, before tables are flattened: the merged bodies of the counted
    // branches fold their leaf-local parts into dictionary expressions of their own (the violation formula folds the union of all
    // alternatives).  The forms are prepared (simplified, folded) and their dictionary atoms interned in the registry's COUNTING
    // space -- no lowering: that happens once, at the first gk_table_totals, against the then frozen registry.
    {
      PrepMemoScope memo;
      std::vector<FP> probe;
      for (uint32_t i : cf->firsts) probe.push_back(cf->rows[i]);
      probe.push_back(cf->flag);
      auto pattern_of = [](const SPath& p) { Pattern pat; for (const Step& st : p) { PatStep ps; if (st.iter) ps.any = true; else ps.key = st.key; pat.push_back(ps); } return pat; };
      std::function<void(const FP&)> walk = [&](const FP& f) {
        if (f->kind == FNode::ATOM) {
          if (f->atom.kind == Atom::DICT) {
            // (the review facts live in the main space, whoever asks: lower.cpp REVIEW FACTS)
            const bool facts = review_fact_leaf(f->atom.path);
            if (!f->atom.alt) { if (facts) e->dict_reg.intern(pattern_of(f->atom.path), f->atom.dx, true, nullptr, false); else e->dict_reg.counting().intern(pattern_of(f->atom.path), f->atom.dx, true); return; }
            // (a promoted group of row predicates: when the counting dictionary cannot take it the totals plan reads the rows)
            try { if (facts) e->dict_reg.intern(pattern_of(f->atom.path), f->atom.dx, true, nullptr, true); else e->dict_reg.counting().intern(pattern_of(f->atom.path), f->atom.dx, true); } catch (const std::runtime_error&) {}
            walk(f->atom.alt);
            return;
          }
          // (every other atom reads rows of its path: a pruned table must hold them -- publish_read_set)
          if (reads && !f->atom.path.empty()) reads->push_back(pattern_of(f->atom.path));
          if (reads && !f->atom.path2.empty()) reads->push_back(pattern_of(f->atom.path2));
          return;
        }
        if (reads && f->kind == FNode::EXISTS) {   // (the element marker rows of a counted array -- and the container's own row: the plan-local guard of a counting loop looks at its type)
          SPath el = f->base; Step st; st.iter = true; st.q = f->q; el.push_back(st); reads->push_back(pattern_of(el));
          if (!f->base.empty()) reads->push_back(pattern_of(f->base));
        }
        for (auto& k : f->kids) walk(k);
      };
      for (auto& f : probe) walk(prepare_constraint(f, mf)->viol);
    }
    for (const SPath& key : cf->keys) {
      Pattern pat;
      for (const Step& st : key) { PatStep ps; if (st.iter) { ps.any = true; ps.elems_only = true; } else ps.key = st.key; pat.push_back(ps); }
      e->dict_reg.add_key(pat);
    }
    return cf;
  } catch (const std::exception& ex) {
    if (getenv("GK_DEBUG_MULTI")) fprintf(stderr, "[gkgpu totals] no counting forms: %s\n", ex.what());
    return nullptr;
  }
}

// the counting forms prepared and trial-lowered against the FROZEN registry (as prepare_multi): all or nothing
void prepare_counts(gk_engine* e, ConstraintRec& c) {
  c.count_rows.clear(); c.count_flag = nullptr; c.count_ready = true;
  if (!c.cforms || !c.cforms->ok) return;
  try {
    PrepMemoScope memo;   // (the rows and the flag share their bodies, node for node)
    std::vector<std::shared_ptr<const PreparedConstraint>> rows;
    for (const FP& r : c.cforms->rows) rows.push_back(prepare_constraint(r, c.mf));
    auto flag = prepare_constraint(c.cforms->flag, c.mf);
    std::vector<std::shared_ptr<const PreparedConstraint>> all = rows;
    all.push_back(flag);
    for (size_t i = 0; i < all.size(); i += 24) {   // (trial builds in batches that fit a plan's result slots)
      PlanBuilder pb(&e->dict, &e->dict_reg, true);
      pb.use_counting_space();
      for (size_t j = i; j < std::min(all.size(), i + 24); j++) pb.add_constraint(all[j]);
      PlanCaps caps;
      pb.build(caps);
    }
    c.count_rows = std::move(rows); c.count_flag = std::move(flag);
  } catch (const std::exception& ex) {
    if (getenv("GK_DEBUG_MULTI")) fprintf(stderr, "[gkgpu totals] %s/%s: counting forms do not lower (%s): the multi formula serves\n", c.kind.c_str(), c.name.c_str(), ex.what());
  }
}

// "may yield more than one result" formula of a constraint (Template::compile_multi), prepared and checked to lower like the
// violation formula is -- at AddConstraint time, so that the dictionary predicates / value-id paths it needs are registered
// before tables are flattened.  Null when it does not lower: gk_table_totals then renders every violating pair of it.
std::shared_ptr<const PreparedConstraint> prepare_multi(gk_engine* e, const Template& t, const Value& params, const MatchFormulas& mf, const Value& inventory = Value()) {
  try {
    FP multi = t.compile_multi(params, &e->next_quant, inventory);
    auto prep = prepare_constraint(multi, mf);
    // (frozen: the formula must be answerable from the rows, dictionary bits and value ids the violation formulas asked the
    //  flattener for -- a guard of its own, say, would refuse reviews the violation formulas can evaluate)
    PlanBuilder pb(&e->dict, &e->dict_reg, true);
    pb.add_constraint(prep);
    PlanCaps caps;
    pb.build(caps);
    return prep;
  } catch (const std::exception& ex) {
    if (getenv("GK_DEBUG_MULTI")) fprintf(stderr, "[gkgpu totals] no multi formula: %s\n", ex.what());
    return nullptr;
  }
}

// A constraint left while value expressions are registered (flatten.hpp DictRegistry::add_vexpr): the registry is emptied and the
// constraints that stay register what they need again, by the steps that registered it when they were added and in that order -- the
// counting forms' keys and dictionary expressions, then the trial lowering of the violation formula.  What only the constraint that
// left had asked for is gone: no value rows, no dictionary bits, no carrier rows, no ranks on its account -- tables and plans are what
// they were before it came.  (Without value expressions the registry stays append-only, as it always was.)  Caller holds mu exclusively.
void reregister_values(gk_engine* e) {
  if (!e->dict_reg.has_vexprs()) return;
  e->dict_reg.reset_all();
  for (auto& c : e->constraints) {
    if (!c.alive) continue;
    try {
      auto it = e->templates.find(lower_str(c.kind));
      c.count_ready = false; c.count_rows.clear(); c.count_flag = nullptr;
      if (it != e->templates.end() && !c.referential) {
        PrepMemoScope memo;
        const Template::CountInfo ci = it->second->compile_all(c.params, &e->next_quant);
        c.cforms = derive_count_forms(e, ci, c.mf, nullptr, &c.count_reads);
      } else {
        c.cforms = nullptr;   // (a referential constraint: its results are counted by rendering until the inventory compiles it again)
        c.count_reads.clear();
      }
      if (c.prep) {
        PlanBuilder pb(&e->dict, &e->dict_reg);
        pb.add_constraint(c.prep);
        PlanCaps caps;
        pb.build(caps);
      }
    } catch (const std::exception&) {}   // (it compiled and lowered when it was added; ensure_plan words whatever is wrong with it now)
  }
}

// ---- referential templates (data.inventory) ----------------------------------------------------------------------------------
// data.inventory as one document, from the mirror of the synced objects (caller holds mu exclusively)
const Value& current_inventory(gk_engine* e) {
  if (e->inv_built == e->inv_gen) return e->inventory;
  struct Node { std::map<std::string, Node> kids; const std::string* json = nullptr; };
  Node root;
  for (auto& kv : e->inv_store) {
    Node* n = &root;
    for (auto& seg : kv.second.first) n = &n->kids[seg];
    n->json = &kv.second.second;
  }
  std::function<Value(const Node&)> build = [&](const Node& n) -> Value {
    if (n.json) return parse_json(n.json->data(), n.json->size());
    ValuePairs ps;
    for (auto& k : n.kids) ps.emplace_back(Value::string(k.first), build(k.second));
    return Value::object(ps);
  };
  e->inventory = build(root);
  e->inv_built = e->inv_gen;
  return e->inventory;
}

// start mirroring the synced objects: everything gk_data_put holds so far (caller holds resident.mu AND mu exclusively, in that order)
void start_inventory_tracking(gk_engine* e) {
  if (e->inv_tracking) return;
  for (auto& o : e->resident.objs) if (o.alive) e->inv_store[o.key] = {o.path, o.json};
  e->inv_tracking = true;
  e->inv_gen++;
}

// violation formula, prepared form and multi formula of a constraint against the current inventory (caller holds mu exclusively);
// throws what compile / the lowering throw
void compile_referential(gk_engine* e, const Template& t, ConstraintRec& c) {
  const Value& inv = current_inventory(e);
  const Template::CountInfo ci = t.compile_all(c.params, &e->next_quant, inv);
  FP viol = ci.viol;
  auto prep = prepare_constraint(viol, c.mf);
  {
    PlanBuilder pb(&e->dict, &e->dict_reg);
    pb.add_constraint(prep);
    PlanCaps caps;
    pb.build(caps);
  }
  c.viol = viol; c.prep = prep;
  c.multi_prep = prepare_multi(e, t, c.params, c.mf, inv);
  c.multi_ready = true;
  c.cforms = derive_count_forms(e, ci, c.mf, nullptr, &c.count_reads);
  c.count_ready = false;
}

// The synced objects changed: the constraints of referential templates are compiled against the new inventory.  One that no
// longer compiles (an inventory too large to unroll, say) is marked broken: evaluations fail with GK_ERR_UNSUPPORTED -- closed --
// until the inventory or the constraint changes.
void refresh_referential(gk_engine* e) {
  {
    std::shared_lock<std::shared_mutex> rl(e->mu);
    if (!e->inv_tracking || e->inv_compiled == e->inv_gen) return;
  }
  std::lock_guard<std::mutex> gate(e->plan_gate);
  std::unique_lock<std::shared_mutex> pl(e->plan_rw);
  std::unique_lock<std::shared_mutex> l(e->mu);
  if (!e->inv_tracking || e->inv_compiled == e->inv_gen) return;
  for (auto& c : e->constraints) {
    if (!c.alive || !c.referential) continue;
    auto it = e->templates.find(lower_str(c.kind));
    if (it == e->templates.end()) continue;
    try { compile_referential(e, *it->second, c); c.broken.clear(); }
    catch (const std::exception& ex) { c.broken = std::string("referential constraint ") + c.kind + "/" + c.name + " does not compile against the synced inventory: " + ex.what(); }
  }
  e->inv_compiled = e->inv_gen;
  e->plan_dirty = true;
}

// The totals plans: the alive constraints' multi formulas in groups that fit one plan each (as ensure_plan groups the violation
// formulas).  Caller holds plan_rw shared + mu shared + totals_mu; ensure_plan ran.
void ensure_totals_plans(gk_engine* e) {
  if (e->totals_gen == e->plan_gen) return;
  for (auto& g : e->totals_groups) dev_plan_free(g->dev);
  e->totals_groups.clear();
  PlanCaps bigcaps;
  bigcaps.level_cap[0] = bigcaps.level_cap[1] = bigcaps.level_cap[2] = 256;
  // the "more than one result" formulas still owed (AddConstraint leaves them to the first totals that need them; only this
  // function -- under totals_mu -- and the exclusive holders of mu touch multi_prep / multi_ready)
  for (auto& c : e->constraints) {
    if (!c.alive || c.multi_ready) continue;
    auto it = e->templates.find(lower_str(c.kind));
    c.multi_prep = it == e->templates.end() ? nullptr : prepare_multi(e, *it->second, c.params, c.mf);
    c.multi_ready = true;
  }
  // ... and the counting forms (round 4): a constraint whose forms lower is served by its count rows + flag row, any other by
  // its multi formula (round 3), one without either has every violating pair rendered
  const auto tc0 = std::chrono::steady_clock::now();
  for (auto& c : e->constraints) if (c.alive && !c.count_ready) prepare_counts(e, c);
  const auto tc1 = std::chrono::steady_clock::now();
  struct Item { std::shared_ptr<const PreparedConstraint> prep; uint32_t cid; uint8_t role; };
  std::vector<Item> have;
  for (auto& c : e->constraints) {
    if (!c.alive) continue;
    if (c.count_flag) {
      have.push_back({c.count_flag, c.id, TR_FLAG});
      for (auto& r : c.count_rows) have.push_back({r, c.id, TR_COUNT});
    } else if (c.multi_prep) have.push_back({c.multi_prep, c.id, TR_MULTI});
  }
  std::function<void(const std::vector<Item>&)> place = [&](const std::vector<Item>& g) {
    if (g.empty()) return;
    std::unique_ptr<gk_engine::Group> grp(new gk_engine::Group());
    try {
      PlanBuilder pb(&e->dict, &e->dict_reg, true);
      pb.use_counting_space(g[0].role != TR_MULTI);   // (a group holds rows of one kind: place() is called per kind)
      for (auto& it : g) pb.add_constraint(it.prep);
      grp->fast = pb.build(default_caps(e));
      grp->big = pb.build(bigcaps);
    } catch (const Unsupported&) {
      if (g.size() <= 1) {   // (checked at preparation; should it fail now: a flag / multi row that is missing means "render", a
        if (!g.empty() && g[0].role == TR_COUNT) throw;   //  missing count row would be an undercount -- never silently)
        return;
      }
      const size_t half = g.size() > 48 ? 48 : g.size() / 2;
      for (size_t i = 0; i < g.size(); i += half) place(std::vector<Item>(g.begin() + i, g.begin() + std::min(g.size(), i + half)));
      return;
    }
    for (auto& it : g) { grp->ids.push_back(it.cid); grp->roles.push_back(it.role); }
    grp->dev = dev_plan_upload(e->opts.device, grp->fast, grp->big);
    dev_plan_no_jit(grp->dev);   // (dozens of small plans, one sweep per audit each: the bytecode kernel serves them)
    e->totals_groups.push_back(std::move(grp));
  };
  {
    std::vector<Item> multis, counts;
    for (auto& it : have) (it.role == TR_MULTI ? multis : counts).push_back(it);
    place(multis);
    place(counts);
    if (getenv("GK_DEBUG_MULTI")) fprintf(stderr, "[gkgpu totals] %zu multi rows, %zu count / flag rows -> %zu plans; counting forms prepared in %.2f s, plans built in %.2f s\n", multis.size(), counts.size(),
                                          e->totals_groups.size(), std::chrono::duration<double>(tc1 - tc0).count(), std::chrono::duration<double>(std::chrono::steady_clock::now() - tc1).count());
  }
  e->totals_gen = e->plan_gen;
}

}  // namespace

extern "C" {

const char* gk_last_error(void) { return g_err.c_str(); }
const char* gk_version(void) { return "gkgpu 0.1 (gfx950)"; }

int gk_engine_create(const gk_opts* opts, gk_engine** out) {
  if (!out) return fail(GK_ERR_INVALID, "out is NULL");
  int dev = opts ? opts->device : 0;
  std::string err = dev_init(dev);
  if (!err.empty()) return fail(GK_ERR_DEVICE, err);
  gk_engine* e = new gk_engine();
  if (opts) {
    e->opts = *opts;
    if (opts->disabled_builtins) { e->disabled_builtins.clear(); for (size_t i = 0; i < opts->n_disabled_builtins; i++) if (opts->disabled_builtins[i]) e->disabled_builtins.insert(opts->disabled_builtins[i]); }
    e->opts.disabled_builtins = nullptr; e->opts.n_disabled_builtins = 0;   // (the caller's array is not kept)
  }
  *out = e;
  return GK_OK;
}

uint32_t gk_host_cpus(void) { return (uint32_t)host_cpus(); }

void gk_engine_destroy(gk_engine* e) {
  if (!e) return;
  gk_batcher_stop(e);
  dev_jit_quiesce();   // background builds of this engine's plans (a host that destroys its engines before exit() never exits under a running compile)
  if (e->comm) dev_comm_free(e->comm);
  for (auto& c : e->resident.chunks) { if (c.ev) gk_eval_free(c.ev); if (c.table) gk_table_free(c.table); }
  for (auto& v : e->variants) dev_plan_free(v.second->dev);
  for (auto& g : e->groups) dev_plan_free(g->dev);
  for (auto& g : e->totals_groups) dev_plan_free(g->dev);
  delete e;
}

int gk_template_add(gk_engine* e, const char* kind, const char* rego, const char* const* libs, size_t nlibs) {
  if (!e || !kind || !rego) return fail(GK_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> policy_turn(e->policy_gate);
  std::unique_lock<std::shared_mutex> policy_change(e->policy_rw);   // (no admission batch is between its flatten and its launch)
  try {
    std::vector<std::string> ls;
    for (size_t i = 0; i < nlibs; i++) ls.emplace_back(libs[i]);
    auto t = std::make_shared<Template>(rego, ls, &e->disabled_builtins);
    // rego.Externs() without "inventory" (GK_OPT_NO_REFERENTIAL, --enable-referential-rules=false): the frameworks' reference check
    // refuses a template that reads data.inventory when it is added (the wording of its error is the third-party driver's: unpinned)
    if ((e->opts.flags & GK_OPT_NO_REFERENTIAL) && t->references_inventory())
      return fail(GK_ERR_REGO, std::string("check refs failed on module {templates[\"admission.k8s.gatekeeper.sh\"][\"") + kind + "\"]}: disallowed ref data.inventory (referential rules are disabled)");
    std::unique_lock<std::mutex> res_lock(e->resident.mu, std::defer_lock);
    if (t->references_inventory()) res_lock.lock();   // (before mu: the order gk_resident_sweep uses)
    std::unique_lock<std::shared_mutex> l(e->mu);
    // Constraints of this kind are recompiled against the new template -- violation formula AND the prepared form every
    // plan is built from -- and put through the checks gk_constraint_add runs (referential template, lowering).  All or
    // nothing: when one of them does not compile the old template and its constraints stay as they are and the caller
    // gets the error (the reference reports it on the ConstraintTemplate's status and keeps serving the old one).
    const std::string k = lower_str(kind);
    struct Redo { ConstraintRec* c; FP viol; std::shared_ptr<const PreparedConstraint> prep, multi; bool referential; std::shared_ptr<const Template::CountForms> cforms; std::vector<Pattern> reads; Template::CountInfo ci; };
    std::vector<Redo> redo;
    for (auto& c : e->constraints) {
      if (!c.alive || lower_str(c.kind) != k) continue;
      const bool ref = t->references_inventory();
      if (ref) start_inventory_tracking(e);
      const Value inv = ref ? current_inventory(e) : Value();
      const Template::CountInfo ci = t->compile_all(c.params, &e->next_quant, inv);
      Redo r{&c, ci.viol, nullptr, nullptr, ref, nullptr};
      r.prep = prepare_constraint(r.viol, c.mf);
      PlanBuilder pb(&e->dict, &e->dict_reg);
      pb.add_constraint(r.prep);
      PlanCaps caps;
      pb.build(caps);
      r.multi = prepare_multi(e, *t, c.params, c.mf, inv);
      r.ci = ci;
      redo.push_back(std::move(r));
    }
    e->templates[k] = t;
    // the counting forms register message keys and dictionary atoms with the flattener (every table becomes stale): only now that
    // every constraint of the kind compiled -- a replacement that is refused leaves the registry as it was (round-4 advisor finding)
    for (auto& r : redo) r.cforms = derive_count_forms(e, r.ci, r.c->mf, nullptr, &r.reads);
    for (auto& r : redo) { r.c->viol = std::move(r.viol); r.c->prep = std::move(r.prep); r.c->multi_prep = std::move(r.multi); r.c->multi_ready = true; r.c->referential = r.referential; r.c->broken.clear(); r.c->cforms = std::move(r.cforms); r.c->count_reads = std::move(r.reads); r.c->count_ready = false; r.c->count_rows.clear(); r.c->count_flag = nullptr; }
    // (inv_compiled stays as it is: referential constraints of OTHER kinds may still hold an older inventory -- refresh_referential
    // recompiles every one of them at the next evaluation; marking the inventory compiled here left them stale, i.e. missed violations)
    e->plan_dirty = true;
    return GK_OK;
  } catch (const RegoError& ex) { return fail(GK_ERR_REGO, ex.what());
  } catch (const Unsupported& ex) { return fail(GK_ERR_UNSUPPORTED, ex.what());
  } catch (const RegexUnsupported& ex) { return fail(GK_ERR_UNSUPPORTED, std::string("unsupported on the device plan: ") + ex.what());
  } catch (const std::exception& ex) { return fail(GK_ERR_INTERNAL, ex.what()); }
}

int gk_template_remove(gk_engine* e, const char* kind) {
  if (!e || !kind) return fail(GK_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> policy_turn(e->policy_gate);
  std::unique_lock<std::shared_mutex> policy_change(e->policy_rw);   // (no admission batch is between its flatten and its launch)
  std::unique_lock<std::shared_mutex> l(e->mu);
  std::string k = lower_str(kind);
  if (!e->templates.erase(k)) return fail(GK_ERR_NOT_FOUND, "unknown template " + k);
  for (auto& c : e->constraints) if (lower_str(c.kind) == k) c.alive = false;
  reregister_values(e);
  e->plan_dirty = true;
  return GK_OK;
}

int gk_constraint_add(gk_engine* e, const char* json, size_t len, uint32_t* id_out) {
  if (!e || !json) return fail(GK_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> policy_turn(e->policy_gate);
  std::unique_lock<std::shared_mutex> policy_change(e->policy_rw);   // (no admission batch is between its flatten and its launch)
  try {
    Value c = parse_json(json, len);
    if (!c.is_object()) return fail(GK_ERR_INVALID, "constraint must be a JSON object");
    ConstraintRec rec;
    rec.kind = obj_string(c, "kind");
    rec.name = obj_string(c, "metadata", "name");
    rec.object = c;
    const Value* spec = c.get("spec");
    const Value* params = spec ? spec->get("parameters") : nullptr;
    rec.params = (params && !params->is_null()) ? *params : Value::object({});
    const Value* match = spec ? spec->get("match") : nullptr;
    rec.match = (match && match->is_object()) ? *match : Value();
    // (a referential template needs the synced objects: resident.mu is taken BEFORE mu, the order gk_resident_sweep uses)
    bool referential = false;
    {
      std::shared_lock<std::shared_mutex> rl(e->mu);
      auto it0 = e->templates.find(lower_str(rec.kind));
      referential = it0 != e->templates.end() && it0->second->references_inventory();
    }
    std::unique_lock<std::mutex> res_lock(e->resident.mu, std::defer_lock);
    if (referential) res_lock.lock();
    std::unique_lock<std::shared_mutex> l(e->mu);
    auto it = e->templates.find(lower_str(rec.kind));
    if (it == e->templates.end()) return fail(GK_ERR_NOT_FOUND, "unknown constraint template validator: " + rec.kind);
    rec.mf = compile_match(rec.match);
    if (it->second->references_inventory()) {
      // Referential (data.inventory): the synced objects are a CONSTANT of the compiled formula -- iterating them unrolls into
      // one alternative per object, so this serves inventories of the size the reference's fixtures have (an inventory that does
      // not fit a plan is refused: GK_ERR_UNSUPPORTED, the stock driver keeps the template); recompiled whenever they change
      if (!res_lock.owns_lock()) return fail(GK_ERR_INTERNAL, "the template of " + rec.kind + " changed while the constraint was added: try again");
      start_inventory_tracking(e);
      rec.referential = true;
      compile_referential(e, *it->second, rec);
    } else {
      const auto ta0 = std::chrono::steady_clock::now();
      PrepMemoScope memo;   // (the violation formula and the counting forms share their bodies node for node: simplified and folded once)
      const Template::CountInfo ci = it->second->compile_all(rec.params, &e->next_quant);
      rec.viol = ci.viol;
      const auto ta1 = std::chrono::steady_clock::now();
      rec.cforms = derive_count_forms(e, ci, rec.mf, &rec.viol, &rec.count_reads);
      const auto ta2 = std::chrono::steady_clock::now();
      if (getenv("GK_DEBUG_COUNTS")) {
        fprintf(stderr, "[gkgpu counts] %s/%s: %zu branches, forms %s\n", rec.kind.c_str(), rec.name.c_str(), ci.br.size(), rec.cforms ? "ok" : "none");
        for (auto& b : ci.br) fprintf(stderr, "   nq=%d keyed=%d const=%d head=%d pre=[%s] sep=[%s] tail=%d key=%s sig0=%s\n", b.nq, (int)b.keyed, (int)b.is_const, (int)b.head, b.pre.c_str(), b.sep.c_str(), (int)b.sep_tail,
                                    spath_to_string(b.key).c_str(), b.sig.empty() ? "" : b.sig[0].c_str());
        if (rec.cforms) fprintf(stderr, "   flag: %s\n", f_to_string(rec.cforms->flag).substr(0, 600).c_str());
      }
      // validate that it lowers (element scopes, register pressure) before accepting it
      {
        PlanBuilder pb(&e->dict, &e->dict_reg);
        rec.prep = prepare_constraint(rec.viol, rec.mf);
        pb.add_constraint(rec.prep);
        PlanCaps caps;
        pb.build(caps);
      }
      rec.multi_ready = false;   // (prepare_multi: on demand, ensure_totals_plans)
      if (getenv("GK_DEBUG_LOAD")) fprintf(stderr, "[gkgpu load] %s/%s: evaluate %.3f s, counting forms %.3f s, prepare + trial plan %.3f s\n", rec.kind.c_str(), rec.name.c_str(),
                                           std::chrono::duration<double>(ta1 - ta0).count(), std::chrono::duration<double>(ta2 - ta1).count(),
                                           std::chrono::duration<double>(std::chrono::steady_clock::now() - ta2).count());
    }
    for (auto& o : e->constraints) if (o.alive && o.kind == rec.kind && o.name == rec.name) o.alive = false;   // replace
    rec.id = (uint32_t)e->constraints.size();
    e->constraints.push_back(rec);
    e->plan_dirty = true;
    if (id_out) *id_out = rec.id;
    return GK_OK;
  } catch (const JsonError& ex) { return fail(GK_ERR_INVALID, ex.what());
  } catch (const RegoError& ex) { return fail(GK_ERR_REGO, ex.what());
  } catch (const Unsupported& ex) { return fail(GK_ERR_UNSUPPORTED, ex.what());
  } catch (const RegexUnsupported& ex) { return fail(GK_ERR_UNSUPPORTED, std::string("unsupported on the device plan: ") + ex.what());
  } catch (const std::exception& ex) { return fail(GK_ERR_INTERNAL, ex.what()); }
}

int gk_constraint_remove(gk_engine* e, const char* kind, const char* name) {
  if (!e || !kind || !name) return fail(GK_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> policy_turn(e->policy_gate);
  std::unique_lock<std::shared_mutex> policy_change(e->policy_rw);   // (no admission batch is between its flatten and its launch)
  std::unique_lock<std::shared_mutex> l(e->mu);
  bool found = false;
  for (auto& c : e->constraints) if (c.alive && c.kind == kind && c.name == name) { c.alive = false; found = true; }
  if (!found) return fail(GK_ERR_NOT_FOUND, std::string("unknown constraint ") + kind + "/" + name);
  reregister_values(e);
  e->plan_dirty = true;
  return GK_OK;
}

namespace {

uint64_t text_hash(const char* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) { h ^= (uint8_t)p[i]; h *= 1099511628211ull; }
  return h ^ (h >> 29);
}

// an object leaves its slot (replaced, removed, or its Namespace changed): the slot is masked out of every answer
void resident_tombstone(gk_engine::Resident& R, gk_engine::ResObj& o) {
  if (o.chunk == UINT32_MAX) return;
  gk_engine::ResChunk& c = R.chunks[o.chunk];
  const uint64_t bit = 1ull << (o.slot % 64);
  if (c.live[o.slot / 64] & bit) { c.live[o.slot / 64] &= ~bit; c.n_live--; R.n_dead_slots++; }
  o.chunk = UINT32_MAX;
}

void resident_requeue(gk_engine::Resident& R, uint32_t id) {
  gk_engine::ResObj& o = R.objs[id];
  if (!o.alive) return;
  const bool queued = o.chunk == UINT32_MAX && std::find(R.pending.begin(), R.pending.end(), id) != R.pending.end();
  resident_tombstone(R, o);
  if (!queued) R.pending.push_back(id);
}

}  // namespace

int gk_data_put(gk_engine* e, const char* const* path, size_t npath, const char* json, size_t len) {
  if (!e || !path || !npath || !json) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    Value v = parse_json(json, len);
    std::vector<std::string> p;
    for (size_t i = 0; i < npath; i++) p.emplace_back(path[i]);
    const bool is_ns = v.is_object() && obj_is_namespace(v) && p.size() == 4 && p[0] == "cluster";
    {
      std::unique_lock<std::shared_mutex> l(e->mu);
      // nsCache.Add: cluster-scoped core/v1 Namespace objects (ns_cache.go:22-43)
      if (is_ns) e->ns_cache.put(p[3], v);
      if (e->inv_tracking) {   // data.inventory of the referential constraints
        std::string k;
        for (auto& x : p) { k += x; k.push_back('/'); }
        auto& slot = e->inv_store[k];
        if (slot.second.size() != len || memcmp(slot.second.data(), json, len) != 0) { slot = {p, std::string(json, len)}; e->inv_gen++; }
      }
    }
    // the resident set: this version of the object is flattened by the next gk_resident_sweep
    gk_engine::Resident& R = e->resident;
    std::lock_guard<std::mutex> rl(R.mu);
    std::string key;
    for (auto& x : p) { key += x; key.push_back('/'); }
    auto it = R.by_key.find(key);
    uint32_t id;
    if (it == R.by_key.end()) {
      id = (uint32_t)R.objs.size();
      R.objs.emplace_back();
      gk_engine::ResObj& o = R.objs.back();
      o.path = p; o.key = key;
      o.ns = (p.size() == 5 && p[0] == "namespace") ? p[1] : std::string();
      o.is_namespace = is_ns;
      R.by_key.emplace(key, id);
      if (!o.ns.empty()) R.by_ns[o.ns].push_back(id);
      R.n_live++;
    } else {
      id = it->second;
      gk_engine::ResObj& o = R.objs[id];
      if (o.alive && o.json.size() == len && memcmp(o.json.data(), json, len) == 0) return GK_OK;   // unchanged
      if (!o.alive) { o.alive = true; R.n_live++; }
      R.by_text.erase(text_hash(o.json.data(), o.json.size()));
    }
    gk_engine::ResObj& o = R.objs[id];
    o.json.assign(json, len);
    R.by_text[text_hash(json, len)] = id;
    resident_requeue(R, id);
    // a Namespace object is part of the review of every object living in it (Matchable.Namespace, namespaceObject)
    if (is_ns) { auto bn = R.by_ns.find(p[3]); if (bn != R.by_ns.end()) for (uint32_t d : bn->second) resident_requeue(R, d); }
    R.swept = false;
    R.set_gen++;
    return GK_OK;
  } catch (const JsonError& ex) { return fail(GK_ERR_INVALID, ex.what()); }
}

int gk_data_remove(gk_engine* e, const char* const* path, size_t npath) {
  if (!e || !path || !npath) return fail(GK_ERR_INVALID, "NULL argument");
  std::vector<std::string> p;
  for (size_t i = 0; i < npath; i++) p.emplace_back(path[i]);
  const bool is_ns = p.size() == 4 && p[0] == "cluster" && p[1] == "v1" && p[2] == "Namespace";
  {
    std::unique_lock<std::shared_mutex> l(e->mu);
    if (is_ns) e->ns_cache.remove(p[3]);
    if (e->inv_tracking) {
      std::string k;
      for (auto& x : p) { k += x; k.push_back('/'); }
      if (e->inv_store.erase(k)) e->inv_gen++;
    }
  }
  gk_engine::Resident& R = e->resident;
  std::lock_guard<std::mutex> rl(R.mu);
  std::string key;
  for (auto& x : p) { key += x; key.push_back('/'); }
  auto it = R.by_key.find(key);
  if (it != R.by_key.end() && R.objs[it->second].alive) {
    gk_engine::ResObj& o = R.objs[it->second];
    resident_tombstone(R, o);
    R.pending.erase(std::remove(R.pending.begin(), R.pending.end(), it->second), R.pending.end());
    R.by_text.erase(text_hash(o.json.data(), o.json.size()));
    o.alive = false; o.json.clear();
    R.n_live--;
    if (is_ns) { auto bn = R.by_ns.find(p[3]); if (bn != R.by_ns.end()) for (uint32_t d : bn->second) resident_requeue(R, d); }
    R.swept = false;
    R.set_gen++;
  }
  return GK_OK;
}

int gk_excluder_replace(gk_engine* e, const char* match_json, size_t len) {
  if (!e) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    static const char* all[] = {"audit", "webhook", "mutation-webhook", "sync"};   // allProcesses (excluder.go:31-36)
    std::map<std::string, std::vector<std::string>> next;
    auto put = [&](const std::string& proc, const std::string& ns) {
      auto& v = next[proc];
      if (std::find(v.begin(), v.end(), ns) == v.end()) v.push_back(ns);
    };
    if (match_json && len) {
      Value m = parse_json(match_json, len);
      if (!m.is_null() && !m.is_array()) return fail(GK_ERR_INVALID, "spec.match must be an array of {excludedNamespaces, processes}");
      if (m.is_array()) for (const Value& ent : m.items()) {   // Excluder.Add (excluder.go:52-76)
        if (!ent.is_object()) continue;
        const Value* nss = ent.get("excludedNamespaces");
        const Value* procs = ent.get("processes");
        if (!nss || !nss->is_array() || !procs || !procs->is_array()) continue;
        for (const Value& ns : nss->items()) {
          if (!ns.is_string()) continue;
          for (const Value& op : procs->items()) {
            if (!op.is_string()) continue;
            if (op.str() == "*") { for (const char* a : all) put(a, ns.str()); } else put(op.str(), ns.str());
          }
        }
      }
    }
    std::unique_lock<std::shared_mutex> l(e->mu);
    if (next != e->excluder) { e->excluder.swap(next); e->excluder_gen++; }   // Excluder.Replace
    return GK_OK;
  } catch (const JsonError& ex) { return fail(GK_ERR_INVALID, ex.what());
  } catch (const std::exception& ex) { return fail(GK_ERR_INTERNAL, ex.what()); }
}

int gk_excluder_excluded(gk_engine* e, const char* process, const gk_review_in* review, int32_t* excluded) {
  if (!e || !process || !review || !excluded) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    *excluded = 0;
    std::vector<std::string> pats;
    {
      std::shared_lock<std::shared_mutex> l(e->mu);
      auto it = e->excluder.find(process);
      if (it == e->excluder.end()) return GK_OK;
      pats = it->second;
    }
    Value body;
    try { body = parse_json(review->json, review->json_len); } catch (const std::exception&) { return GK_OK; }   // decode error: not excluded
    *excluded = review_excluded(pats, review->kind, body) ? 1 : 0;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_INTERNAL, ex.what()); }
}

// `prem` (may be NULL): per review, non-zero = the caller ran Matcher.Match itself (RF_PREMATCHED, plan.hpp); GK_TABLE_PRE_MATCHED = all of them
static int table_create_impl(gk_engine* e, const gk_review_in* reviews, size_t n, uint32_t flags, int32_t* statuses, const uint8_t* prem, gk_table** out);
int gk_table_create(gk_engine* e, const gk_review_in* reviews, size_t n, uint32_t flags, int32_t* statuses, gk_table** out) {
  return table_create_impl(e, reviews, n, flags, statuses, nullptr, out);
}
static int table_create_impl(gk_engine* e, const gk_review_in* reviews, size_t n, uint32_t flags, int32_t* statuses, const uint8_t* prem, gk_table** out) {
  if (!e || !out || (n && !reviews)) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    // referential constraints follow the synced inventory: compiled again -- and their dictionary expressions registered -- BEFORE
    // the rows are made, or the table would lack the <leaf>.$d rows the new plan reads (a plan that does not build is the
    // evaluation's error to report, not this call's)
    try { ensure_plan(e); } catch (const std::exception&) {}
    std::unique_ptr<gk_table> t(new gk_table());
    t->eng = e;
    bool keep = flags & GK_TABLE_KEEP_DOCS;
    t->review_errors.resize(n);
    t->key_span.assign(n, {0u, 0u});
    if (keep) t->docs.resize(n);
    if ((flags & GK_TABLE_KEEP_TEXT) && !keep) t->texts.assign(reviews, reviews + n);
    const auto t_begin = std::chrono::steady_clock::now();
    // Reviews are flattened by host threads, each on a contiguous range of whole tiles (the path dictionary is shared and
    // thread-safe).  Fast path: JSON text -> rows in one pass (Flattener::add_json); reviews it declines -- and every
    // review when the parsed documents must be kept for rendering -- go through parse_json + HandleReview normalisation +
    // Flattener::add, which produces the same rows.  The parts are then copied, in parallel, into the table's arrays.
    // reviews per row group: small batches (admission) keep 64-review groups; resident sets get large groups, whose
    // segments fill the lanes of the waves that stream them (plan.hpp / kernel_body.inc).  GK_RPT overrides (64|128|256|512).
    uint32_t rpt = n >= 8192 ? 256 : GK_RPT_MIN;
    if (rpt == 256) {
      // a large policy set (several plan groups, or accumulators too wide for three 256-review groups per CU) runs better on
      // 128-review groups: 4-wave workgroups of half the LDS footprint keep more waves resident and let the plan groups'
      // kernels share the CUs (configs[4]'s 200 templates: 0.81 against 1.11 ms per sweep, profiles/r03_variants_f_*.log)
      try {
        ensure_plan(e);
        std::shared_lock<std::shared_mutex> pl(e->plan_rw);
        if (e->groups.size() > 1 || (size_t)e->groups[0]->fast.dims.acc_words * 256 * 4 > 72 * 1024) rpt = 128;
      } catch (const std::exception&) {}
    }
    if (const char* rp = getenv("GK_RPT")) { int v = atoi(rp); if (v == 64 || v == 128 || v == 256 || v == 512) rpt = (uint32_t)v; }
    t->rpt = rpt;
    t->dict_gen = e->dict_reg.gen();
    t->pruned = ((flags & GK_TABLE_PRUNED) != 0 || getenv("GK_FORCE_PRUNE") != nullptr) && !getenv("GK_NO_PRUNE");   // (GK_FORCE_PRUNE: the test suites run every table pruned)
    t->reads_gen = e->dict_reg.reads_gen();
    const size_t n_tiles = (n + rpt - 1) / rpt;
    // host threads of a table build: at most 64 -- measured on the 256-thread GPU box (profiles/r03_phases_d_*.log): 1M objects
    // flatten in 0.45 s on 64 threads, 0.61 s on 128, 0.68 s on 256 (first-touch page faults and the shared dictionaries
    // contend; the GPU-side assembly does not care how many parts there are)
    // (ingest is a BURST: a 64 k-review batch is 20-25 ms of work on 64 threads, shorter than the 100 ms period of a cgroup CPU
    //  quota, so it may run wider than the quota -- measured on a 16-CPU-quota box: streaming 2.3-2.5 M reviews/s on 64 threads,
    //  1.8 M/s on 16; the 1 M-object build is the same either way.  Sustained host passes (gk_table_totals) size by host_cpus().)
    size_t n_threads = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(std::thread::hardware_concurrency(), 64), (n + 511) / 512));
    if (const char* ht = getenv("GK_HOST_THREADS")) n_threads = std::max(1, atoi(ht));
    n_threads = std::min(n_threads, std::max<size_t>(n_tiles, 1));
    const size_t tiles_per = (n_tiles + n_threads - 1) / std::max<size_t>(n_threads, 1);
    t->key_per_part = std::max<size_t>(1, tiles_per * rpt);
    t->key_arena.assign(std::max<size_t>(n_threads, 1), std::string());
    const bool slow_only = keep || getenv("GK_SLOW_INGEST") != nullptr;
    std::vector<HostTable> parts(n_threads);
    std::vector<std::string> part_err(n_threads);
    std::vector<uint64_t> part_fast(n_threads, 0);
    // process excluder: reviews of a table built for a process (audit sweep / validating webhook) whose namespace the
    // Config excludes for that process are skipped BEFORE evaluation -- pkg/audit/manager.go:530,599 (skipExcludedNamespace),
    // pkg/webhook/policy.go:197, pkg/webhook/common.go:149-189.  They keep their slot, hold no rows and report
    // GK_REVIEW_EXCLUDED.
    std::vector<std::string> excl;
    if (flags & (GK_TABLE_PROCESS_AUDIT | GK_TABLE_PROCESS_WEBHOOK)) {
      std::shared_lock<std::shared_mutex> l(e->mu);
      auto it = e->excluder.find((flags & GK_TABLE_PROCESS_AUDIT) ? "audit" : "webhook");
      if (it != e->excluder.end()) excl = it->second;
    }
    const Flattener::ExcludeFn excl_fn = [&](bool is_ns, const std::string& ns, const std::string& name) { return excluder_matches(excl, is_ns ? name : ns); };
    auto work = [&](size_t w) {
      try {
        // one Flattener per host thread and engine, kept across tables (Flattener::begin_table)
        thread_local std::unordered_map<uint64_t, std::unique_ptr<Flattener>> tl_flatteners;
        std::unique_ptr<Flattener>& slot = tl_flatteners[e->uid];
        if (!slot) { if (tl_flatteners.size() > 8) { tl_flatteners.clear(); } tl_flatteners[e->uid].reset(new Flattener(&e->dict, &e->dict_reg)); }
        Flattener& fl = *tl_flatteners[e->uid];
        fl.set_pruning(t->pruned);
        fl.begin_table();
        parts[w].rpt = rpt;
        const size_t lo = std::min(n, w * tiles_per * rpt), hi = std::min(n, (w + 1) * tiles_per * rpt);
        {
          // the part's arrays, sized ONCE from the JSON text it will flatten (a row per ~9 bytes of Kubernetes JSON, a
          // heap byte per ~5; a quarter on top): no growth by reallocation while 255 other threads do the same
          size_t jb = 0;
          for (size_t i = lo; i < hi; i++) jb += reviews[i].json_len + reviews[i].namespace_len / 4;
          if (jb >= (256u << 10)) {
            const size_t rows_est = jb / 7 + 4096;
            parts[w].rows.presize(rows_est);
            parts[w].shdr.presize(rows_est);
            parts[w].heap.presize(jb / 4 + 65536);
          }
        }
        std::string key_scratch;
        std::string& arena = t->key_arena[w];
        arena.reserve((hi - lo) * 40);
        auto put_key = [&](size_t i, const std::string& k) { t->key_span[i] = {(uint32_t)arena.size(), (uint32_t)k.size()}; arena += k; };
        // a review that may turn out to be beyond the device's limits keeps its text with the table (rare: a copy per such review)
        auto keep_if_big = [&](size_t i, const HostTable& part) {
          if (part.rflags.empty() || !(part.rflags.back() & (RF_TOO_BIG | RF_REFUSE | RF_HOST_CAND))) return;
          const gk_review_in& r = reviews[i];
          gk_table::OwnedReview o;
          o.kind = r.kind; o.source = r.source;
          o.json.assign(r.json ? r.json : "", r.json ? r.json_len : 0);
          if (r.namespace_json) { o.has_ns = true; o.ns.assign(r.namespace_json, r.namespace_len); }
          if (r.ns_object_json) { o.has_nsobj = true; o.nsobj.assign(r.ns_object_json, r.ns_object_len); }
          if (r.operation) { o.has_op = true; o.op = r.operation; }
          std::lock_guard<std::mutex> bl(t->big_mu);
          t->big_texts[(uint32_t)i] = std::move(o);
        };
        for (size_t i = lo; i < hi; i++) {
          const gk_review_in& r = reviews[i];
          if (i + 2 < hi && reviews[i + 2].json) {   // the text of the review after next: first touched by the scanner otherwise, a DRAM round trip per line
            const char* nj = reviews[i + 2].json;
            const size_t nl = std::min<size_t>(reviews[i + 2].json_len, 4096);
            for (size_t o = 0; o < nl; o += 64) __builtin_prefetch(nj + o, 0, 1);
          }
          if (!slow_only) {
            RawReview rr;
            rr.kind = r.kind; rr.source = r.source; rr.json = r.json; rr.json_len = r.json_len;
            rr.ns_json = r.namespace_json; rr.ns_len = r.namespace_len; rr.nsobj_json = r.ns_object_json; rr.nsobj_len = r.ns_object_len;
            rr.operation = r.operation;
            int rc = fl.add_json(rr, e->ns_cache, &parts[w], &key_scratch, excl.empty() ? nullptr : &excl_fn);
            if (rc == Flattener::ADDED) { put_key(i, key_scratch); if (statuses) statuses[i] = GK_OK; part_fast[w]++; keep_if_big(i, parts[w]); continue; }
            if (rc == Flattener::EXCLUDED) {
              if (statuses) statuses[i] = GK_REVIEW_EXCLUDED;
              fl.add_skipped(&parts[w]);
              part_fast[w]++;
              continue;
            }
          }
          ReviewDoc doc;
          int st = GK_OK;
          try {
            Value body = parse_json(r.json, r.json_len);
            Value mns = parse_opt(r.namespace_json, r.namespace_len);
            Value nso = parse_opt(r.ns_object_json, r.ns_object_len);
            if (!excl.empty() && review_excluded(excl, r.kind, body)) {
              if (statuses) statuses[i] = GK_REVIEW_EXCLUDED;
              doc.request = Value::object({});
              fl.add_skipped(&parts[w]);
              if (keep) t->docs[i] = doc;
              continue;
            }
            if (r.kind == GK_REVIEW_OBJECT) doc = normalize_object(body, mns, nso, r.source, r.operation ? r.operation : "", e->ns_cache);
            else doc = normalize_admission_request(body, mns, nso, r.source, e->ns_cache);
          } catch (const std::exception& ex) {
            st = GK_ERR_REVIEW;
            t->review_errors[i] = ex.what();
            doc = ReviewDoc();
            doc.request = Value::object({});
          }
          if (statuses) statuses[i] = st;
          {   // object identity in the order pkg/audit sorts violations by
            const Value* o = doc.request.get("object");
            if (!o || !o->is_object()) o = doc.request.get("oldObject");
            std::string g_, v_, k_, key;
            if (o && o->is_object()) {
              obj_gvk(*o, &g_, &v_, &k_);
              key = g_; key.push_back('\0'); key += v_; key.push_back('\0'); key += k_; key.push_back('\0');
              key += obj_string(*o, "metadata", "namespace"); key.push_back('\0'); key += obj_string(*o, "metadata", "name");
            }
            put_key(i, key);
          }
          if (st == GK_ERR_REVIEW) fl.add_skipped(&parts[w]);   // HandleReview's error is the caller's answer: nothing is evaluated
          else { fl.add(doc, &parts[w]); keep_if_big(i, parts[w]); }
          if (keep) t->docs[i] = doc;
        }
        fl.flush(&parts[w]);
      } catch (const std::exception& ex) { part_err[w] = ex.what(); }
    };
    auto run_threads = [&](const std::function<void(size_t)>& fn) {
      if (n_threads <= 1) { fn(0); return; }
      HostWorkers::get().run(n_threads, fn);
    };
    // content digest (test aid, GK_TABLE_DIGEST=1): per part while its rows are still on the host; parts are combined in
    // order, strings by value (not by heap offset), so the digest does not depend on the number of host threads
    const bool want_digest = getenv("GK_TABLE_DIGEST") != nullptr;
    std::vector<std::vector<uint64_t>> part_digest(n_threads);
    auto digest_part = [&](size_t w) {
      const HostTable& P = parts[w];
      for (size_t tl = 0; tl + 0 < P.tile_seg.size(); tl++) {
        uint64_t d = 1469598103934665603ull;
        auto mix = [&](uint64_t v) { d ^= v; d *= 1099511628211ull; d ^= d >> 31; };
        const uint32_t s0 = P.tile_seg[tl], s1 = tl + 1 < P.tile_seg.size() ? P.tile_seg[tl + 1] : (uint32_t)P.segs.size();
        for (uint32_t sg = s0; sg < s1; sg++) {
          const uint32_t a = P.segs[sg].start, b = sg + 1 < P.segs.size() ? P.segs[sg + 1].start : (uint32_t)P.rows.size();
          for (uint32_t i = a; i < b; i++) {
            const Row& r = P.rows[i];
            mix(P.segs[sg].path); mix(((uint64_t)r.rev << 32) | r.meta);
            if ((r.meta & ROW_TYPE_MASK) == T_STRING && !(r.meta & ROW_STR_INLINE)) {
              uint32_t len; memcpy(&len, &P.heap[r.lo - 4], 4);
              mix(len); mix(r.hi);
              for (uint32_t k = 0; k < len; k++) mix(P.heap[r.lo + k]);
              for (int k = 0; k < 4; k++) mix(P.shdr[i].w[k]);
            } else mix(((uint64_t)r.hi << 32) | r.lo);
          }
        }
        part_digest[w].push_back(d);
      }
    };
    std::vector<DevPart*> dev_parts(n_threads, nullptr);
    std::vector<double> part_upload_s(n_threads, 0);
    run_threads([&](size_t w) {
      work(w);
      if (!part_err[w].empty()) return;
      try {
        if (want_digest) digest_part(w);
        const auto u0 = std::chrono::steady_clock::now();
        dev_parts[w] = dev_part_upload(e->opts.device, parts[w]);   // each thread ships its part as soon as it is flattened
        part_upload_s[w] = std::chrono::duration<double>(std::chrono::steady_clock::now() - u0).count();
      } catch (const std::exception& ex) { part_err[w] = ex.what(); }
    });
    for (auto& pe_ : part_err) if (!pe_.empty()) { for (DevPart* dp : dev_parts) dev_part_free(dp); return fail(GK_ERR_INTERNAL, pe_); }
    // ---- what is global: row / heap bases by prefix sum -> segment starts, the slot index, review flags
    HostTable& H = t->host;
    H.rpt = rpt;
    {
      size_t rb = 0, hb = 0;
      for (size_t w = 0; w < n_threads; w++) {
        HostTable& P = parts[w];
        const uint32_t sb = (uint32_t)H.segs.size();
        for (const auto& sg : P.segs) H.segs.push_back({sg.path, (uint32_t)(sg.start + rb)});
        for (uint32_t ts : P.tile_seg) H.tile_seg.push_back(ts + sb);
        H.rflags.insert(H.rflags.end(), P.rflags.begin(), P.rflags.end());
        if (P.path_rows.size() > H.path_rows.size()) H.path_rows.resize(P.path_rows.size(), 0);
        for (size_t i = 0; i < P.path_rows.size(); i++) H.path_rows[i] += P.path_rows[i];
        if (P.path_max.size() > H.path_max.size()) H.path_max.resize(P.path_max.size(), 0);
        for (size_t i = 0; i < P.path_max.size(); i++) H.path_max[i] = std::max(H.path_max[i], P.path_max[i]);
        rb += P.n_rows_total; hb += P.heap_total;
        t->stats.fast_reviews += part_fast[w];
        H.n_reviews += P.n_reviews;
      }
      if (rb >= 0xFFFFFFF0ull || hb >= 0xFFFFFFF0ull) {
        for (DevPart* dp : dev_parts) dev_part_free(dp);
        return fail(GK_ERR_INVALID, "table too large for 32-bit row/heap offsets: split the batch");
      }
      t->n_rows = rb;
      t->stats.heap_bytes = hb;
      H.n_rows_total = rb;
    }
    if (prem || (flags & GK_TABLE_PRE_MATCHED))
      for (size_t i = 0; i < n && i < H.rflags.size(); i++) if ((flags & GK_TABLE_PRE_MATCHED) || prem[i]) { H.rflags[i] |= RF_PREMATCHED; t->any_prematched = true; }
    Flattener::build_index(&t->host);
    if (want_digest) {
      uint64_t d = 1469598103934665603ull;
      auto mix = [&](uint64_t v) { d ^= v; d *= 1099511628211ull; d ^= d >> 31; };
      for (auto& pd : part_digest) for (uint64_t x : pd) mix(x);
      for (uint32_t f : H.rflags) mix(f);
      for (uint32_t sp : H.slot_path) mix(sp);
      for (size_t i = 0; i < n; i++) for (unsigned char c : t->obj_key(i)) mix(c);
      t->stats.digest = d;
    }
    const auto t_indexed = std::chrono::steady_clock::now();
    t->dev = dev_table_assemble(e->opts.device, dev_parts, t->host);
    t->sides.emplace_back();
    t->sides[0].dev = t->dev;
    const auto t_up = std::chrono::steady_clock::now();
    t->n_reviews = (uint32_t)n;
    t->dir_bytes = t->host.rflags.size() * 4;
    t->slot_path = t->host.slot_path;
    t->path_rows = t->host.path_rows;
    t->path_max = t->host.path_max;
    t->resident = (flags & GK_TABLE_RESIDENT) != 0;
    t->stats.n_reviews = n; t->stats.n_rows = t->n_rows; t->stats.host_threads = (uint32_t)n_threads;
    t->stats.device_bytes = dev_table_bytes(t->dev);
    // the parts' transfers overlap the flattening of the other host threads: upload_s is what is NOT hidden (slot index,
    // review flags, placing the parts on the device), flatten_s the rest of the wall clock
    t->stats.upload_s = std::chrono::duration<double>(t_up - t_indexed).count();
    t->stats.flatten_s = std::chrono::duration<double>(t_indexed - t_begin).count();
    for (size_t i = 0; i < n; i++) t->stats.json_bytes += reviews[i].json_len;
    if (!g_debug_keep_slot_index.load()) { t->host.tile_idx.clear(); t->host.tile_idx.shrink_to_fit(); }
    *out = t.release();
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

// ------------------------------------------------------------------------------------------------ audit spool (row f4)
namespace {
struct SpoolHolder {
  gk_spool_info pub;   // first member
  std::vector<std::string> names;
  std::vector<const char*> ptrs;
  std::vector<int32_t> statuses;
};
bool read_file(const std::string& path, std::string* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char buf[65536];
  size_t n;
  out->clear();
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, n);
  const bool ok = !ferror(f);
  fclose(f);
  return ok;
}
}  // namespace

int gk_table_create_spool(gk_engine* e, const char* api_cache_dir, const char* kind, uint32_t folders, uint32_t flags,
                          gk_spool_info** info, gk_table** out) {
  if (!e || !api_cache_dir || !kind || !out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    std::unique_ptr<SpoolHolder> h(new SpoolHolder());
    memset(&h->pub, 0, sizeof h->pub);
    // 1. the files, folder by folder (reviewObjects, manager.go:676-686), numeric order within a folder
    struct Item { std::string name, text, ns_text; };
    std::vector<Item> items;
    for (uint32_t fo = 0; fo < folders; fo++) {
      const std::string sub = std::string(kind) + "_" + std::to_string(fo), dir = std::string(api_cache_dir) + "/" + sub;
      std::vector<std::string> files;
      if (DIR* d = opendir(dir.c_str())) {
        while (dirent* de = readdir(d)) { if (de->d_name[0] != '.') files.emplace_back(de->d_name); }
        closedir(d);
      } else h->pub.n_folders_missing++;   // (a folder that cannot be opened: "Unable to get files from directory", the loop goes on)
      std::sort(files.begin(), files.end(), [](const std::string& a, const std::string& b) { return a.size() != b.size() ? a.size() < b.size() : a < b; });
      for (const std::string& fn : files) {
        h->pub.n_files++;
        Item it;
        it.name = sub + "/" + fn;
        if (!read_file(dir + "/" + fn, &it.text)) { h->pub.n_unreadable++; continue; }
        h->pub.bytes += it.text.size();
        items.push_back(std::move(it));
      }
    }
    // 2. the Namespace of every object, from the driver's cache (nsCache.Get, manager.go:694-704): looked up by metadata.namespace
    std::unordered_map<std::string, std::string> ns_json;   // namespace name -> its JSON ("" = not cached)
    std::vector<Item> kept;
    for (Item& it : items) {
      std::string nsname;
      try {
        Value v = parse_json(it.text.data(), it.text.size());
        if (!v.is_object()) { h->pub.n_unreadable++; continue; }
        nsname = obj_string(v, "metadata", "namespace");
      } catch (const std::exception&) { h->pub.n_unreadable++; continue; }   // readUnstructured fails: logged, next file
      if (!nsname.empty()) {
        auto f = ns_json.find(nsname);
        if (f == ns_json.end()) {
          Value ns = e->ns_cache.get(nsname);
          f = ns_json.emplace(nsname, ns.defined() ? to_json(ns) : std::string()).first;
        }
        if (f->second.empty()) { h->pub.n_namespace_missing++; continue; }   // "Unable to look up object namespace": skipped
        it.ns_text = f->second;
      }
      kept.push_back(std::move(it));
    }
    // 3. one table of AugmentedUnstructured{Object, Namespace, Source: Original} + the namespaceObject option
    std::vector<gk_review_in> rins(kept.size());
    for (size_t i = 0; i < kept.size(); i++) {
      gk_review_in& r = rins[i];
      memset(&r, 0, sizeof r);
      r.kind = GK_REVIEW_OBJECT;
      r.source = GK_SRC_ORIGINAL;
      r.json = kept[i].text.data(); r.json_len = kept[i].text.size();
      if (!kept[i].ns_text.empty()) {
        r.namespace_json = kept[i].ns_text.data(); r.namespace_len = kept[i].ns_text.size();
        r.ns_object_json = kept[i].ns_text.data(); r.ns_object_len = kept[i].ns_text.size();
      }
      h->names.push_back(kept[i].name);
    }
    h->statuses.assign(std::max<size_t>(1, kept.size()), GK_OK);
    int rc = gk_table_create(e, rins.data(), rins.size(), flags, h->statuses.data(), out);
    if (rc != GK_OK) return rc;
    h->statuses.resize(kept.size());
    h->pub.n_reviews = kept.size();
    h->pub.statuses = h->statuses.data();
    // (HandleReview's verdict per spooled object, as gk_table_create reports it: the reference logs "Unable to review object from
    //  file" for a rejected one and goes on; GK_REVIEW_EXCLUDED = the process excluder skipped it)
    for (int32_t st : h->statuses) { if (st == GK_REVIEW_EXCLUDED) h->pub.n_excluded++; else if (st != GK_OK) h->pub.n_rejected++; }
    // GK_TABLE_KEEP_TEXT remembers WHERE the text lives: here it lives in `kept`, so the table takes it over (round-3 advisor
    // finding: gk_table_totals / gk_render read freed memory).  Moving the vector keeps every string where it is.
    if ((*out)->texts.size() == kept.size() && !kept.empty()) (*out)->owned_text = std::make_shared<std::vector<Item>>(std::move(kept));
    for (auto& nm : h->names) h->ptrs.push_back(nm.c_str());
    h->pub.names = h->ptrs.data();
    if (info) *info = &h.release()->pub;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_INTERNAL, ex.what()); }
}

void gk_spool_info_free(gk_spool_info* info) { if (info) delete reinterpret_cast<SpoolHolder*>(info); }

int gk_table_get_stats(const gk_table* t, gk_table_stats* out) {
  if (!t || !out) return fail(GK_ERR_INVALID, "NULL argument");
  *out = t->stats;
  return GK_OK;
}

void gk_table_free(gk_table* t) {
  if (!t) return;
  for (DevTable* v : t->tviews) dev_table_free(v);
  table_changes_drop(t);
  dev_keys_free(t->dkeys);
  for (size_t g = t->sides.size(); g-- > 0;) {   // (views before the table: side 0 last)
    gk_table::Side& s = t->sides[g];
    if (s.vview) { dev_verify_forget(s.vview); dev_table_free(s.vview); }
    dev_plan_free(s.vtwin);
    dev_verify_forget(s.dev);
    dev_tviol_forget(s.dev);
    dev_tchg_forget(s.dev);
    dev_delta_drop(s.dev);
    dev_table_free(s.dev);
  }
  delete t;
}

struct EvalHolder {
  gk_eval_out pub;   // first member: gk_eval_free recovers the holder from the public pointer
  uint32_t lds_bytes = 0;
  EvalOut out;
  std::vector<uint32_t> ids;
  std::vector<uint32_t> host_evaluated;   // reviews beyond the device's limits that the host evaluator answered (complete_on_host)
};
static void complete_on_host(gk_engine* e, gk_table* t, EvalHolder* h, bool want_match, bool want_list);

int gk_table_eval(gk_engine* e, gk_table* t, uint32_t flags, gk_eval_out** out) {
  if (!e || !t || !out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    ensure_plan(e);
    if (const char* why = table_stale(e, t)) return fail(GK_ERR_INVALID, why);
    std::unique_ptr<EvalHolder> h(new EvalHolder());
    EvalOptions opt;
    opt.download = !(flags & GK_EVAL_NO_DOWNLOAD);
    opt.want_match = flags & GK_EVAL_WANT_MATCH;
    opt.time_each = (flags & GK_EVAL_TIME_EACH) != 0;
    opt.kernel_only = (flags & GK_EVAL_KERNEL_ONLY) != 0 && (flags & GK_EVAL_ASYNC) != 0;
    // (timing events only where the caller can want the kernels' duration: an evaluation that launches and collects in one call, or
    //  enqueue-only launches under one of the two timing flags)
    opt.timed = !(flags & GK_EVAL_ASYNC) || opt.time_each || opt.kernel_only;
    // an admission batch (small, evaluated once) never waits for a compiler; an audit-sized or resident table does
    opt.jit_wait = t->resident || t->n_reviews >= 8192;
    {
      { std::lock_guard<std::mutex> gate(e->plan_gate); }   // (a plan change that is waiting goes first)
      std::shared_lock<std::shared_mutex> l(e->plan_rw);
      h->ids = all_ids(e);
      table_results_move(t);
      if (flags & GK_EVAL_WANT_LIST) opt.list_capacity = std::max<uint32_t>(1024, t->n_reviews * 4u);
      table_plans(e, t);   // every plan group: its side of the table, its table-sized variant
      // every plan group is LAUNCHED before any is collected: the groups work on their own streams (sides of the table) and
      // overlap on the device as far as their footprints allow
      if (!(flags & GK_EVAL_COLLECT)) {
        // (several plan groups: their plan-specialised builds are all started first and compile side by side)
        if (e->groups.size() > 1 && opt.jit_wait) each_group(e, t, [&](const GroupAt& g) { dev_jit_prefetch(g.side.plan, g.side.dev); });
        each_group(e, t, [&](const GroupAt& g) { dev_eval_launch(g.side.plan, g.side.dev, opt); });
      }
      if (flags & GK_EVAL_ASYNC) {   // enqueue only; a later call without GK_EVAL_ASYNC collects
        t->ts_pending = true;
        *out = nullptr;
        return GK_OK;
      }
      // collected in group order: the primary group's answer is the call's, the rows of every further group are appended below it
      each_group(e, t, [&](const GroupAt& g) {
        EvalOut& o = h->out;
        if (g.g == 0) { dev_eval_finish(g.side.plan, g.side.dev, opt, &o); dev_tviol_note(g.side.dev, o); dev_tchg_note(g.side.dev, o); h->lds_bytes = o.lds_bytes; return; }
        EvalOut og;
        dev_eval_finish(g.side.plan, g.side.dev, opt, &og);
        dev_tviol_note(g.side.dev, og); dev_tchg_note(g.side.dev, og);
        const uint32_t row_base = o.n_constraints;
        o.viol.insert(o.viol.end(), og.viol.begin(), og.viol.end());
        o.err.insert(o.err.end(), og.err.begin(), og.err.end());
        o.match.insert(o.match.end(), og.match.begin(), og.match.end());
        o.counts.insert(o.counts.end(), og.counts.begin(), og.counts.end());
        for (size_t k = 0; k + 1 < og.list.size(); k += 2) { o.list.push_back(og.list[k] + row_base); o.list.push_back(og.list[k + 1]); }
        for (size_t k = 0; k < og.too_big.size() && k < o.too_big.size(); k++) o.too_big[k] |= og.too_big[k];
        o.list_total += og.list_total;
        o.n_overflow += og.n_overflow;
        o.kernel_ms += og.kernel_ms; o.fast_kernel_ms += og.fast_kernel_ms;
        o.list_bytes += og.list_bytes;
        o.rw_bytes += og.rw_bytes; o.rw_rows += og.rw_rows; o.rw_hdr_rows += og.rw_hdr_rows;
        o.kernel_hash = o.kernel_hash * 1099511628211ull ^ og.kernel_hash;   // (several plan groups: one figure that names all their texts)
        o.n_constraints += og.n_constraints;
        o.d_viol = o.d_err = o.d_counts = nullptr;   // not one contiguous device buffer any more
      });
      t->ts_pending = false;
      t->eval_plan_gen = e->plan_gen;   // (what gk_table_violations streams: these bitmaps, of this plan generation)
    }
    // reviews the device could not evaluate (too_big) are answered by the engine's own exact evaluator where their text is at hand
    if (opt.download && !(flags & GK_EVAL_DEVICE_ONLY)) complete_on_host(e, t, h.get(), opt.want_match, (flags & GK_EVAL_WANT_LIST) != 0);
    else if (opt.download) { std::lock_guard<std::mutex> hl(t->host_mu); t->host_viol.clear(); t->host_err.clear(); t->host_ids.clear(); }
    gk_eval_out& p = h->pub;
    memset(&p, 0, sizeof p);
    p.n_host_evaluated = (uint32_t)h->host_evaluated.size();
    p.host_evaluated = h->host_evaluated.empty() ? nullptr : h->host_evaluated.data();
    p.n_reviews = h->out.n_reviews; p.n_constraints = h->out.n_constraints; p.n_tiles = h->out.n_tiles;
    p.constraint_ids = h->ids.data();
    p.viol = h->out.viol.data(); p.err = h->out.err.data();
    p.match = h->out.match.empty() ? nullptr : h->out.match.data();
    p.too_big = h->out.too_big.data();
    p.counts = h->out.counts.data();
    p.list = h->out.list.data(); p.list_len = (uint32_t)(h->out.list.size() / 2); p.list_total = h->out.list_total;
    p.n_overflow = h->out.n_overflow;
    p.kernel_ms = h->out.kernel_ms; p.fast_kernel_ms = h->out.fast_kernel_ms; p.n_launches = h->out.n_launches;
    p.d_viol = h->out.d_viol; p.d_err = h->out.d_err; p.d_counts = h->out.d_counts;
    p.n_rows = t->n_rows;
    t->last_nc = p.n_constraints; t->last_ids = h->ids;
    p.lds_bytes = h->lds_bytes;
    p.kernel_text_hash = h->out.kernel_hash;
    // algorithmic bytes: rows of the segments whose path carries predicates (+ their string headers
    // where a predicate reads string bytes) + the groups' chunk lists (8 B per entry) + review flags, all read once;
    // plan tables read once; bitmaps written once; 8 B per list entry
    uint64_t rows_read = 0, hdrs_read = 0, bound = 0, plan_bytes = 0;
    std::vector<uint8_t> seen(t->slot_path.size(), 0);   // per slot: 1 = rows counted, 2 = string headers counted (table-once figure)
    uint64_t rows_once = 0, hdrs_once = 0;
    auto account = [&](const HostPlan& hp) {   // every plan group streams its own bound segments
      for (size_t si = 0; si < t->slot_path.size(); si++) {
        const uint32_t pth = t->slot_path[si];
        if (pth >= hp.ptab.size() || !hp.ptab[pth]) continue;
        bound++;
        uint64_t n = pth < t->path_rows.size() ? t->path_rows[pth] : 0;
        rows_read += n;
        uint32_t ent = hp.ptab[pth];
        bool str = false;
        for (uint32_t j = 0; j < (ent & 0xFF); j++) str = str || pred_needs_str(hp.path_preds[(ent >> 8) + j]);
        if (str) hdrs_read += n;
        static const bool dbg_path_rows = getenv("GK_DEBUG_PATH_ROWS") != nullptr;   // (read once)
        if (dbg_path_rows) fprintf(stderr, "[gkgpu paths] %-70s rows %9llu preds %3u%s\n", e->dict.to_string(pth).c_str(), (unsigned long long)n, ent & 0xFF, str ? " +hdr" : "");
        if (!(seen[si] & 1)) { seen[si] |= 1; rows_once += n; }
        if (str && !(seen[si] & 2)) { seen[si] |= 2; hdrs_once += n; }
      }
      plan_bytes += (uint64_t)hp.path_preds.size() * sizeof(Pred) + hp.code.size() * 4 + hp.cheap.size();
    };
    size_t n_groups = 0;
    {
      std::shared_lock<std::shared_mutex> l(e->plan_rw);
      for (auto& g : e->groups) account(g->fast);
      n_groups = e->groups.size();
    }
    // (review words, review_words.hpp: a sweep whose binding evaluated the all-global classes once streams their words -- 4 B per word
    //  and review, padded to 64 reviews -- instead of their rows; the one-off binding pass is not a per-sweep figure)
    const uint64_t rw_rows = std::min<uint64_t>(h->out.rw_rows, rows_read), rw_hdrs = std::min<uint64_t>(h->out.rw_hdr_rows, hdrs_read);
    rows_read -= rw_rows; hdrs_read -= rw_hdrs;
    // (the once-per-table figures: with one plan group a hoisted slot is not streamed at all; with several, a slot hoisted by one group
    //  may be kept by another, which the sums cannot tell -- the figure then stays the upper bound)
    if (n_groups == 1) { rows_once -= std::min(rows_once, rw_rows); hdrs_once -= std::min(hdrs_once, rw_hdrs); }
    p.n_rows_read = rows_read;
    (void)bound;
    p.algo_bytes = rows_read * sizeof(Row) + hdrs_read * sizeof(StrHdr) + h->out.list_bytes + h->out.rw_bytes +
                   t->dir_bytes * n_groups + plan_bytes + (uint64_t)p.n_constraints * p.n_tiles * 16 + (uint64_t)p.list_total * 8;
    p.algo_bytes_once = p.algo_bytes - (rows_read - rows_once) * sizeof(Row) - (hdrs_read - hdrs_once) * sizeof(StrHdr) - t->dir_bytes * (n_groups - 1);   // (the review flags once, not per group)
    p.n_plan_groups = (uint32_t)n_groups;
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const Unsupported& ex) { return fail(GK_ERR_UNSUPPORTED, ex.what());
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

struct TopkHolder {
  gk_topk_out pub;   // first member
  std::vector<uint32_t> ids, counts, reviews, overflow;
};

// object-key order of the table, once: order = the reviews sorted by obj_key, grp = dense key rank with ties equal (what gk_table_topk
// and gk_resident_audit hand to the device)
static void table_key_order(gk_table* t) {
  if (t->order.size() == t->n_reviews) return;
  t->order.resize(t->n_reviews);
  for (uint32_t i = 0; i < t->n_reviews; i++) t->order[i] = i;
  // field-wise order == order of the \0-joined keys (\0 sorts below every byte a name can contain)
  std::stable_sort(t->order.begin(), t->order.end(), [&](uint32_t a, uint32_t b) { return t->obj_key(a) < t->obj_key(b); });
  t->grp.resize(t->n_reviews);
  uint32_t gid = 0;
  for (uint32_t p = 0; p < t->n_reviews; p++) {
    if (p && t->obj_key(t->order[p]) != t->obj_key(t->order[p - 1])) gid++;
    t->grp[p] = gid;
  }
}

int gk_table_topk(gk_engine* e, gk_table* t, uint32_t k, gk_topk_out** out) {
  if (!e || !t || !out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    table_key_order(t);
    std::unique_ptr<TopkHolder> h(new TopkHolder());
    const uint32_t cap = k + 64;
    h->ids = t->last_ids;
    {
      std::shared_lock<std::shared_mutex> l(e->plan_rw);
      each_group(e, t, [&](const GroupAt& g) {   // the groups' rows, appended
        std::vector<uint32_t> r, c, o;
        dev_topk(g.side.dev, g.nc, t->order, t->grp, k, cap, &r, &c, &o);
        append(h->reviews, std::move(r)); append(h->counts, std::move(c)); append(h->overflow, std::move(o));
      });
    }
    // (violating pairs the host evaluation of the last gk_table_eval added are no part of the device bitmaps: they join the candidates
    //  -- a candidate too many costs a rendering, the host sorts and cuts the lists anyway; a full row says "walk the bitmap row")
    std::vector<std::pair<uint32_t, uint32_t>> hv;
    { std::lock_guard<std::mutex> hl(t->host_mu); if (t->host_ids == h->ids) hv = t->host_viol; }   // (another policy set's pairs: dropped)
    if (!hv.empty()) {
      std::vector<std::unordered_set<uint32_t>> have(h->counts.size());   // (a set per touched row, not a linear search per pair)
      for (auto& hp : hv) {
        const uint32_t row = hp.first;
        if (row >= h->counts.size()) continue;
        uint32_t* lst = &h->reviews[(size_t)row * cap];
        if (have[row].empty()) have[row].insert(lst, lst + h->counts[row]);
        if (!have[row].insert(hp.second).second) continue;
        if (h->counts[row] < cap) lst[h->counts[row]++] = hp.second; else h->overflow[row] = 1;
      }
    }
    h->pub.n_constraints = t->last_nc; h->pub.stride = cap;
    h->pub.constraint_ids = h->ids.data(); h->pub.counts = h->counts.data(); h->pub.reviews = h->reviews.data(); h->pub.overflow = h->overflow.data();
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

struct TotalsHolder {
  gk_totals_out pub;   // first member
  std::vector<uint32_t> ids;
  std::vector<uint64_t> results, pairs;
};

// Result-level totals.  The device answers "does (constraint, review) violate" (one bit); the reference counts RESULTS
// (pkg/audit/manager.go:902: totalViolationsPerConstraint[key]++ per types.Result), and a violating pair yields as many
// results as the template's violation set has distinct {msg, details} members for that review.  The violating pairs of
// (the review document of table slot r: kept (GK_TABLE_KEEP_DOCS) or parsed now from the caller's text (GK_TABLE_KEEP_TEXT))
static ReviewDoc make_doc(gk_engine* e, const gk_review_in& in) {
  Value body = parse_json(in.json, in.json_len);
  Value mns = parse_opt(in.namespace_json, in.namespace_len);
  Value nso = parse_opt(in.ns_object_json, in.ns_object_len);
  if (in.kind == GK_REVIEW_OBJECT) return normalize_object(body, mns, nso, in.source, in.operation ? in.operation : "", e->ns_cache);
  return normalize_admission_request(body, mns, nso, in.source, e->ns_cache);
}
static const ReviewDoc* doc_for(gk_engine* e, const gk_table* t, uint32_t r, ReviewDoc* tmp) {
  if (r < t->docs.size()) return &t->docs[r];
  if (r < t->texts.size()) { *tmp = make_doc(e, t->texts[r]); return tmp; }
  auto it = t->big_texts.find(r);   // (written while the table was built, read-only afterwards)
  if (it != t->big_texts.end()) { const gk_review_in in = it->second.in(); *tmp = make_doc(e, in); return tmp; }
  return nullptr;
}

// ---- exact host evaluation of the reviews the device refuses (round 5).  A review with more than 255 elements in an iterated
// array, an object where predicates iterate array elements, or a non-empty container in a value join sets its bit in too_big:
// the kernels never guess.  The reference has no such limit (its audit loop reviews every object, pkg/audit/manager.go:591-642),
// and the engine owns an exact evaluator (ceval.cpp: the one that renders the messages).  So, for every too_big review whose
// text the table holds (kept at flatten time for exactly these reviews):
//   * the MATCH layer is answered by the device from a STRIPPED copy of the review -- object / oldObject cut down to apiVersion,
//     kind and metadata, which is all match.Matches reads (pkg/mutation/match/match.go:32-258) -- flattened into a one-review table
//     and evaluated with GK_EVAL_WANT_MATCH: the same compiled formulas, the same error conditions;
//   * for every constraint that matches, the template's violation set is evaluated on the whole document: a bit per non-empty set.
// The review's too_big bit is cleared and its index reported in gk_eval_out.host_evaluated.  Anything that goes wrong on the way
// (no text, the stripped review refused as well, an evaluation error, a policy change in between) leaves the review in too_big:
// fail closed, as before.
static Value strip_object(const Value& o) {
  if (!o.is_object()) return o;
  ValuePairs keep;
  for (auto& kv : o.pairs()) if (kv.first.is_string() && (kv.first.str() == "apiVersion" || kv.first.str() == "kind" || kv.first.str() == "metadata")) keep.push_back(kv);
  return Value::object(std::move(keep));
}
// (the nested evaluation of a stripped review must never complete on the host again: a stripped review that is still beyond the
//  device's limits -- 300 metadata.ownerReferences iterated by an element-scoped rule -- strips to itself and would recurse without
//  bound; with the guard it takes the "refused as well" branch below and the review stays in too_big: fail closed)
static thread_local int tl_host_completion_depth = 0;
// at most this many refused reviews are completed per evaluation; the rest stay in too_big (fail closed) -- the host evaluator is
// the exception path, not a second engine: a table of a million 300-container pods belongs on the reference driver
static constexpr size_t GK_HOST_COMPLETIONS_MAX = 4096;
static void complete_on_host(gk_engine* e, gk_table* t, EvalHolder* h, bool want_match, bool want_list) {
  EvalOut& o = h->out;
  static const bool env_off = [] { const char* off = getenv("GK_HOST_EVAL"); return off && atoi(off) == 0; }();   // (GK_HOST_EVAL=0, read once: the device's answer alone; per call: GK_EVAL_DEVICE_ONLY)
  static const bool dbg = getenv("GK_DEBUG_HOST") != nullptr;
  auto why = [&](uint32_t r, const char* what) { if (dbg) fprintf(stderr, "[gkgpu host] review %u stays refused: %s\n", r, what); };
  // the pairs this pass adds belong to THIS evaluation: collected locally, published under the table's lock with the constraint-id
  // list they index (gk_table_totals / gk_table_topk drop them when their own list differs)
  std::vector<std::pair<uint32_t, uint32_t>> add_viol, add_err;
  struct Publish {
    gk_table* t; EvalHolder* h; std::vector<std::pair<uint32_t, uint32_t>>*v, *er;
    ~Publish() {
      std::lock_guard<std::mutex> hl(t->host_mu);
      t->host_viol.swap(*v); t->host_err.swap(*er); t->host_ids = h->ids;
      t->host_done = h->host_evaluated; t->host_gen = t->ts_gen;   // (gk_table_violations: the pairs of THIS evaluation)
    }
  } publish{t, h, &add_viol, &add_err};
  if (env_off || tl_host_completion_depth > 0) return;
  struct Depth { Depth() { tl_host_completion_depth++; } ~Depth() { tl_host_completion_depth--; } } depth_guard;
  const uint32_t nt = o.n_tiles, nc = o.n_constraints;
  if (nc == 0 || h->ids.size() != nc) return;
  // ---- the candidates: refused reviews whose text is at hand
  struct Cand { uint32_t r; gk_review_in in; bool prem; std::string stext; int mrow = -1; };
  std::vector<Cand> cands;
  for (uint32_t w = 0; w < nt && w < o.too_big.size(); w++)
    for (uint64_t m = o.too_big[w]; m; m &= m - 1) {
      const uint32_t r = w * GK_TILE + (uint32_t)__builtin_ctzll(m);
      if (r >= t->n_reviews) continue;
      if (cands.size() >= GK_HOST_COMPLETIONS_MAX) { why(r, "more refused reviews than one evaluation completes"); continue; }
      Cand c;
      c.r = r;
      if (r < t->texts.size()) c.in = t->texts[r];
      else { auto it = t->big_texts.find(r); if (it == t->big_texts.end()) { why(r, "no text kept"); continue; } c.in = it->second.in(); }
      c.prem = r < t->host.rflags.size() && (t->host.rflags[r] & RF_PREMATCHED) != 0;
      cands.push_back(std::move(c));
    }
  if (cands.empty()) return;
  // ---- 1. match layer: the stripped reviews on the device, ONE table and ONE launch for all of them -- unless the caller ran
  //         Matcher.Match itself (RF_PREMATCHED: every constraint counts as matching, nothing is autorejected)
  std::vector<gk_review_in> sins;
  for (Cand& c : cands) {
    if (c.prem) continue;
    try {
      Value body = parse_json(c.in.json, c.in.json_len);
      if (!body.is_object()) { why(c.r, "not an object"); continue; }
      Value stripped;
      if (c.in.kind == GK_REVIEW_OBJECT) stripped = strip_object(body);
      else {
        ValuePairs kv = body.pairs();
        for (auto& pr : kv) if (pr.first.is_string() && (pr.first.str() == "object" || pr.first.str() == "oldObject")) pr.second = strip_object(pr.second);
        stripped = Value::object(std::move(kv));
      }
      c.stext = to_json(stripped);
      c.mrow = (int)sins.size();
      sins.push_back(c.in);
    } catch (const std::exception& ex) { why(c.r, ex.what()); }
  }
  for (Cand& c : cands) if (c.mrow >= 0) { sins[c.mrow].json = c.stext.data(); sins[c.mrow].json_len = c.stext.size(); }   // (after the loop: the strings no longer move)
  gk_table* mt = nullptr;
  gk_eval_out* mo = nullptr;
  std::vector<int32_t> mst(sins.size(), GK_OK);
  std::unique_ptr<gk_table, void (*)(gk_table*)> mt_guard(nullptr, gk_table_free);
  std::unique_ptr<gk_eval_out, void (*)(gk_eval_out*)> mo_guard(nullptr, gk_eval_free);
  bool match_ok = sins.empty();
  if (!sins.empty()) {
    if (gk_table_create(e, sins.data(), sins.size(), 0, mst.data(), &mt) == GK_OK && mt) {
      mt_guard.reset(mt);
      if (gk_table_eval(e, mt, GK_EVAL_WANT_MATCH | GK_EVAL_DEVICE_ONLY, &mo) == GK_OK && mo) {
        mo_guard.reset(mo);
        match_ok = mo->n_constraints == nc && mo->match != nullptr;
        for (uint32_t row = 0; row < nc && match_ok; row++) match_ok = mo->constraint_ids[row] == h->ids[row];   // (else: the policy set changed between the two evaluations)
      }
    }
    if (!match_ok && dbg) fprintf(stderr, "[gkgpu host] the stripped reviews' match table failed: %s\n", gk_last_error());
  }
  // ---- 2. violations: the template's violation set on the whole document, for the constraints that match; 3. the answer replaces the refusal
  for (Cand& c : cands) {
    const uint32_t r = c.r, w = r / GK_TILE;
    const uint64_t bit = 1ull << (r % GK_TILE);
    try {
      std::vector<uint8_t> v(nc, 0), er(nc, 0), ma(nc, c.prem ? 1 : 0);
      if (!c.prem) {
        if (c.mrow < 0 || !match_ok) { why(r, "no match answer"); continue; }
        if (mst[c.mrow] != GK_OK) { why(r, "stripped review rejected"); continue; }
        const uint32_t mw = (uint32_t)c.mrow / GK_TILE;
        const uint64_t mbit = 1ull << ((uint32_t)c.mrow % GK_TILE);
        if (mo->too_big[mw] & mbit) { why(r, "stripped review refused as well"); continue; }
        for (uint32_t row = 0; row < nc; row++) {
          er[row] = (mo->err[(size_t)row * mo->n_tiles + mw] & mbit) ? 1 : 0;
          ma[row] = (mo->match[(size_t)row * mo->n_tiles + mw] & mbit) ? 1 : 0;
        }
      }
      ReviewDoc tmp;
      const ReviewDoc* doc = doc_for(e, t, r, &tmp);
      if (!doc) { why(r, "no document"); continue; }
      {
        std::shared_lock<std::shared_mutex> l(e->mu);
        for (uint32_t row = 0; row < nc; row++) {
          if (!ma[row]) continue;
          const ConstraintRec& cr = e->constraints[h->ids[row]];
          auto it = e->templates.find(lower_str(cr.kind));
          if (it == e->templates.end()) throw std::runtime_error("no template");
          v[row] = it->second->render(doc->request, cr.params, e->inventory).empty() ? 0 : 1;
        }
      }
      for (uint32_t row = 0; row < nc; row++) {
        uint64_t& vw = o.viol[(size_t)row * nt + w];
        uint64_t& ew = o.err[(size_t)row * nt + w];
        if ((vw & bit) && row < o.counts.size() && o.counts[row]) o.counts[row]--;   // (never set for a refused review; kept consistent anyway)
        vw &= ~bit; ew &= ~bit;
        if (v[row]) { vw |= bit; if (row < o.counts.size()) o.counts[row]++; add_viol.emplace_back(row, r); if (want_list) { o.list.push_back(row); o.list.push_back(r); o.list_total++; } }
        if (er[row]) { ew |= bit; add_err.emplace_back(row, r); }
        if (want_match && !o.match.empty()) { uint64_t& mw = o.match[(size_t)row * nt + w]; mw = ma[row] ? (mw | bit) : (mw & ~bit); }
      }
      o.too_big[w] &= ~bit;
      h->host_evaluated.push_back(r);
    } catch (const std::exception& ex) {
      why(r, ex.what());
      // (an evaluation error, a document that does not parse: the review stays refused -- fail closed)
    }
  }
}

// Which violating pairs have to be RENDERED to know their result count: need[row][tile], a subset of viol.  The totals plans
// (ensure_totals_plans) answer "this review may yield more than one result" per constraint on the device; a violating pair
// they do not flag has exactly one result.  Everything they cannot answer stays in: constraints without a multi formula,
// reviews beyond the totals plans' limits, GK_TOTALS_RENDER_ALL=1 (test aid: the host pass over every violating pair, as
// before round 3).  Caller holds plan_rw shared and mu shared; ensure_plan ran; ids = constraint id per bitmap row.
// `counted[row]` (round 4): the device COUNTED the results of the row's unflagged pairs -- `sum[row]` of them -- instead of deciding
// "exactly one".
static std::vector<uint64_t> render_needed(gk_engine* e, gk_table* t, const std::vector<uint32_t>& ids, uint32_t nt, const std::vector<uint64_t>& viol,
                                           std::vector<uint8_t>* counted, std::vector<uint64_t>* sum) {
  std::vector<uint64_t> need = viol;
  counted->assign(ids.size(), 0); sum->assign(ids.size(), 0);
  if (getenv("GK_TOTALS_RENDER_ALL") || t->n_reviews == 0) return need;
  if (table_stale(e, t)) return need;   // (a table flattened before the constraint set changed: no totals plan can read it)
  std::lock_guard<std::mutex> tl(e->totals_mu);
  ensure_totals_plans(e);
  if (e->totals_groups.empty()) return need;
  std::map<uint32_t, uint32_t> row_of;
  for (uint32_t r = 0; r < ids.size(); r++) row_of[ids[r]] = r;
  EvalOptions opt;
  opt.download = true;
  opt.jit_wait = false;   // one pass per audit: the bytecode kernel serves it unless the specialised build is there already
  while (t->tviews.size() < e->totals_groups.size()) t->tviews.push_back(dev_table_view(t->dev));
  std::vector<uint64_t> beyond(nt, 0);
  std::vector<uint8_t> answered(ids.size(), 0);   // 1: a multi row, 2: a flag row (count rows follow)
  std::vector<uint64_t> multi((size_t)ids.size() * nt, 0);
  std::vector<std::vector<uint64_t>> count_rows;   // count rows of all groups, with the main row they belong to
  std::vector<uint32_t> count_main;
  // (the groups are launched in waves: each holds a view of the table -- a stream and result buffers of its own)
  const size_t wave = 8;
  // A PRUNED table holds rows of the published read set only (publish_read_set: the main plans and the counting forms' paths).  A
  // totals plan that has a predicate on any other path -- the lazily prepared "more than one result?" formulas are not published --
  // would read "absent" where the object has a value: its rows stay unanswered for this table and their pairs are rendered
  // (round-4 advisor finding: nothing enforced that compile_multi reads the violation formula's paths only)
  std::vector<uint8_t> usable(e->totals_groups.size(), 1);
  if (t->pruned)
    for (size_t gi = 0; gi < e->totals_groups.size(); gi++)
      for (const HostPlan* hp : {&e->totals_groups[gi]->fast, &e->totals_groups[gi]->big})
        for (const Pattern& pat : hp->pred_patterns) if (!e->dict_reg.reads_has(pat)) { usable[gi] = 0; if (getenv("GK_DEBUG_MULTI")) fprintf(stderr, "[gkgpu totals] plan %zu reads %s: not in the pruned table's read set\n", gi, pattern_to_string(pat).c_str()); }
  // (a constraint's flag row and its count rows may sit in different plans: with ANY of them unanswered its pairs are rendered -- a flag
  //  row that says "counted" with a count row missing would undercount)
  std::vector<uint8_t> blocked(ids.size(), 0);
  for (size_t gi = 0; gi < e->totals_groups.size(); gi++)
    if (!usable[gi]) for (uint32_t id : e->totals_groups[gi]->ids) { auto it = row_of.find(id); if (it != row_of.end()) blocked[it->second] = 1; }
  for (size_t g0 = 0; g0 < e->totals_groups.size(); g0 += wave) {
    const size_t g1 = std::min(e->totals_groups.size(), g0 + wave);
    for (size_t gi = g0; gi < g1; gi++) if (usable[gi]) dev_eval_launch(e->totals_groups[gi]->dev, t->tviews[gi], opt);
    for (size_t gi = g0; gi < g1; gi++) {
      if (!usable[gi]) continue;
      EvalOut og;
      dev_eval_finish(e->totals_groups[gi]->dev, t->tviews[gi], opt, &og);
      const gk_engine::Group& G = *e->totals_groups[gi];
      for (uint32_t w = 0; w < nt && w < og.too_big.size(); w++) beyond[w] |= og.too_big[w];
      for (uint32_t r = 0; r < G.ids.size() && r < og.n_constraints; r++) {
        auto it = row_of.find(G.ids[r]);
        if (it == row_of.end() || og.n_tiles != nt || blocked[it->second]) continue;
        const uint8_t role = r < G.roles.size() ? G.roles[r] : (uint8_t)TR_MULTI;
        const uint64_t* bits = &og.viol[(size_t)r * nt];
        // (autoreject pairs of the totals plan are the main plan's: they carry no violation bit either way)
        if (role == TR_COUNT) { count_rows.emplace_back(bits, bits + nt); count_main.push_back(it->second); continue; }
        answered[it->second] = role == TR_FLAG ? 2 : 1;
        for (uint32_t w = 0; w < nt; w++) multi[(size_t)it->second * nt + w] = bits[w];
      }
    }
  }
  for (uint32_t r = 0; r < ids.size(); r++) {
    if (!answered[r]) continue;
    for (uint32_t w = 0; w < nt; w++) need[(size_t)r * nt + w] = viol[(size_t)r * nt + w] & (multi[(size_t)r * nt + w] | beyond[w]);
    if (answered[r] == 2) (*counted)[r] = 1;
  }
  for (size_t k = 0; k < count_rows.size(); k++) {
    const uint32_t r = count_main[k];
    if (!(*counted)[r]) continue;   // (its flag row is missing: the pairs are rendered)
    uint64_t n = 0;
    for (uint32_t w = 0; w < nt; w++) n += (uint64_t)__builtin_popcountll(count_rows[k][w] & viol[(size_t)r * nt + w] & ~need[(size_t)r * nt + w]);
    (*sum)[r] += n;
  }
  if (getenv("GK_DEBUG_COUNT_CHECK")) {   // debugging aid: every counted pair is rendered as well and compared, review by review
    int shown = 0;
    for (uint32_t r = 0; r < ids.size() && shown < 12; r++) {
      if (!(*counted)[r]) continue;
      const ConstraintRec& c = e->constraints[ids[r]];
      auto itt = e->templates.find(lower_str(c.kind));
      for (uint32_t i = 0; i < t->n_reviews && shown < 12; i++) {
        const uint32_t w = i / 64; const uint64_t b = 1ull << (i % 64);
        if (!(viol[(size_t)r * nt + w] & b) || (need[(size_t)r * nt + w] & b)) continue;
        uint32_t dev = 0;
        for (size_t k = 0; k < count_rows.size(); k++) if (count_main[k] == r && (count_rows[k][w] & b)) dev++;
        ReviewDoc tmp;
        const ReviewDoc* doc = doc_for(e, t, i, &tmp);
        const size_t host = doc ? itt->second->render(doc->request, c.params, e->inventory).size() : 0;
        if (host != dev) { shown++; fprintf(stderr, "[gkgpu count check] %s/%s review %u: device %u, renderer %zu\n", c.kind.c_str(), c.name.c_str(), i, dev, host); }
      }
    }
  }
  return need;
}

// the table's most recent evaluation are rendered on host threads (the reference renders -- and logs -- every message
// as well, manager.go:926-928); only the counts are kept.
int gk_table_totals(gk_engine* e, gk_table* t, gk_totals_out** out) {
  if (!e || !t || !out) return fail(GK_ERR_INVALID, "NULL argument");
  if (t->docs.size() != t->n_reviews && t->texts.size() != t->n_reviews) return fail(GK_ERR_INVALID, "table was created without GK_TABLE_KEEP_DOCS / GK_TABLE_KEEP_TEXT");
  try {
    std::unique_ptr<TotalsHolder> h(new TotalsHolder());
    h->ids = t->last_ids;
    const uint32_t nc = t->last_nc, nt = (t->n_reviews + GK_TILE - 1) / GK_TILE;
    std::vector<uint64_t> viol;
    {
      std::shared_lock<std::shared_mutex> l(e->plan_rw);
      each_group(e, t, [&](const GroupAt& g) {
        std::vector<uint64_t> v;
        dev_last_viol(g.side.dev, g.nc, &v);
        append(viol, std::move(v));
      });
    }
    if (viol.size() != (size_t)nc * nt) return fail(GK_ERR_INVALID, "gk_table_totals: evaluate the table first");
    h->results.assign(nc, 0); h->pairs.assign(nc, 0);
    ensure_plan(e);
    std::shared_lock<std::shared_mutex> pl(e->plan_rw);
    std::shared_lock<std::shared_mutex> rl(e->mu);
    // Round 3: the device decides which violating pairs CAN have more than one result; every other violating pair counts one
    // result without being rendered (configs[2]: 1.8 M violating pairs, ~1 % of them rendered)
    std::vector<uint8_t> counted;
    std::vector<uint64_t> counted_sum;
    // (pairs the host evaluation of the last gk_table_eval added are no part of the device bitmaps: they join here and are rendered)
    std::vector<std::pair<uint32_t, uint32_t>> hv;
    { std::lock_guard<std::mutex> hl(t->host_mu); if (t->host_ids == h->ids) hv = t->host_viol; }   // (another policy set's pairs: dropped)
    for (auto& hp : hv) if (hp.first < nc && hp.second / GK_TILE < nt) viol[(size_t)hp.first * nt + hp.second / GK_TILE] |= 1ull << (hp.second % GK_TILE);
    std::vector<uint64_t> need = render_needed(e, t, h->ids, nt, viol, &counted, &counted_sum);
    for (auto& hp : hv) if (hp.first < nc && hp.second / GK_TILE < nt) need[(size_t)hp.first * nt + hp.second / GK_TILE] |= 1ull << (hp.second % GK_TILE);
    for (uint32_t row = 0; row < nc; row++) {
      for (uint32_t w = 0; w < nt; w++) {
        const uint64_t v = viol[(size_t)row * nt + w];
        h->pairs[row] += (uint64_t)__builtin_popcountll(v);
        if (!counted[row]) h->results[row] += (uint64_t)__builtin_popcountll(v & ~need[(size_t)row * nt + w]);   // exactly one result each
      }
      if (counted[row]) h->results[row] += counted_sum[row];   // (round 4) counted on the device: as many as their count rows say
    }
    uint64_t n_rendered = 0;
    for (uint64_t x : need) n_rendered += (uint64_t)__builtin_popcountll(x);
    h->pub.rendered_pairs = n_rendered;
    struct CRef { const ConstraintRec* c; const Template* tm; };
    std::vector<CRef> cref(nc);
    for (uint32_t row = 0; row < nc; row++) {
      const ConstraintRec& c = e->constraints[h->ids[row]];
      auto it = e->templates.find(lower_str(c.kind));
      if (it == e->templates.end()) return fail(GK_ERR_NOT_FOUND, "unknown constraint template validator: " + c.kind);
      cref[row] = {&c, it->second.get()};
    }
    size_t n_threads = std::max<size_t>(1, std::min<size_t>(host_cpus(), nt / 4 + 1));
    if (const char* ht = getenv("GK_HOST_THREADS")) n_threads = std::max(1, atoi(ht));
    std::vector<std::vector<uint64_t>> part_r(n_threads, std::vector<uint64_t>(nc, 0));
    std::vector<std::string> errs(n_threads);
    std::atomic<uint32_t> next_tile{0};
    auto work = [&](size_t w) {
      try {
        for (;;) {
          const uint32_t tl = next_tile.fetch_add(1);
          if (tl >= nt) break;
          // review-major: a violating review is parsed (GK_TABLE_KEEP_TEXT) at most once, then rendered for each of its constraints
          uint64_t any = 0;
          for (uint32_t row = 0; row < nc; row++) any |= need[(size_t)row * nt + tl];
          for (uint64_t m = any; m; m &= m - 1) {
            const uint32_t b = (uint32_t)__builtin_ctzll(m), r = tl * GK_TILE + b;
            ReviewDoc tmp;
            const ReviewDoc* doc = doc_for(e, t, r, &tmp);
            if (!doc) throw std::runtime_error("review document unavailable");
            for (uint32_t row = 0; row < nc; row++) {
              if (!((need[(size_t)row * nt + tl] >> b) & 1ull)) continue;
              part_r[w][row] += cref[row].tm->render(doc->request, cref[row].c->params, e->inventory).size();
            }
          }
        }
      } catch (const std::exception& ex) { errs[w] = ex.what(); }
    };
    HostWorkers::get().run(n_threads, work);
    for (auto& er : errs) if (!er.empty()) return fail(GK_ERR_REGO, er);
    for (size_t w = 0; w < n_threads; w++) for (uint32_t row = 0; row < nc; row++) h->results[row] += part_r[w][row];
    h->pub.n_constraints = nc; h->pub.constraint_ids = h->ids.data(); h->pub.results = h->results.data(); h->pub.pairs = h->pairs.data();
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_totals_free(gk_totals_out* o) {
  if (o) delete reinterpret_cast<TotalsHolder*>(o);
}

void gk_topk_free(gk_topk_out* o) {
  if (o) delete reinterpret_cast<TopkHolder*>(o);
}

void gk_eval_free(gk_eval_out* o) {
  if (!o) return;
  delete reinterpret_cast<EvalHolder*>(o);   // pub is the first member
}

int gk_render(gk_engine* e, gk_table* t, uint32_t constraint_id, uint32_t review, char** json_out) {
  if (!e || !t || !json_out) return fail(GK_ERR_INVALID, "NULL argument");
  if (t->docs.empty() && t->texts.empty()) return fail(GK_ERR_INVALID, "table was created without GK_TABLE_KEEP_DOCS / GK_TABLE_KEEP_TEXT");
  if (review >= std::max(t->docs.size(), t->texts.size())) return fail(GK_ERR_INVALID, "review index out of range");
  try {
    std::shared_lock<std::shared_mutex> l(e->mu);
    if (constraint_id >= e->constraints.size()) return fail(GK_ERR_NOT_FOUND, "unknown constraint id");
    const ConstraintRec& c = e->constraints[constraint_id];
    auto it = e->templates.find(lower_str(c.kind));
    if (it == e->templates.end()) return fail(GK_ERR_NOT_FOUND, "unknown constraint template validator: " + c.kind);
    ReviewDoc tmp;
    const ReviewDoc& doc = *doc_for(e, t, review, &tmp);
    ValueVec arr;
    auto vs = it->second->render(doc.request, c.params, e->inventory);
    for (auto& v : vs) {
      static const Value k_msg = Value::string("msg"), k_details = Value::string("details"), no_details = Value::object({});
      ValuePairs o{{k_details, v.details.defined() ? v.details : no_details}, {k_msg, Value::string(v.msg)}};
      arr.push_back(Value::object(o));
    }
    std::string s = to_json(Value::array(arr));
    char* buf = (char*)malloc(s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    *json_out = buf;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_REGO, ex.what()); }
}

int gk_render_error(gk_engine* e, gk_table* t, uint32_t constraint_id, uint32_t review, char** json_out) {
  if (!e || !t || !json_out) return fail(GK_ERR_INVALID, "NULL argument");
  if (review >= std::max(t->docs.size(), t->texts.size())) return fail(GK_ERR_INVALID, "review index out of range (needs GK_TABLE_KEEP_DOCS / GK_TABLE_KEEP_TEXT)");
  std::shared_lock<std::shared_mutex> l(e->mu);
  if (constraint_id >= e->constraints.size()) return fail(GK_ERR_NOT_FOUND, "unknown constraint id");
  ReviewDoc tmp;
  std::string msg;
  try { msg = autoreject_message(e->constraints[constraint_id].match, *doc_for(e, t, review, &tmp)); } catch (const std::exception& ex) { return fail(GK_ERR_REGO, ex.what()); }
  ValuePairs o{{Value::string("msg"), Value::string(msg)}, {Value::string("autoreject"), Value::boolean(true)}, {Value::string("details"), Value::object({})}};
  std::string s = to_json(Value::array({Value::object(o)}));
  char* buf = (char*)malloc(s.size() + 1);
  memcpy(buf, s.c_str(), s.size() + 1);
  *json_out = buf;
  return GK_OK;
}

void gk_free(void* p) { free(p); }

// ------------------------------------------------------------------------------------------------ micro-batcher (row f1)
namespace {

// results of ONE review of an evaluated table as the JSON gk_query returns; renders from `doc` (parsed lazily: most
// admission reviews violate nothing and never become a Value tree)
// `wanted` (may be NULL): sorted constraint ids the caller asked about (Driver.Query's `constraints`); others are not rendered
std::string query_results_json(gk_engine* e, gk_table* t, const gk_eval_out& ev, uint32_t r, const gk_review_in& in, bool* too_big,
                               const std::vector<uint32_t>* wanted = nullptr) {
  const uint32_t nt = ev.n_tiles, w = r / GK_TILE;
  const uint64_t bit = 1ull << (r % GK_TILE);
  *too_big = (ev.too_big[w] & bit) != 0;
  std::string out = "[";
  bool have_doc = false;
  ReviewDoc doc;
  auto need_doc = [&]() {
    if (have_doc) return;
    Value body = parse_json(in.json, in.json_len);
    Value mns = parse_opt(in.namespace_json, in.namespace_len);
    Value nso = parse_opt(in.ns_object_json, in.ns_object_len);
    if (in.kind == GK_REVIEW_OBJECT) doc = normalize_object(body, mns, nso, in.source, in.operation ? in.operation : "", e->ns_cache);
    else doc = normalize_admission_request(body, mns, nso, in.source, e->ns_cache);
    have_doc = true;
  };
  std::shared_lock<std::shared_mutex> l(e->mu);
  for (uint32_t row = 0; row < ev.n_constraints; row++) {
    const bool is_err = (ev.err[(size_t)row * nt + w] & bit) != 0, is_viol = (ev.viol[(size_t)row * nt + w] & bit) != 0;
    if (!is_err && !is_viol) continue;
    const uint32_t cid = ev.constraint_ids[row];
    if (wanted && !std::binary_search(wanted->begin(), wanted->end(), cid)) continue;
    const ConstraintRec& c = e->constraints[cid];
    need_doc();
    if (is_err) {
      ValuePairs o{{Value::string("constraint"), Value::integer(cid)}, {Value::string("msg"), Value::string(autoreject_message(c.match, doc))},
                   {Value::string("autoreject"), Value::boolean(true)}, {Value::string("details"), Value::object({})}};
      if (out.size() > 1) out += ",";
      out += to_json(Value::object(o));
      continue;
    }
    auto it = e->templates.find(lower_str(c.kind));
    // the device flagged this pair: a template that has gone, or a renderer that finds nothing, is a disagreement between
    // the plan and the evaluator -- an error for the caller (Client.ReviewBatch treats it the same way), never "no results"
    if (it == e->templates.end()) throw std::runtime_error("device / renderer disagree: constraint " + c.kind + "/" + c.name + " has no template");
    const auto vs = it->second->render(doc.request, c.params, e->inventory);
    if (vs.empty()) throw std::runtime_error("device / renderer disagree: the plan reports a violation of " + c.kind + "/" + c.name + " that the evaluator does not render");
    for (auto& v : vs) {
      static const Value k_constraint = Value::string("constraint"), k_msg = Value::string("msg"), k_details = Value::string("details"), no_details = Value::object({});
      ValuePairs o{{k_constraint, Value::integer(cid)}, {k_details, v.details.defined() ? v.details : no_details}, {k_msg, Value::string(v.msg)}};   // (in key order: Value::object has nothing to sort)
      if (out.size() > 1) out += ",";
      out += to_json(Value::object(o));
    }
  }
  return out + "]";
}

}  // namespace
struct gk_engine::BatchResult {
  gk_table* table = nullptr;
  gk_eval_out* ev = nullptr;
  ~BatchResult() { if (ev) gk_eval_free(ev); if (table) gk_table_free(table); }
};
namespace {

void batcher_loop(gk_engine* e) {
  gk_engine::Batcher& B = e->batcher;
  for (;;) {
    std::vector<gk_engine::Request*> batch;
    {
      std::unique_lock<std::mutex> l(B.mu);
      B.cv.wait(l, [&] { return B.stop || !B.queue.empty(); });
      if (B.stop && B.queue.empty()) return;
      // the first request of a batch waits up to window_us for company (or until max_batch requests are queued)
      const auto deadline = B.queue.front()->arrived + std::chrono::microseconds(B.opts.window_us);
      B.cv.wait_until(l, deadline, [&] { return B.stop || B.queue.size() >= B.opts.max_batch; });
      while (!B.queue.empty() && batch.size() < B.opts.max_batch) { batch.push_back(B.queue.front()); B.queue.pop_front(); }
    }
    const auto t_start = std::chrono::steady_clock::now();
    std::vector<gk_review_in> ins;
    std::vector<uint8_t> prem;
    bool any_prem = false;
    for (auto* r : batch) { ins.push_back(*r->in); prem.push_back(r->pre_matched ? 1 : 0); any_prem = any_prem || r->pre_matched; }
    std::vector<int32_t> st(batch.size(), GK_OK);
    auto br = std::make_shared<gk_engine::BatchResult>();
    // an admission batch serves the policy set loaded now and is evaluated once: a PRUNED table (rows of the key paths that set reads,
    // the ingest walks past the rest).  A constraint that arrives between the two calls makes it stale: built again, once
    int rc = GK_OK;
    std::string err;
    { std::lock_guard<std::mutex> turn(e->policy_gate); }   // (a policy change that is waiting goes first)
    std::shared_lock<std::shared_mutex> policy_epoch(e->policy_rw);   // the policy set does not change between the flatten and the launch
    for (int attempt = 0; attempt < 3; attempt++) {   // (what can still make the table stale: a referential constraint recompiled against a changed inventory)
      if (br->table) { gk_table_free(br->table); br->table = nullptr; }
      rc = table_create_impl(e, ins.data(), ins.size(), attempt < 2 ? GK_TABLE_PRUNED : 0u, st.data(), any_prem ? prem.data() : nullptr, &br->table);
      err = rc == GK_OK ? "" : gk_last_error();
      if (rc != GK_OK) break;
      rc = gk_table_eval(e, br->table, 0, &br->ev);
      if (rc == GK_OK) break;
      err = gk_last_error();
      if (rc != GK_ERR_INVALID) break;
    }
    policy_epoch.unlock();
    const double dev_us = br->ev ? br->ev->kernel_ms * 1e3 : 0;
    for (size_t i = 0; i < batch.size(); i++) {
      gk_engine::Request* r = batch[i];
      r->batch_size = (uint32_t)batch.size();
      r->queue_us = std::chrono::duration<double, std::micro>(t_start - r->arrived).count();
      r->device_us = dev_us;
      r->index = (uint32_t)i;
      if (rc != GK_OK) { r->status = rc; r->error = err; }
      else if (st[i] != GK_OK) { r->status = GK_ERR_REVIEW; r->error = br->table->review_errors[i]; }
      else r->batch = br;   // the caller renders its own results (gk_query): rendering runs in parallel across callers
    }
    {
      std::lock_guard<std::mutex> l(B.mu);
      B.batches++; B.reviews += batch.size();
      for (auto* r : batch) { r->done = true; r->cv.notify_one(); }
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ multi-GPU (row e)
int gk_comm_unique_id(char id[GK_COMM_ID_BYTES]) {
  std::string err;
  if (!id) return fail(GK_ERR_INVALID, "NULL argument");
  if (!dev_comm_unique_id(id, &err)) return fail(GK_ERR_DEVICE, err);
  return GK_OK;
}

int gk_comm_init(gk_engine* e, const char id[GK_COMM_ID_BYTES], int rank, int world) {
  if (!e || !id || rank < 0 || world < 1 || rank >= world) return fail(GK_ERR_INVALID, "bad argument");
  std::string err;
  DevComm* c = dev_comm_init(e->opts.device, id, rank, world, &err);
  if (!c) return fail(GK_ERR_DEVICE, err);
  if (e->comm) dev_comm_free(e->comm);
  e->comm = c;
  return GK_OK;
}

// used by the test-only CPU emulation (tests/native/hostemu.cpp): adopt a communicator built elsewhere
int gk_comm_init_host_impl(gk_engine* e, DevComm* c) { if (!e || !c) return GK_ERR_INVALID; if (e->comm) dev_comm_free(e->comm); e->comm = c; return GK_OK; }

void gk_comm_destroy(gk_engine* e) { if (e && e->comm) { dev_comm_free(e->comm); e->comm = nullptr; } }

int gk_comm_info(gk_engine* e, int32_t* rank, int32_t* world) {
  if (!e || !rank || !world) return fail(GK_ERR_INVALID, "NULL argument");
  if (!e->comm) return fail(GK_ERR_INVALID, "gk_comm_init first");
  std::string err;
  int r = 0, w = 0;
  if (!dev_comm_query(e->comm, &r, &w, &err)) return fail(GK_ERR_DEVICE, err);
  *rank = r; *world = w;
  return GK_OK;
}

struct ShardHolder {
  gk_shard_out pub;   // first member
  std::vector<uint32_t> ids, shard_reviews;
  std::vector<int64_t> totals, err_totals;
  std::vector<uint64_t> gathered;
  uint64_t merged_slot = 0;
};

int gk_table_sweep_sharded(gk_engine* e, gk_table* t, uint32_t flags, gk_shard_out** out) {
  const bool enqueue = (flags & GK_SHARD_ENQUEUE) != 0;
  if (!e || !t || (!out && !enqueue)) return fail(GK_ERR_INVALID, "NULL argument");
  if (!e->comm) return fail(GK_ERR_INVALID, "gk_comm_init first");
  try {
    ensure_plan(e);
    if (const char* why = table_stale(e, t)) return fail(GK_ERR_INVALID, why);
    std::unique_ptr<ShardHolder> h(new ShardHolder());
    std::shared_lock<std::shared_mutex> l(e->plan_rw);
    table_sides(e, t);
    { std::lock_guard<std::mutex> vl(e->variants_mu); plan_for_group(e, t, 0); }
    // (here only the primary group runs its table-sized variant; the further groups run their base plans)
    auto plan_of = [](const GroupAt& g) { const DevPlan* p = g.grp.dev; if (g.g == 0) p = g.side.plan; return p; };
    const size_t n_groups = e->groups.size();
    const ShardInfo& shard0 = t->sides[0].shard;
    table_results_move(t);
    if (t->shard_gen != e->plan_gen || shard0.shard_reviews.empty()) {   // (collective) once per table and plan
      each_group(e, t, [&](const GroupAt& g) { dev_shard_setup(g.side.dev, e->comm, g.nc, &g.side.shard); });
      t->shard_gen = e->plan_gen;
    }
    EvalOptions opt;
    opt.download = false;
    opt.shard = true;
    opt.jit_wait = true;   // a shard of the audit set is a resident table: the plan-specialised kernel or nothing
    if (t->n_rejected == ~0ull) {   // (a table's reviews never change: counted once, not per sweep -- a million strings)
      uint64_t nr = 0;
      for (const std::string& er : t->review_errors) if (!er.empty()) nr++;
      t->n_rejected = nr;
    }
    const uint64_t rejected = t->n_rejected;
    if (enqueue) {   // sweep + exchange of every plan group onto the stream(s); whoever collects waits for them
      // (four enqueues per plan group; GK_SHARD_GRAPH=1: a single plan group's step replays as one captured graph)
      each_group(e, t, [&](const GroupAt& g) { dev_shard_enqueue(plan_of(g), g.side.dev, e->comm, opt, g.nc, rejected, n_groups == 1); });
      if (out) *out = nullptr;
      return GK_OK;
    }
    // Per plan group: the local evaluation, finished (incl. the large-capacity pass for overflowing reviews) BEFORE the exchange, so
    // that the gathered bitmaps are complete; then the exchange step on the same stream (each group has its own slot buffer on its
    // side of the table).  GK_SHARD_COLLECT, one plan group only: the answer of the last enqueue-only pass, without sweeping again --
    // unless some review of that pass, on any rank, was left to the large-capacity re-run (then this is an ordinary collecting sweep;
    // every rank decides alike).
    // What the bitmaps cannot say travels with the totals (fail closed, like Client.AuditAggregate): autoreject pairs, reviews
    // beyond the engine's limits, reviews HandleReview rejected when this shard was built
    EvalOut eo;
    const void* d_all = nullptr;
    const bool want_host = (flags & GK_SHARD_DOWNLOAD) != 0;
    std::vector<std::vector<uint64_t>> parts(n_groups);   // the groups' gathered slots (host copies)
    int64_t beyond = 0, not_eval = 0;
    uint32_t nc = 0;
    bool collected = false;
    each_group(e, t, [&](const GroupAt& g) {
      std::vector<int64_t> raw;   // [nc] pairs | [nc] autoreject | beyond | not evaluated | left to the re-run
      std::vector<uint64_t>* host = want_host ? &parts[g.g] : nullptr;
      if ((flags & GK_SHARD_COLLECT) && n_groups == 1) collected = dev_shard_collect(g.side.dev, e->comm, g.nc, &raw, host, &d_all);
      if (!collected) {
        EvalOut og;
        dev_eval(plan_of(g), g.side.dev, opt, &og);
        eo.kernel_ms += og.kernel_ms; eo.fast_kernel_ms += og.fast_kernel_ms; eo.n_overflow += og.n_overflow;
        dev_shard_exchange(g.side.dev, e->comm, g.nc, rejected, &raw, host, &d_all);
      }
      h->err_totals.insert(h->err_totals.end(), raw.begin() + g.nc, raw.begin() + 2 * (size_t)g.nc);
      beyond += raw[2 * (size_t)g.nc];
      if (g.g == 0) not_eval = raw[2 * (size_t)g.nc + 1];
      h->totals.insert(h->totals.end(), raw.begin(), raw.begin() + g.nc);
      nc += g.nc;
    });
    if (n_groups == 1) h->gathered.swap(parts[0]);
    else {
      d_all = nullptr;   // several device buffers: only the merged host copy is handed out
      if (want_host) {
        // merged view for the caller: per rank [all groups' bitmap rows | all groups' counts], same stride; host copy only
        const int world = dev_comm_world(e->comm);
        const uint32_t stride = shard0.stride_tiles;
        const uint64_t merged_slot = (((uint64_t)nc * stride * 8 + (uint64_t)nc * 4) + 15) & ~(uint64_t)15;
        h->gathered.assign((size_t)world * merged_slot / 8, 0);
        for (int r = 0; r < world; r++) {
          uint8_t* dst = reinterpret_cast<uint8_t*>(h->gathered.data()) + (size_t)r * merged_slot;
          each_group(e, t, [&](const GroupAt& g) {
            const uint8_t* src = reinterpret_cast<const uint8_t*>(parts[g.g].data()) + (size_t)r * g.side.shard.slot_bytes;
            memcpy(dst + (size_t)g.row0 * stride * 8, src, (size_t)g.nc * stride * 8);
            memcpy(dst + (size_t)nc * stride * 8 + (size_t)g.row0 * 4, src + (size_t)g.nc * stride * 8, (size_t)g.nc * 4);
          });
        }
        h->merged_slot = merged_slot;
      }
    }
    h->ids = all_ids(e);
    h->shard_reviews = shard0.shard_reviews;
    gk_shard_out& p = h->pub;
    memset(&p, 0, sizeof p);
    p.world = (uint32_t)dev_comm_world(e->comm); p.rank = (uint32_t)dev_comm_rank(e->comm);
    p.n_constraints = nc; p.stride_tiles = shard0.stride_tiles; p.slot_bytes = n_groups == 1 ? shard0.slot_bytes : h->merged_slot;
    p.constraint_ids = h->ids.data(); p.shard_reviews = h->shard_reviews.data(); p.totals = h->totals.data();
    p.gathered = h->gathered.empty() ? nullptr : h->gathered.data();
    p.d_gathered = d_all;
    p.kernel_ms = eo.kernel_ms; p.fast_kernel_ms = eo.fast_kernel_ms; p.n_overflow = eo.n_overflow;
    p.err_totals = h->err_totals.data(); p.beyond_limits = beyond; p.not_evaluated = not_eval;
    // the exchange step's own figures: time and bytes of every group (a collected enqueue-only pass was not timed), overlap as the primary group says
    each_group(e, t, [&](const GroupAt& g) {
      const ShardExchangeStats xs = dev_shard_exchange_stats(g.side.dev, e->comm);
      if (!collected) p.exchange_ms += xs.exchange_ms;
      p.exchange_bytes_inbound += xs.inbound_bytes;
      if (g.g == 0) p.exchange_overlapped = xs.overlap ? 1u : 0u;
    });
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const Unsupported& ex) { return fail(GK_ERR_UNSUPPORTED, ex.what());
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_shard_free(gk_shard_out* o) { if (o) delete reinterpret_cast<ShardHolder*>(o); }

// ------------------------------------------------------------------------------------------------ resident set (row f2)
namespace {

struct SweepHolder {
  gk_sweep_out pub;   // first member
  std::vector<uint32_t> ids;
  std::vector<uint64_t> results, pairs;
};

const gk_engine::ResObj* resident_namespace_of(const gk_engine::Resident& R, const gk_engine::ResObj& o) {
  if (o.ns.empty()) return nullptr;
  auto it = R.by_key.find("cluster/v1/Namespace/" + o.ns + "/");
  if (it == R.by_key.end() || !R.objs[it->second].alive) return nullptr;
  return &R.objs[it->second];
}

// the review pkg/audit builds for a cached object (auditFromCache, pkg/audit/manager.go:591-642): AugmentedUnstructured
// {Object, Namespace: the cached Namespace it lives in}, no Source, and the same Namespace as the namespaceObject option
gk_review_in resident_review_in(const gk_engine::Resident& R, const gk_engine::ResObj& o) {
  gk_review_in in;
  memset(&in, 0, sizeof in);
  in.kind = GK_REVIEW_OBJECT;
  in.source = GK_SRC_EMPTY;
  in.json = o.json.data(); in.json_len = o.json.size();
  if (const gk_engine::ResObj* ns = resident_namespace_of(R, o)) {
    in.namespace_json = ns->json.data(); in.namespace_len = ns->json.size();
    in.ns_object_json = ns->json.data(); in.ns_object_len = ns->json.size();
  }
  return in;
}

void resident_drop_chunk(gk_engine::ResChunk& c) {
  if (c.ev) gk_eval_free(c.ev);
  if (c.table) gk_table_free(c.table);
  c.ev = nullptr; c.table = nullptr;
}

}  // namespace

// What gk_resident_sweep and gk_resident_audit share (R.mu held by the caller): flatten what changed since the last sweep into a new
// chunk (everything again when the set is compacted), evaluate the chunks whose bitmaps are stale, refresh the shown masks, and list
// the constraint ids of the bitmap rows.  *t1: when flattening was done (sync_s / eval_s of gk_sweep_out).
static int resident_update(gk_engine* e, uint64_t* flattened_out, std::chrono::steady_clock::time_point* t1_out, std::vector<uint32_t>* ids) {
  gk_engine::Resident& R = e->resident;
  ensure_plan(e);
  uint64_t flattened = 0;
  // compaction: when masked-out slots outnumber the live ones (or the chunks have piled up) everything is flattened
  // again into one chunk
  bool stale_rows = false;   // a constraint with dictionary predicates arrived: every chunk lacks its <leaf>.$d rows
  for (auto& c : R.chunks) stale_rows = stale_rows || table_stale(e, c.table);
  if (stale_rows || R.n_dead_slots > R.n_live + 1024 || R.chunks.size() > 16) {
    for (auto& c : R.chunks) resident_drop_chunk(c);
    R.chunks.clear();
    R.pending.clear();
    R.n_dead_slots = 0;
    R.compactions++;
    for (uint32_t id = 0; id < R.objs.size(); id++) if (R.objs[id].alive) { R.objs[id].chunk = UINT32_MAX; R.pending.push_back(id); }
  }
  if (!R.pending.empty()) {
    std::vector<gk_review_in> ins;
    gk_engine::ResChunk c;
    for (uint32_t id : R.pending) {
      if (!R.objs[id].alive) continue;
      ins.push_back(resident_review_in(R, R.objs[id]));
      c.obj_of_slot.push_back(id);
    }
    R.pending.clear();
    if (!ins.empty()) {
      std::vector<int32_t> st(ins.size(), GK_OK);
      int rc = gk_table_create(e, ins.data(), ins.size(), GK_TABLE_RESIDENT | GK_TABLE_PRUNED, st.data(), &c.table);   // (stale chunks are flattened again: stale_rows above)
      if (rc != GK_OK) return rc;
      c.live.assign((ins.size() + 63) / 64, 0);
      for (size_t k = 0; k < ins.size(); k++) {
        gk_engine::ResObj& o = R.objs[c.obj_of_slot[k]];
        o.chunk = (uint32_t)R.chunks.size(); o.slot = (uint32_t)k;
        if (st[k] == GK_OK) { c.live[k / 64] |= 1ull << (k % 64); c.n_live++; }
      }
      flattened = ins.size();
      R.flattened_total += flattened;
      R.chunks.push_back(std::move(c));
    }
  }
  *flattened_out = flattened;
  *t1_out = std::chrono::steady_clock::now();
  ensure_plan(e);   // flattening may have interned new key paths: the plan is re-bound to the dictionary first
  uint64_t gen;
  { std::shared_lock<std::shared_mutex> l(e->plan_rw); gen = e->plan_gen; }
  for (auto& c : R.chunks) {
    if (c.ev && c.plan_gen == gen) continue;   // bitmaps still valid: same rows, same policies
    if (c.ev) { gk_eval_free(c.ev); c.ev = nullptr; }
    int rc = gk_table_eval(e, c.table, 0, &c.ev);
    if (rc != GK_OK) return rc;
    c.plan_gen = gen;
  }
  {   // audit-process excluder over the resident objects (manager.go:599): a mask beside `live`, refreshed when the Config changes
    std::shared_lock<std::shared_mutex> l(e->mu);
    auto ex = e->excluder.find("audit");
    for (auto& c : R.chunks) {
      if (c.excl_gen == e->excluder_gen && c.shown.size() == c.live.size()) {
        bool died = false;   // a slot was replaced or removed since the last sweep
        for (size_t w = 0; w < c.live.size(); w++) { died = died || (c.shown[w] & ~c.live[w]); c.shown[w] &= c.live[w]; }
        if (died) c.shown_gen++;
        continue;
      }
      c.shown = c.live;
      c.shown_gen++;
      if (ex != e->excluder.end() && !ex->second.empty())
        for (size_t k = 0; k < c.obj_of_slot.size(); k++) {
          const gk_engine::ResObj& o = R.objs[c.obj_of_slot[k]];
          if (excluder_matches(ex->second, o.is_namespace ? o.path.back() : o.ns)) c.shown[k / 64] &= ~(1ull << (k % 64));
        }
      c.excl_gen = e->excluder_gen;
    }
  }
  // the constraint ids of the bitmap rows
  if (!R.chunks.empty()) {
    const gk_eval_out* ev0 = R.chunks[0].ev;
    ids->assign(ev0->constraint_ids, ev0->constraint_ids + ev0->n_constraints);
  } else {
    { std::lock_guard<std::mutex> gate(e->plan_gate); }   // (a plan change that is waiting goes first)
    std::shared_lock<std::shared_mutex> l(e->plan_rw);
    *ids = all_ids(e);
  }
  return GK_OK;
}

// shown reviews of a chunk that its evaluation left beyond the device's limits
static uint64_t shown_beyond(const gk_engine::ResChunk& c) {
  uint64_t n = 0;
  for (uint32_t w = 0; w < c.ev->n_tiles && w < c.shown.size(); w++) n += (uint64_t)__builtin_popcountll(c.ev->too_big[w] & c.shown[w]);
  return n;
}

// a resident object's inventory path as a JSON array, appended to `out`
static void append_path_json(const std::vector<std::string>& path, std::string& out) {
  out += '[';
  bool first = true;
  for (const std::string& seg : path) { if (!first) out += ','; first = false; json_escape(seg, out); }
  out += ']';
}

// results, not pairs (pkg/audit/manager.go:902), over the shown slots of all chunks (R.mu held by the caller)
static void resident_result_totals(gk_engine* e, const std::vector<uint32_t>& ids, std::vector<uint64_t>* results) {
  gk_engine::Resident& R = e->resident;
  const uint32_t nc = (uint32_t)ids.size();
  // as gk_table_totals: the device says which violating live pairs can have more than one result; the others count one
  std::shared_lock<std::shared_mutex> pl(e->plan_rw);
  std::shared_lock<std::shared_mutex> l(e->mu);
  for (auto& c : R.chunks) {
    const gk_eval_out* ev = c.ev;
    const uint32_t nt = ev->n_tiles, ncc = std::min<uint32_t>(ev->n_constraints, nc);
    std::vector<uint64_t> shown_viol((size_t)nc * nt, 0);
    for (uint32_t row = 0; row < ncc; row++)
      for (uint32_t w = 0; w < nt; w++) shown_viol[(size_t)row * nt + w] = ev->viol[(size_t)row * nt + w] & c.shown[w];
    std::vector<uint8_t> counted;
    std::vector<uint64_t> counted_sum;
    const std::vector<uint64_t> need = render_needed(e, c.table, ids, nt, shown_viol, &counted, &counted_sum);
    for (uint32_t row = 0; row < ncc; row++) {
      if (counted[row]) { (*results)[row] += counted_sum[row]; continue; }   // (round 4: counted on the device)
      for (uint32_t w = 0; w < nt; w++) (*results)[row] += (uint64_t)__builtin_popcountll(shown_viol[(size_t)row * nt + w] & ~need[(size_t)row * nt + w]);
    }
    for (uint32_t slot = 0; slot < c.obj_of_slot.size(); slot++) {
      const uint64_t bit = 1ull << (slot % 64);
      bool any = false;
      for (uint32_t row = 0; row < ncc && !any; row++) any = (need[(size_t)row * nt + slot / 64] & bit) != 0;
      if (!any) continue;
      const gk_review_in in = resident_review_in(R, R.objs[c.obj_of_slot[slot]]);
      ReviewDoc doc = normalize_object(parse_json(in.json, in.json_len), parse_opt(in.namespace_json, in.namespace_len),
                                       parse_opt(in.ns_object_json, in.ns_object_len), in.source, "", e->ns_cache);
      for (uint32_t row = 0; row < ncc; row++) {
        if (!(need[(size_t)row * nt + slot / 64] & bit)) continue;
        const ConstraintRec& k = e->constraints[ids[row]];
        auto it = e->templates.find(lower_str(k.kind));
        if (it != e->templates.end()) (*results)[row] += it->second->render(doc.request, k.params, e->inventory).size();
      }
    }
  }
}

int gk_resident_sweep(gk_engine* e, uint32_t flags, gk_sweep_out** out) {
  if (!e || !out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    gk_engine::Resident& R = e->resident;
    std::lock_guard<std::mutex> rl(R.mu);
    const auto t0 = std::chrono::steady_clock::now();
    auto t1 = t0;
    uint64_t flattened = 0;
    std::unique_ptr<SweepHolder> h(new SweepHolder());
    int rc = resident_update(e, &flattened, &t1, &h->ids);
    if (rc != GK_OK) return rc;
    // per-constraint totals over the live, not excluded slots of all chunks
    const uint32_t nc = (uint32_t)h->ids.size();
    h->pairs.assign(nc, 0); h->results.assign(nc, 0);
    uint64_t beyond = 0;
    for (auto& c : R.chunks) {
      const gk_eval_out* ev = c.ev;
      for (uint32_t row = 0; row < ev->n_constraints && row < nc; row++)
        for (uint32_t w = 0; w < ev->n_tiles; w++) h->pairs[row] += (uint64_t)__builtin_popcountll(ev->viol[(size_t)row * ev->n_tiles + w] & c.shown[w]);
      beyond += shown_beyond(c);
    }
    if (flags & GK_SWEEP_RESULT_TOTALS) resident_result_totals(e, h->ids, &h->results);
    R.swept = true;
    gk_sweep_out& p = h->pub;
    memset(&p, 0, sizeof p);
    p.n_objects = R.n_live; p.n_constraints = nc; p.constraint_ids = h->ids.data();
    p.pairs = h->pairs.data(); p.results = (flags & GK_SWEEP_RESULT_TOTALS) ? h->results.data() : nullptr;
    p.n_chunks = (uint32_t)R.chunks.size(); p.flattened = flattened; p.beyond_limits = beyond;
    p.sync_s = std::chrono::duration<double>(t1 - t0).count();
    p.eval_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_sweep_free(gk_sweep_out* o) { if (o) delete reinterpret_cast<SweepHolder*>(o); }

namespace {
struct AuditHolder {
  gk_audit_out pub;   // first member
  std::vector<uint32_t> ids, counts, objects, overflow;
  std::vector<uint64_t> pairs, results, err_pairs;
  std::vector<std::string> path_text;
  std::vector<const char*> paths;
};
}  // namespace

// What an audit run writes into a constraint's status, for the resident set (pkg/audit/manager.go:885-941 over auditFromCache's
// objects): per chunk the device counts the shown violators of every bitmap row and picks the k with the smallest object key plus the
// key ties of the k-th (dev_audit_select); the chunks' candidates are merged here (audit_merge.hpp) and only they are named to the caller.
int gk_resident_audit(gk_engine* e, uint32_t k, uint32_t flags, gk_audit_out** out) {
  if (!e || !out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    gk_engine::Resident& R = e->resident;
    std::lock_guard<std::mutex> rl(R.mu);
    std::unique_ptr<AuditHolder> h(new AuditHolder());
    uint64_t flattened = 0;
    auto t1 = std::chrono::steady_clock::now();
    int rc = resident_update(e, &flattened, &t1, &h->ids);
    if (rc != GK_OK) return rc;
    const uint32_t nc = (uint32_t)h->ids.size();
    const uint32_t stride = (uint32_t)std::min<uint64_t>(k, R.n_live) + 64;   // (k beyond the set's size selects everything)
    h->pairs.assign(nc, 0); h->results.assign(nc, 0); h->err_pairs.assign(nc, 0); h->counts.assign(nc, 0); h->overflow.assign(nc, 0);
    h->objects.assign((size_t)nc * stride, 0xFFFFFFFFu);
    std::vector<std::vector<AuditCand>> cands(nc);
    uint64_t beyond = 0;
    for (auto& c : R.chunks) {
      gk_table* t = c.table;
      const gk_eval_out* ev = c.ev;
      beyond += shown_beyond(c);
      table_key_order(t);
      const uint32_t kc = std::min(k, t->n_reviews), cap = kc + 64;
      std::vector<uint32_t> pairs, idx, cnt, ovf;
      {
        std::shared_lock<std::shared_mutex> l(e->plan_rw);
        if (e->plan_dirty || c.plan_gen != e->plan_gen) return fail(GK_ERR_DEVICE, "the policies changed while gk_resident_audit ran: call it again");
        each_group(e, t, [&](const GroupAt& g) {   // the groups' rows, appended
          std::vector<uint32_t> p, r, n, o;
          dev_audit_select(g.side.dev, g.nc, t->n_reviews, t->order, t->grp, c.shown, c.shown_gen, kc, cap, &p, &r, &n, &o);
          append(pairs, std::move(p)); append(idx, std::move(r)); append(cnt, std::move(n)); append(ovf, std::move(o));
        });
      }
      const uint32_t rows = std::min<uint32_t>((uint32_t)pairs.size(), nc);
      for (uint32_t row = 0; row < rows; row++) {
        h->pairs[row] += pairs[row];
        if (ovf[row]) h->overflow[row] = 1;
        for (uint32_t i = 0; i < cnt[row]; i++) {
          const uint32_t slot = idx[(size_t)row * cap + i];
          if (slot < c.obj_of_slot.size()) cands[row].push_back(AuditCand{t->obj_key(slot), c.obj_of_slot[slot]});
        }
      }
      // (violating pairs the host evaluation of over-limit reviews added are no part of the device bitmaps -- the kernels never set a
      //  refused review's bit: where their slot is shown they join the candidates and the pairs, as in gk_table_topk)
      std::vector<std::pair<uint32_t, uint32_t>> hv;
      { std::lock_guard<std::mutex> hl(t->host_mu); if (t->host_ids == h->ids) hv = t->host_viol; }
      for (auto& hp : hv) {
        const uint32_t row = hp.first, slot = hp.second;
        if (row >= rows || slot >= c.obj_of_slot.size() || !(c.shown[slot / 64] & (1ull << (slot % 64)))) continue;
        h->pairs[row]++;
        cands[row].push_back(AuditCand{t->obj_key(slot), c.obj_of_slot[slot]});
      }
      // Autoreject pairs (Matcher.Match returned an error: one Result each, which the audit counts and lists like any other) are rare and
      // their bitmap is on the host already.  Counted once per (evaluation, mask); the rows that have any are then walked in key order
      // until each has its k and their ties, or all it has -- once per (evaluation, mask, k) as well: where the first of them sits far
      // down the key order the walk costs more than the two kernels (profiles/resident_audit.md).
      if (c.err_shown_gen != c.shown_gen || c.err_plan_gen != c.plan_gen || c.err_pairs.size() != rows) {
        c.err_pairs.assign(rows, 0);
        for (uint32_t row = 0; row < rows; row++)
          for (uint32_t w = 0; w < ev->n_tiles; w++) c.err_pairs[row] += (uint64_t)__builtin_popcountll(ev->err[(size_t)row * ev->n_tiles + w] & c.shown[w]);
        c.err_shown_gen = c.shown_gen; c.err_plan_gen = c.plan_gen;
        c.err_slots.clear();
      }
      if (c.err_slots.size() != rows || c.err_k != kc) {
        c.err_slots.assign(rows, std::vector<uint32_t>());
        c.err_k = kc;
        struct ErrRow { uint32_t row; uint64_t left; uint32_t found = 0, grp_k = 0; };
        std::vector<ErrRow> open;
        for (uint32_t row = 0; row < rows; row++) if (kc && c.err_pairs[row]) open.push_back(ErrRow{row, c.err_pairs[row]});
        for (uint32_t p = 0; p < t->n_reviews && !open.empty(); p++) {
          const uint32_t slot = t->order[p];
          if (!(c.shown[slot / 64] & (1ull << (slot % 64)))) continue;
          for (size_t i = 0; i < open.size();) {
            ErrRow& r = open[i];
            bool close = false;
            if ((ev->err[(size_t)r.row * ev->n_tiles + slot / 64] >> (slot % 64)) & 1ull) {
              if (r.found >= kc && t->grp[p] != r.grp_k) close = true;
              else {
                if (r.found == kc - 1) r.grp_k = t->grp[p];
                c.err_slots[r.row].push_back(slot);
                r.found++;
                close = --r.left == 0;
              }
            }
            if (close) { open[i] = open.back(); open.pop_back(); } else i++;
          }
        }
      }
      for (uint32_t row = 0; row < rows; row++) {
        h->err_pairs[row] += c.err_pairs[row];
        for (uint32_t slot : c.err_slots[row]) cands[row].push_back(AuditCand{t->obj_key(slot), c.obj_of_slot[slot]});
      }
    }
    std::unordered_map<uint32_t, uint32_t> path_of;   // resident object -> index into paths
    for (uint32_t row = 0; row < nc; row++) {
      if (!audit_merge(&cands[row], k, stride)) h->overflow[row] = 1;
      h->counts[row] = (uint32_t)cands[row].size();
      for (size_t i = 0; i < cands[row].size(); i++) {
        auto ins = path_of.emplace(cands[row][i].obj, (uint32_t)h->path_text.size());
        if (ins.second) { h->path_text.emplace_back(); append_path_json(R.objs[cands[row][i].obj].path, h->path_text.back()); }
        h->objects[(size_t)row * stride + i] = ins.first->second;
      }
    }
    for (const std::string& p : h->path_text) h->paths.push_back(p.c_str());
    if (flags & GK_SWEEP_RESULT_TOTALS) resident_result_totals(e, h->ids, &h->results);
    R.swept = true;
    gk_audit_out& p = h->pub;
    memset(&p, 0, sizeof p);
    p.n_objects = R.n_live; p.n_constraints = nc; p.stride = stride; p.n_chunks = (uint32_t)R.chunks.size();
    p.constraint_ids = h->ids.data(); p.pairs = h->pairs.data(); p.results = (flags & GK_SWEEP_RESULT_TOTALS) ? h->results.data() : nullptr;
    p.counts = h->counts.data(); p.objects = h->objects.data(); p.overflow = h->overflow.data();
    p.n_paths = (uint32_t)h->paths.size(); p.paths = h->paths.empty() ? nullptr : h->paths.data();
    p.beyond_limits = beyond;
    p.err_pairs = h->err_pairs.data();
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_audit_free(gk_audit_out* o) { if (o) delete reinterpret_cast<AuditHolder*>(o); }

// ---- the plan-specialised kernel checked against the bytecode kernel (gk_table_verify, gk_resident_verify)
namespace {
struct VerifyHolder {
  gk_verify_out pub;   // first member
  std::vector<uint32_t> ids;
  VerifyMerge m;
  std::vector<gk_verify_entry> entries;
  std::vector<std::string> path_text;
  std::vector<char*> paths;
  // over all tables verified by the call
  uint32_t n_reviews = 0, n_plan_groups = 0, specialised_groups = 0, quarantined_groups = 0;
  uint64_t hash = 0;
  float a_ms = 0, b_ms = 0;
};
}  // namespace

// One table: every plan group on the specialised path (into the table's own buffers, as gk_table_eval), again with the bytecode kernel
// into the verification views, the comparison per group on the device, the groups merged into h->m.  `mask`: the reviews to compare
// (nullptr: all); review_base: what the table's reviews are shifted by in the merged answer (chunks of the resident set).  The first
// table of a call fixes the constraint ids of the rows; a later one that sees other ids fails (the policies changed in between).
static int verify_table(gk_engine* e, gk_table* t, uint32_t flags, uint32_t max_entries, const std::vector<uint64_t>* mask, uint32_t review_base, bool first, VerifyHolder* h) {
  ensure_plan(e);
  if (const char* why = table_stale(e, t)) return fail(GK_ERR_INVALID, why);
  if (!t->sides[0].shard.shard_reviews.empty())
    return fail(GK_ERR_INVALID, "gk_table_verify: the table is set up as a shard (gk_table_sweep_sharded), its bitmaps live in the exchange buffer: verify a table of its own");
  const bool want_match = (flags & GK_VERIFY_WANT_MATCH) != 0;
  std::vector<size_t> differing;   // plan groups
  uint64_t gen = 0;
  {
    { std::lock_guard<std::mutex> gate(e->plan_gate); }   // (a plan change that is waiting goes first)
    std::shared_lock<std::shared_mutex> l(e->plan_rw);
    gen = e->plan_gen;
    const std::vector<uint32_t> ids = all_ids(e);
    if (first) { h->ids = ids; h->m.begin((uint32_t)ids.size(), want_match); }
    else if (ids != h->ids) return fail(GK_ERR_DEVICE, "the policies changed while the verification ran: call it again");
    const size_t ng = e->groups.size();
    table_plans(e, t);
    // the bytecode side of every group: a view of the table, and the plan it evaluates -- the group's own plan under EvalOptions::bytecode,
    // or the backend's twin of it (kept while the plan generation stands)
    each_group(e, t, [&](const GroupAt& g) {
      gk_table::Side& s = g.side;
      if (!s.vview) s.vview = dev_table_view(t->dev);
      if (s.vtwin_gen != gen) { dev_plan_free(s.vtwin); s.vtwin = dev_verify_twin(e->opts.device, *s.host, g.grp.big); s.vtwin_gen = gen; }
    });
    EvalOptions oa;
    oa.download = false;
    oa.want_match = want_match;
    oa.jit_wait = true;   // whatever the table's size: the bytecode kernel is not compared with itself
    EvalOptions ob = oa;
    ob.bytecode = true;
    if (ng > 1) each_group(e, t, [&](const GroupAt& g) { dev_jit_prefetch(g.side.plan, g.side.dev); });   // (the builds compile side by side)
    std::vector<EvalOut> A(ng), B(ng);
    table_results_move(t);
    each_group(e, t, [&](const GroupAt& g) { dev_verify_eval(g.side.plan, g.side.dev, oa, &A[g.g]); dev_tviol_note(g.side.dev, A[g.g]); dev_tchg_note(g.side.dev, A[g.g]); });
    each_group(e, t, [&](const GroupAt& g) { dev_verify_eval(g.side.vtwin ? g.side.vtwin : g.side.plan, g.side.vview, ob, &B[g.g]); });
    t->last_nc = (uint32_t)ids.size(); t->last_ids = ids;   // (the table's bitmaps are this evaluation's now, as after gk_table_eval)
    t->ts_pending = false; t->eval_plan_gen = gen;
    // fault injection (gk_debug_set "verify_flip"): one bit or word of the bytecode side
    const int64_t flip = g_debug_verify_flip.load();
    const uint32_t f_kind = (uint32_t)((uint64_t)flip >> 56) & 0x7Fu, f_row = (uint32_t)((uint64_t)flip >> 32) & 0x7FFFFFu, f_review = (uint32_t)((uint64_t)flip & 0xFFFFFFFFu);
    const bool f_word = (((uint64_t)flip >> 55) & 1u) != 0, f_here = flip >= 0 && f_review >= review_base && f_review - review_base < t->n_reviews;
    uint32_t row_base = 0;
    each_group(e, t, [&](const GroupAt& g) {
      const EvalOut& a = A[g.g];
      const uint32_t nc = a.n_constraints;
      h->n_plan_groups++;
      h->a_ms += a.kernel_ms; h->b_ms += B[g.g].kernel_ms;
      h->hash = h->n_plan_groups == 1 ? a.kernel_hash : h->hash * 1099511628211ull ^ a.kernel_hash;   // (as gk_eval_out: one figure that names all the texts)
      if (f_here && nc && t->n_reviews && (f_kind == VERIFY_TOO_BIG ? g.g == 0 : f_row >= row_base && f_row - row_base < nc))
        dev_verify_flip(g.side.vview, nc, f_kind, f_kind == VERIFY_TOO_BIG ? 0 : f_row - row_base, f_review - review_base, f_word);
      // (else: no specialised build for this group -- GK_NO_JIT, a failed build, a quarantined group, whatever a backend that cannot take
      //  a plan off its specialised code goes on running for it: nothing to compare)
      if (a.specialised && !e->quarantined.count(g.g)) {
        h->specialised_groups++;
        VerifyDiff d;
        dev_verify_diff(g.side.dev, g.side.vview, nc, t->n_reviews, want_match, mask, max_entries, &d);
        h->m.add(d, row_base, review_base);
        if (d.entries_total != 0 && (flags & GK_VERIFY_QUARANTINE)) differing.push_back(g.g);
      }
      row_base += nc;
    });
    h->n_reviews += t->n_reviews;
  }
  if (!differing.empty()) {
    // nobody evaluates while a plan changes hands: the tables' cached launch state is keyed by what dev_plan_no_jit replaces
    std::lock_guard<std::mutex> gate(e->plan_gate);
    std::unique_lock<std::shared_mutex> l(e->plan_rw);
    if (e->plan_gen == gen)   // (else the plans were replaced in between: verify again)
      for (size_t g : differing) {
        // the plan that ran -- the table-sized variant of a resident table -- and every other plan of the group: same formulas, same generator
        e->quarantined.insert(g);
        dev_plan_no_jit(e->groups[g]->dev);
        for (auto& v : e->variants) if (v.first.first == g && v.second->dev) dev_plan_no_jit(v.second->dev);
        h->quarantined_groups++;
        fprintf(stderr, "[gkgpu] the plan-specialised kernel disagrees with the bytecode kernel (gk_table_verify), using the bytecode kernel for this plan\n");
      }
  }
  return GK_OK;
}

static void verify_publish(VerifyHolder* h, uint32_t flags, uint32_t max_entries) {
  h->m.finish(max_entries);
  for (const VerifyEntry& en : h->m.entries) h->entries.push_back(gk_verify_entry{en.kind, en.row, en.review, en.a_bit});
  gk_verify_out& p = h->pub;
  memset(&p, 0, sizeof p);
  p.n_reviews = h->n_reviews; p.n_constraints = (uint32_t)h->ids.size(); p.n_plan_groups = h->n_plan_groups;
  p.constraint_ids = h->ids.data();
  p.specialised_groups = h->specialised_groups;
  p.kernel_text_hash = h->hash;
  p.diff_viol = h->m.diff[0].data(); p.diff_err = h->m.diff[1].data();
  p.diff_match = (flags & GK_VERIFY_WANT_MATCH) ? h->m.diff[2].data() : nullptr;
  p.diff_too_big = h->m.diff_too_big; p.diff_total = h->m.diff_total();
  p.n_entries = (uint32_t)h->entries.size(); p.entries_total = h->m.entries_total;
  p.entries = h->entries.empty() ? nullptr : h->entries.data();
  p.quarantined_groups = h->quarantined_groups;
  p.specialised_ms = h->a_ms; p.bytecode_ms = h->b_ms; p.diff_ms = h->m.ms;
}

int gk_table_verify(gk_engine* e, gk_table* t, uint32_t flags, uint32_t max_entries, gk_verify_out** out) {
  if (!e || !t || !out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    std::unique_ptr<VerifyHolder> h(new VerifyHolder());
    int rc = verify_table(e, t, flags, max_entries, nullptr, 0, true, h.get());
    if (rc != GK_OK) return rc;
    verify_publish(h.get(), flags, max_entries);
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const Unsupported& ex) { return fail(GK_ERR_UNSUPPORTED, ex.what());
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_verify_free(gk_verify_out* o) { if (o) delete reinterpret_cast<VerifyHolder*>(o); }

int gk_resident_verify(gk_engine* e, uint32_t flags, uint32_t max_entries, gk_verify_out** out, char*** entry_paths) {
  if (!e || !out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    gk_engine::Resident& R = e->resident;
    std::lock_guard<std::mutex> rl(R.mu);
    std::unique_ptr<VerifyHolder> h(new VerifyHolder());
    uint64_t flattened = 0;
    auto t1 = std::chrono::steady_clock::now();
    std::vector<uint32_t> ids;
    int rc = resident_update(e, &flattened, &t1, &ids);
    if (rc != GK_OK) return rc;
    R.swept = true;
    h->ids = ids;
    h->m.begin((uint32_t)ids.size(), (flags & GK_VERIFY_WANT_MATCH) != 0);
    std::vector<uint32_t> base;   // first merged review of every chunk
    uint32_t at = 0;
    for (auto& c : R.chunks) {
      base.push_back(at);
      rc = verify_table(e, c.table, flags, max_entries, &c.live, at, false, h.get());   // (dead slots are not compared)
      if (rc != GK_OK) return rc;
      at += c.table->n_reviews;
    }
    verify_publish(h.get(), flags, max_entries);
    for (const gk_verify_entry& en : h->entries) {
      size_t ci = std::upper_bound(base.begin(), base.end(), en.review) - base.begin();
      static const std::vector<std::string> no_path;
      const bool known = ci > 0 && en.review - base[ci - 1] < R.chunks[ci - 1].obj_of_slot.size();
      h->path_text.emplace_back();
      append_path_json(known ? R.objs[R.chunks[ci - 1].obj_of_slot[en.review - base[ci - 1]]].path : no_path, h->path_text.back());
    }
    for (std::string& p : h->path_text) h->paths.push_back(&p[0]);
    if (entry_paths) *entry_paths = h->paths.empty() ? nullptr : h->paths.data();
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const Unsupported& ex) { return fail(GK_ERR_UNSUPPORTED, ex.what());
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

namespace {
// the cached answer for one resident object, as gk_query's JSON; false: not resident / not swept / its slot is stale
// audit: the answer pkg/audit would get -- an object the Config excludes from the audit process is never reviewed ("[]")
bool resident_answer(gk_engine* e, uint32_t id, std::string* json, int* status, std::string* err, bool audit = false, const std::vector<uint32_t>* wanted = nullptr) {
  gk_engine::Resident& R = e->resident;
  const gk_engine::ResObj& o = R.objs[id];
  if (!R.swept || !o.alive || o.chunk == UINT32_MAX) return false;
  const gk_engine::ResChunk& c = R.chunks[o.chunk];
  if (!c.ev || !(c.live[o.slot / 64] & (1ull << (o.slot % 64)))) return false;
  if (audit) {
    { std::shared_lock<std::shared_mutex> l(e->mu); if (c.excl_gen != e->excluder_gen) return false; }   // Config changed since the sweep
    if (!(c.shown[o.slot / 64] & (1ull << (o.slot % 64)))) { *json = "[]"; *status = GK_OK; return true; }
  }
  { std::shared_lock<std::shared_mutex> l(e->plan_rw); if (e->plan_dirty || c.plan_gen != e->plan_gen) return false; }
  const gk_review_in in = resident_review_in(R, o);
  bool too_big = false;
  *json = query_results_json(e, c.table, *c.ev, o.slot, in, &too_big, wanted);
  *status = GK_OK;
  if (too_big) { *status = GK_ERR_LIMIT; *err = "review is beyond the engine's limits (more than 255 elements in an array that constraint predicates iterate, or an object where they iterate array elements)"; }
  return true;
}
}  // namespace

// ---- gk_resident_violations: every shown resident object with at least one result, in pages (viol_stream.hpp holds the pure part)
namespace {
struct ViolationsHolder {
  gk_violations_out pub;   // first member
  std::vector<uint32_t> ids;
  std::vector<uint64_t> viol, err;
  std::string path_arena;   // the page's path texts, \0 between them: one allocation (a string per entry was most of a 65 536-entry page's time)
  std::vector<std::string> result_text;
  std::vector<const char*> paths, results;
};
const char* const k_stream_moved = "the resident set or the policies changed since the stream began: start again with cursor 0";

// What both resident streams render for a page (GK_VIOLATIONS_RENDER / GK_CHANGES_RENDER): gk_resident_review's answer for the objects
// of the page entries listed in `todo` (indices into slots, ascending), on the host workers (GK_HOST_THREADS), one object per task
// handed out in page order; text is [slots].  GK_OK, or the first failure's status with its text in *error (the remaining objects are
// then not rendered).  R.mu held.
int resident_render_page(gk_engine* e, const gk_engine::ResChunk& c, const std::vector<uint32_t>& slots, const std::vector<size_t>& todo,
                         std::vector<std::string>* text, std::string* error) {
  text->resize(slots.size());
  if (todo.empty()) return GK_OK;
  size_t n_threads = std::max<size_t>(1, std::min<size_t>(host_cpus(), todo.size()));
  if (const char* ht = getenv("GK_HOST_THREADS")) n_threads = std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, atoi(ht)), todo.size()));
  std::atomic<size_t> next{0};
  std::mutex err_mu;
  int first_status = GK_OK;
  auto worker = [&](size_t) {
    for (;;) {
      const size_t k = next.fetch_add(1);
      if (k >= todo.size()) return;
      const size_t i = todo[k];
      std::string err;
      int st = GK_OK;
      try {
        if (!resident_answer(e, c.obj_of_slot[slots[i]], &(*text)[i], &st, &err, true)) { st = GK_ERR_INVALID; err = k_stream_moved; }
      } catch (const std::exception& ex) { st = GK_ERR_REGO; err = ex.what(); }
      if (st != GK_OK) {
        std::lock_guard<std::mutex> l(err_mu);
        if (first_status == GK_OK) { first_status = st; *error = err; }
        next.store(todo.size());
      }
    }
  };
  HostWorkers::get().run(n_threads, worker);
  return first_status;
}

// The index of one chunk: per plan group the device counts the shown reviews with a bit per bitmap word (dev_viol_index) and keeps the
// prefix sum that places its entries.  Where nothing else can add an entry -- one group, no autoreject bit, no host-evaluated
// violation: the common state -- those counts ARE the index and 4 bytes per word come back.  Otherwise an object may be named by
// several sources, so the groups' `any` words come back as well and are ORed here with the host's.  R.mu and plan_rw (shared) held.
void resident_viol_index(gk_engine* e, gk_engine::ResChunk& c, const std::vector<uint32_t>& ids) {
  gk_table* t = c.table;
  const gk_eval_out* ev = c.ev;
  const uint32_t pw = (t->n_reviews + 63u) / 64u, nt = ev->n_tiles, rows = std::min<uint32_t>(ev->n_constraints, (uint32_t)ids.size());
  std::vector<uint64_t> host_words(pw, 0);
  for (uint32_t row = 0; row < rows; row++)
    for (uint32_t w = 0; w < pw && w < nt; w++) host_words[w] |= ev->err[(size_t)row * nt + w];
  {
    std::lock_guard<std::mutex> hl(t->host_mu);
    if (t->host_ids == ids)
      for (auto& hp : t->host_viol) if (hp.first < rows && hp.second < t->n_reviews) host_words[hp.second / 64] |= 1ull << (hp.second % 64);
  }
  bool has_host = false;
  for (uint32_t w = 0; w < pw; w++) { host_words[w] &= w < c.shown.size() ? c.shown[w] : 0ull; has_host = has_host || host_words[w]; }
  const bool merged = has_host || (e->groups.size() > 1 && t->sides.size() > 1);
  std::vector<uint64_t> any(pw, 0), a;
  std::vector<uint32_t> cnt(pw, 0), n;
  each_group(e, t, [&](const GroupAt& g) {
    if (g.nc == 0) return;
    dev_viol_index(g.side.dev, g.nc, t->n_reviews, c.shown, c.shown_gen, &n, merged ? &a : nullptr);
    if (n.size() != pw || (merged && a.size() != pw)) throw std::runtime_error("dev_viol_index: wrong size");
    if (merged) for (uint32_t w = 0; w < pw; w++) any[w] |= a[w];
    else cnt = n;
  });
  c.vs_prefix.assign((size_t)pw + 1, 0);
  for (uint32_t w = 0; w < pw; w++) c.vs_prefix[w + 1] = c.vs_prefix[w] + (merged ? (uint64_t)__builtin_popcountll(any[w] | host_words[w]) : cnt[w]);
  c.vs_host_slots.clear();
  for (uint32_t w = 0; w < pw; w++)
    for (uint64_t m = host_words[w]; m; m &= m - 1) c.vs_host_slots.push_back(w * 64u + (uint32_t)__builtin_ctzll(m));
  c.vs_plan_gen = c.plan_gen; c.vs_shown_gen = c.shown_gen;
}
}  // namespace

int gk_resident_violations(gk_engine* e, uint64_t cursor, uint32_t max_objects, uint32_t flags, gk_violations_out** out) {
  if (!e || !out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    gk_engine::Resident& R = e->resident;
    std::lock_guard<std::mutex> rl(R.mu);
    std::unique_ptr<ViolationsHolder> h(new ViolationsHolder());
    if (cursor == 0) {   // a stream begins: the set is brought up to date as by gk_resident_sweep
      uint64_t flattened = 0;
      auto t1 = std::chrono::steady_clock::now();
      int rc = resident_update(e, &flattened, &t1, &h->ids);
      if (rc != GK_OK) return rc;
      R.swept = true;
    } else {
      // nothing is flattened or evaluated for a later page: whatever the answer depends on must stand as the stream's first call left it
      if (!R.swept || R.vs_gen == 0 || R.set_gen != R.vs_set_gen || R.compactions != R.vs_compactions) return fail(GK_ERR_INVALID, k_stream_moved);
      { std::shared_lock<std::shared_mutex> l(e->mu); if (e->excluder_gen != R.vs_excl_gen) return fail(GK_ERR_INVALID, k_stream_moved); }
      if (!R.chunks.empty()) h->ids.assign(R.chunks[0].ev->constraint_ids, R.chunks[0].ev->constraint_ids + R.chunks[0].ev->n_constraints);
    }
    const uint32_t nc = (uint32_t)h->ids.size(), mw = (nc + 63u) / 64u;
    uint64_t beyond = 0, total = 0;
    std::vector<uint32_t> slots;
    uint32_t page_chunk = 0;
    uint64_t next_cursor = 0;
    {
      std::shared_lock<std::shared_mutex> pl(e->plan_rw);
      if (cursor == 0) {
        for (auto& c : R.chunks) {
          if (e->plan_dirty || c.plan_gen != e->plan_gen) return fail(GK_ERR_DEVICE, "the policies changed while gk_resident_violations ran: call it again");
          if (c.vs_prefix.empty() || c.vs_plan_gen != c.plan_gen || c.vs_shown_gen != c.shown_gen) resident_viol_index(e, c, h->ids);
        }
        const uint64_t plan_gen = e->plan_gen, excl_gen = R.chunks.empty() ? 0 : R.chunks[0].excl_gen;
        if (R.vs_gen == 0 || R.vs_set_gen != R.set_gen || R.vs_compactions != R.compactions || R.vs_plan_gen != plan_gen || R.vs_excl_gen != excl_gen) {
          R.vs_gen = viol_next_gen(R.vs_gen);
          R.vs_set_gen = R.set_gen; R.vs_compactions = R.compactions; R.vs_plan_gen = plan_gen; R.vs_excl_gen = excl_gen;
        }
      } else {
        if (e->plan_dirty || e->plan_gen != R.vs_plan_gen) return fail(GK_ERR_INVALID, k_stream_moved);
        for (auto& c : R.chunks)
          if (!c.ev || c.plan_gen != e->plan_gen || c.vs_prefix.empty() || c.vs_plan_gen != c.plan_gen || c.vs_shown_gen != c.shown_gen || c.excl_gen != R.vs_excl_gen)
            return fail(GK_ERR_INVALID, k_stream_moved);
      }
      std::vector<uint32_t> chunk_words;
      for (auto& c : R.chunks) {
        chunk_words.push_back((uint32_t)(c.vs_prefix.size() - 1));
        total += c.vs_prefix.back();
        beyond += shown_beyond(c);
      }
      // where the page begins: the cursor's word, or the first word of the set that has entries
      ViolCursor at;
      bool have = false;
      if (cursor != 0) {
        if (!viol_cursor_check(cursor, R.vs_gen, chunk_words, &at)) return fail(GK_ERR_INVALID, k_stream_moved);
        if (viol_next_word(R.chunks[at.chunk].vs_prefix, at.word) != at.word) return fail(GK_ERR_INVALID, k_stream_moved);   // (no page begins at a word without entries)
        have = true;
      } else {
        at.gen = R.vs_gen;
        for (uint32_t ci = 0; ci < R.chunks.size() && !have; ci++) {
          const uint32_t w = viol_next_word(R.chunks[ci].vs_prefix, 0);
          if (w < chunk_words[ci]) { at.chunk = ci; at.word = w; have = true; }
        }
      }
      if (have) {
        gk_engine::ResChunk& c = R.chunks[at.chunk];
        gk_table* t = c.table;
        const gk_eval_out* ev = c.ev;
        const uint32_t w0 = at.word, w1 = viol_page_end(c.vs_prefix, w0, max_objects);
        const uint32_t nt = ev->n_tiles, rows = std::min<uint32_t>(ev->n_constraints, nc);
        page_chunk = at.chunk;
        // the device's entries of every plan group, then the slots only the host knows
        std::vector<std::vector<uint32_t>> rev(e->groups.size());
        std::vector<std::vector<uint64_t>> msk(e->groups.size());
        each_group(e, t, [&](const GroupAt& g) {
          if (g.nc == 0) return;
          dev_viol_entries(g.side.dev, g.nc, t->n_reviews, c.shown, c.shown_gen, w0, w1, &rev[g.g], &msk[g.g]);
          slots = slots.empty() ? rev[g.g] : viol_merge_slots(slots, rev[g.g]);
        });
        const auto x0 = std::lower_bound(c.vs_host_slots.begin(), c.vs_host_slots.end(), w0 * 64u);
        const auto x1 = std::lower_bound(x0, c.vs_host_slots.end(), (uint64_t)w1 * 64u, [](uint32_t s, uint64_t lim) { return s < lim; });
        const std::vector<uint32_t> host_slots(x0, x1);
        if (!host_slots.empty()) slots = viol_merge_slots(slots, host_slots);
        if (slots.size() != c.vs_prefix[w1] - c.vs_prefix[w0]) throw std::runtime_error("gk_resident_violations: the page's entries do not add up to the chunk's index");
        h->viol.assign(slots.size() * (size_t)mw, 0); h->err.assign(slots.size() * (size_t)mw, 0);
        each_group(e, t, [&](const GroupAt& g) {
          if (g.nc && !viol_scatter(slots, mw, rev[g.g], msk[g.g], g.nc, g.row0, &h->viol))
            throw std::runtime_error("gk_resident_violations: a plan group's entries do not fit the page");
        });
        for (uint32_t slot : host_slots) {   // autoreject pairs: the downloaded error bitmap
          const size_t i = viol_find(slots, slot);
          for (uint32_t row = 0; row < rows; row++)
            if ((ev->err[(size_t)row * nt + slot / 64] >> (slot % 64)) & 1ull) h->err[i * mw + row / 64] |= 1ull << (row % 64);
        }
        {   // violating pairs the host evaluation of over-limit reviews added: no part of the device bitmaps (as gk_resident_audit)
          std::lock_guard<std::mutex> hl(t->host_mu);
          if (t->host_ids == h->ids)
            for (auto& hp : t->host_viol) {
              if (hp.first >= rows || hp.second / 64 < w0 || hp.second / 64 >= w1) continue;
              const size_t i = viol_find(slots, hp.second);
              if (i < slots.size()) h->viol[i * mw + hp.first / 64] |= 1ull << (hp.first % 64);   // (not on the page: not shown)
            }
        }
        // the next page begins at the next word with entries, in this chunk or a later one
        ViolCursor nx;
        nx.gen = R.vs_gen;
        bool more = false;
        for (uint32_t ci = at.chunk; ci < R.chunks.size() && !more; ci++) {
          const uint32_t w = viol_next_word(R.chunks[ci].vs_prefix, ci == at.chunk ? w1 : 0);
          if (w < chunk_words[ci]) { nx.chunk = ci; nx.word = w; more = true; }
        }
        if (more) {
          next_cursor = viol_cursor_pack(nx);
          if (!next_cursor) throw std::runtime_error("gk_resident_violations: the position does not fit a cursor");
        }
      }
    }
    // ---- the page's objects: inventory paths, and with GK_VIOLATIONS_RENDER what gk_resident_review answers for each
    const gk_engine::ResChunk* pc = slots.empty() ? nullptr : &R.chunks[page_chunk];
    {
      size_t room = 0;
      for (uint32_t slot : slots) { room += 3; for (const std::string& seg : R.objs[pc->obj_of_slot[slot]].path) room += seg.size() + 3; }
      std::string& a = h->path_arena;
      a.reserve(room + room / 8);   // (escapes are rare; the string grows by itself when they are not)
      std::vector<size_t> at;
      at.reserve(slots.size());
      for (uint32_t slot : slots) {
        at.push_back(a.size());
        append_path_json(R.objs[pc->obj_of_slot[slot]].path, a);
        a += '\0';
      }
      h->paths.reserve(slots.size());
      for (size_t off : at) h->paths.push_back(a.data() + off);   // (after the last append: the arena no longer moves)
    }
    if ((flags & GK_VIOLATIONS_RENDER) && !slots.empty()) {
      std::vector<size_t> todo(slots.size());   // every entry has a result
      for (size_t i = 0; i < todo.size(); i++) todo[i] = i;
      std::string err;
      const int st = resident_render_page(e, *pc, slots, todo, &h->result_text, &err);
      if (st != GK_OK) return fail(st, err);
      for (const std::string& r : h->result_text) h->results.push_back(r.c_str());
    }
    gk_violations_out& p = h->pub;
    memset(&p, 0, sizeof p);
    p.n_objects = R.n_live; p.n_constraints = nc; p.n_chunks = (uint32_t)R.chunks.size(); p.mask_words = mw;
    p.constraint_ids = h->ids.data();
    p.total_objects = total;
    p.n_entries = (uint32_t)slots.size();
    p.paths = h->paths.empty() ? nullptr : h->paths.data();
    p.viol = h->viol.data(); p.err = h->err.data();
    p.results_json = h->results.empty() ? nullptr : h->results.data();
    p.beyond_limits = beyond;
    p.next_cursor = next_cursor;
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_violations_free(gk_violations_out* o) { if (o) delete reinterpret_cast<ViolationsHolder*>(o); }

// ---- gk_resident_changes: what differs in that stream's answer since the last changes stream that was handed out completely
// (viol_stream.hpp: pages and cursors; delta_stream.hpp: the pairs only the host knows)
namespace {
struct ChangesHolder {
  gk_changes_out pub;   // first member
  std::vector<uint32_t> ids, entry_flags;
  std::vector<uint64_t> viol, err, was_viol, was_err;
  std::string path_arena;
  std::vector<std::string> result_text;
  std::vector<const char*> paths, results;
};

// per plan group the constraint ids in bitmap-row order: what a baseline is comparable with (plan_rw held)
std::vector<std::vector<uint32_t>> changes_group_ids(const gk_engine* e) {
  std::vector<std::vector<uint32_t>> v;
  for (const auto& g : e->groups) v.push_back(g->ids);
  return v;
}

// The index of one chunk against its baseline (reset: against nothing).  Per plan group the device marks the shown-now or shown-then
// slots whose bits differ (dev_delta_index); the pairs no device bitmap carries are listed as they are now and compared with the
// baseline's lists.  A slot counts once whatever its sources: the words are ORed before they are counted.  R.mu and plan_rw (shared) held.
void resident_delta_index(gk_engine* e, gk_engine::ResChunk& c, const std::vector<uint32_t>& ids, bool reset, uint64_t base_gen, float* ms) {
  gk_table* t = c.table;
  const gk_eval_out* ev = c.ev;
  const uint32_t pw = (t->n_reviews + 63u) / 64u, nt = ev->n_tiles, rows = std::min<uint32_t>(ev->n_constraints, (uint32_t)ids.size());
  const bool use_base = !reset && c.cs_has_base;
  auto shown_bit = [&](uint32_t slot) { return slot / 64 < c.shown.size() && ((c.shown[slot / 64] >> (slot % 64)) & 1ull); };
  c.cs_now_err.clear(); c.cs_now_hviol.clear();
  for (uint32_t w = 0; w < pw && w < nt && w < c.shown.size(); w++) {   // (word by word, slot by slot: the list comes out in order)
    uint64_t any = 0;
    for (uint32_t row = 0; row < rows; row++) any |= ev->err[(size_t)row * nt + w];
    for (uint64_t m = any & c.shown[w]; m; m &= m - 1) {
      const uint32_t b = (uint32_t)__builtin_ctzll(m), slot = w * 64u + b;
      if (slot >= t->n_reviews) break;
      for (uint32_t row = 0; row < rows; row++)
        if ((ev->err[(size_t)row * nt + w] >> b) & 1ull) c.cs_now_err.emplace_back(slot, row);
    }
  }
  {
    std::lock_guard<std::mutex> hl(t->host_mu);
    if (t->host_ids == ids)
      for (auto& hp : t->host_viol) if (hp.first < rows && hp.second < t->n_reviews && shown_bit(hp.second)) c.cs_now_hviol.emplace_back(hp.second, hp.first);
  }
  delta_pairs_sort(&c.cs_now_hviol);
  static const std::vector<DeltaPair> none;
  const std::vector<uint32_t> host_slots = viol_merge_slots(delta_pairs_changed(c.cs_now_err, use_base ? c.cs_base_err : none),
                                                            delta_pairs_changed(c.cs_now_hviol, use_base ? c.cs_base_hviol : none));
  std::vector<uint64_t> changed(pw, 0), a;
  for (uint32_t slot : host_slots) if (slot < t->n_reviews) changed[slot / 64] |= 1ull << (slot % 64);
  c.cs_merged = !host_slots.empty() || (e->groups.size() > 1 && t->sides.size() > 1);
  std::vector<uint32_t> n;
  each_group(e, t, [&](const GroupAt& g) {
    if (g.nc == 0) return;
    float m = 0;
    dev_delta_index(g.side.dev, g.nc, t->n_reviews, c.shown, c.shown_gen, use_base, &n, &a, &m);
    if (n.size() != pw || a.size() != pw) throw std::runtime_error("dev_delta_index: wrong size");
    for (uint32_t w = 0; w < pw; w++) changed[w] |= a[w];
    *ms += m;
  });
  c.cs_prefix.assign((size_t)pw + 1, 0);
  for (uint32_t w = 0; w < pw; w++) c.cs_prefix[w + 1] = c.cs_prefix[w] + (uint64_t)__builtin_popcountll(changed[w]);
  c.cs_changed.swap(changed);
  c.cs_plan_gen = c.plan_gen; c.cs_shown_gen = c.shown_gen; c.cs_base_gen = base_gen; c.cs_reset = reset;
}
}  // namespace

int gk_resident_changes(gk_engine* e, uint64_t cursor, uint32_t max_objects, uint32_t flags, gk_changes_out** out) {
  if (!e || !out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    gk_engine::Resident& R = e->resident;
    std::lock_guard<std::mutex> rl(R.mu);
    std::unique_ptr<ChangesHolder> h(new ChangesHolder());
    if (cursor == 0) {   // a stream begins: the set is brought up to date as by gk_resident_sweep
      uint64_t flattened = 0;
      auto t1 = std::chrono::steady_clock::now();
      int rc = resident_update(e, &flattened, &t1, &h->ids);
      if (rc != GK_OK) return rc;
      R.swept = true;
    } else {
      if (!R.swept || R.cs_gen == 0 || R.set_gen != R.cs_set_gen || R.compactions != R.cs_compactions) return fail(GK_ERR_INVALID, k_stream_moved);
      { std::shared_lock<std::shared_mutex> l(e->mu); if (e->excluder_gen != R.cs_excl_gen) return fail(GK_ERR_INVALID, k_stream_moved); }
      if (!R.chunks.empty()) h->ids.assign(R.chunks[0].ev->constraint_ids, R.chunks[0].ev->constraint_ids + R.chunks[0].ev->n_constraints);
    }
    const uint32_t nc = (uint32_t)h->ids.size(), mw = (nc + 63u) / 64u;
    uint64_t beyond = 0, total = 0, next_cursor = 0;
    float device_ms = 0;
    std::vector<uint32_t> slots;
    uint32_t page_chunk = 0;
    bool reset = false;
    {
      std::shared_lock<std::shared_mutex> pl(e->plan_rw);
      if (cursor == 0) {
        for (auto& c : R.chunks)
          if (e->plan_dirty || c.plan_gen != e->plan_gen) return fail(GK_ERR_DEVICE, "the policies changed while gk_resident_changes ran: call it again");
        // is there a baseline these bitmaps can be compared with?
        reset = R.cs_base_gen == 0 || (flags & GK_CHANGES_RESTART) || R.compactions != R.cs_base_compactions || changes_group_ids(e) != R.cs_base_ids;
        for (auto& c : R.chunks) {
          if (reset || !c.cs_has_base) continue;
          each_group(e, c.table, [&](const GroupAt& g) { if (g.nc && !dev_delta_has(g.side.dev, g.nc)) reset = true; });   // (a side that lost its copy)
        }
        for (auto& c : R.chunks)
          if (c.cs_prefix.empty() || c.cs_plan_gen != c.plan_gen || c.cs_shown_gen != c.shown_gen || c.cs_base_gen != R.cs_base_gen || c.cs_reset != reset)
            resident_delta_index(e, c, h->ids, reset, R.cs_base_gen, &device_ms);
        const uint64_t plan_gen = e->plan_gen, excl_gen = R.chunks.empty() ? 0 : R.chunks[0].excl_gen;
        if (R.cs_gen == 0 || R.cs_set_gen != R.set_gen || R.cs_compactions != R.compactions || R.cs_plan_gen != plan_gen || R.cs_excl_gen != excl_gen ||
            R.cs_reset != reset || R.cs_stream_base_gen != R.cs_base_gen) {
          R.cs_gen = viol_next_gen(R.cs_gen);
          R.cs_set_gen = R.set_gen; R.cs_compactions = R.compactions; R.cs_plan_gen = plan_gen; R.cs_excl_gen = excl_gen;
          R.cs_reset = reset; R.cs_stream_base_gen = R.cs_base_gen;
        }
      } else {
        if (e->plan_dirty || e->plan_gen != R.cs_plan_gen || R.cs_stream_base_gen != R.cs_base_gen) return fail(GK_ERR_INVALID, k_stream_moved);
        reset = R.cs_reset;
        for (auto& c : R.chunks)
          if (!c.ev || c.plan_gen != e->plan_gen || c.cs_prefix.empty() || c.cs_plan_gen != c.plan_gen || c.cs_shown_gen != c.shown_gen || c.excl_gen != R.cs_excl_gen ||
              c.cs_base_gen != R.cs_base_gen || c.cs_reset != reset)
            return fail(GK_ERR_INVALID, k_stream_moved);
      }
      std::vector<uint32_t> chunk_words;
      for (auto& c : R.chunks) {
        chunk_words.push_back((uint32_t)(c.cs_prefix.size() - 1));
        total += c.cs_prefix.back();
        beyond += shown_beyond(c);
      }
      // where the page begins: the cursor's word, or the first word of the set that has entries
      ViolCursor at;
      bool have = false;
      if (cursor != 0) {
        if (!viol_cursor_check(cursor, R.cs_gen, chunk_words, &at)) return fail(GK_ERR_INVALID, k_stream_moved);
        if (viol_next_word(R.chunks[at.chunk].cs_prefix, at.word) != at.word) return fail(GK_ERR_INVALID, k_stream_moved);   // (no page begins at a word without entries)
        have = true;
      } else {
        at.gen = R.cs_gen;
        for (uint32_t ci = 0; ci < R.chunks.size() && !have; ci++) {
          const uint32_t w = viol_next_word(R.chunks[ci].cs_prefix, 0);
          if (w < chunk_words[ci]) { at.chunk = ci; at.word = w; have = true; }
        }
      }
      if (have) {
        gk_engine::ResChunk& c = R.chunks[at.chunk];
        gk_table* t = c.table;
        const uint32_t w0 = at.word, w1 = viol_page_end(c.cs_prefix, w0, max_objects);
        const uint32_t rows = std::min<uint32_t>(c.ev->n_constraints, nc);
        const bool use_base = !reset && c.cs_has_base;
        page_chunk = at.chunk;
        // the page's slots are the index's words; every plan group emits its masks of the two sides for them
        for (uint32_t w = w0; w < w1; w++)
          for (uint64_t m = c.cs_changed[w]; m; m &= m - 1) slots.push_back(w * 64u + (uint32_t)__builtin_ctzll(m));
        std::vector<uint32_t> off((size_t)(w1 - w0) + 1);
        for (uint32_t w = w0; w <= w1; w++) off[w - w0] = (uint32_t)(c.cs_prefix[w] - c.cs_prefix[w0]);
        const std::vector<uint64_t> extra(c.cs_changed.begin() + w0, c.cs_changed.begin() + w1);
        h->viol.assign(slots.size() * (size_t)mw, 0); h->err.assign(slots.size() * (size_t)mw, 0);
        h->was_viol.assign(slots.size() * (size_t)mw, 0); h->was_err.assign(slots.size() * (size_t)mw, 0);
        each_group(e, t, [&](const GroupAt& g) {
          if (g.nc == 0) return;
          std::vector<uint32_t> rev;
          std::vector<uint64_t> now, was;
          float m = 0;
          dev_delta_entries(g.side.dev, g.nc, t->n_reviews, c.shown, c.shown_gen, use_base, w0, w1, off, c.cs_merged ? &extra : nullptr, &rev, &now, &was, &m);
          device_ms += m;
          if (rev != slots) throw std::runtime_error("gk_resident_changes: the page's entries do not add up to the chunk's index");
          if (!viol_scatter(slots, mw, rev, now, g.nc, g.row0, &h->viol) || !viol_scatter(slots, mw, rev, was, g.nc, g.row0, &h->was_viol))
            throw std::runtime_error("gk_resident_changes: a plan group's entries do not fit the page");
        });
        // the pairs no device bitmap carries: autoreject, host-completed violations -- now, and as the baseline kept them
        delta_pairs_or(c.cs_now_err, slots, mw, rows, &h->err);
        delta_pairs_or(c.cs_now_hviol, slots, mw, rows, &h->viol);
        if (use_base) {
          delta_pairs_or(c.cs_base_err, slots, mw, rows, &h->was_err);
          delta_pairs_or(c.cs_base_hviol, slots, mw, rows, &h->was_viol);
        }
        for (uint32_t slot : slots) h->entry_flags.push_back((c.shown[slot / 64] >> (slot % 64)) & 1ull ? 0u : GK_CHANGE_GONE);
        // the next page begins at the next word with entries, in this chunk or a later one
        ViolCursor nx;
        nx.gen = R.cs_gen;
        bool more = false;
        for (uint32_t ci = at.chunk; ci < R.chunks.size() && !more; ci++) {
          const uint32_t w = viol_next_word(R.chunks[ci].cs_prefix, ci == at.chunk ? w1 : 0);
          if (w < chunk_words[ci]) { nx.chunk = ci; nx.word = w; more = true; }
        }
        if (more) {
          next_cursor = viol_cursor_pack(nx);
          if (!next_cursor) throw std::runtime_error("gk_resident_changes: the position does not fit a cursor");
        }
      }
    }
    // ---- the page's objects: inventory paths, and with GK_CHANGES_RENDER what gk_resident_review answers for those with a result now
    const gk_engine::ResChunk* pc = slots.empty() ? nullptr : &R.chunks[page_chunk];
    {
      std::string& a = h->path_arena;
      std::vector<size_t> at;
      at.reserve(slots.size());
      for (uint32_t slot : slots) {
        at.push_back(a.size());
        append_path_json(R.objs[pc->obj_of_slot[slot]].path, a);
        a += '\0';
      }
      h->paths.reserve(slots.size());
      for (size_t off : at) h->paths.push_back(a.data() + off);   // (after the last append: the arena no longer moves)
    }
    if ((flags & GK_CHANGES_RENDER) && !slots.empty()) {
      std::vector<size_t> todo;   // entries with a result now
      for (size_t i = 0; i < slots.size(); i++) {
        uint64_t any = 0;
        for (uint32_t k = 0; k < mw; k++) any |= h->viol[i * mw + k] | h->err[i * mw + k];
        if (any) todo.push_back(i);
      }
      std::string err;
      const int st = resident_render_page(e, *pc, slots, todo, &h->result_text, &err);
      if (st != GK_OK) return fail(st, err);
      h->results.assign(slots.size(), nullptr);
      for (size_t i : todo) h->results[i] = h->result_text[i].c_str();
    }
    uint64_t base_bytes = 0;
    {
      std::shared_lock<std::shared_mutex> pl(e->plan_rw);
      if (next_cursor == 0) {
        // ---- the last page: the baseline becomes the streamed state.  A chunk that has a baseline and no entry keeps its copy (what
        // it shows is what the baseline shows); afterwards every chunk's index against the NEW baseline is known to be empty.
        if (e->plan_dirty || e->plan_gen != R.cs_plan_gen) return fail(GK_ERR_INVALID, k_stream_moved);
        try {
          for (auto& c : R.chunks) {
            if (!reset && c.cs_has_base && c.cs_prefix.back() == 0) continue;
            each_group(e, c.table, [&](const GroupAt& g) { if (g.nc) dev_delta_keep(g.side.dev, g.nc, c.table->n_reviews, c.shown, c.shown_gen); });
            c.cs_has_base = true;
            c.cs_base_shown = c.shown;
            c.cs_base_err = c.cs_now_err; c.cs_base_hviol = c.cs_now_hviol;
          }
        } catch (...) {   // (half a baseline is none: the next stream starts over)
          R.cs_base_gen = 0;
          for (auto& c : R.chunks) { c.cs_has_base = false; c.cs_prefix.clear(); }
          throw;
        }
        R.cs_base_gen++;
        R.cs_base_compactions = R.compactions;
        R.cs_base_ids = changes_group_ids(e);
        for (auto& c : R.chunks) {
          std::fill(c.cs_prefix.begin(), c.cs_prefix.end(), 0);
          std::fill(c.cs_changed.begin(), c.cs_changed.end(), 0);
          c.cs_merged = e->groups.size() > 1 && c.table->sides.size() > 1;
          c.cs_base_gen = R.cs_base_gen; c.cs_reset = false;
        }
      }
      for (auto& c : R.chunks) each_group(e, c.table, [&](const GroupAt& g) { base_bytes += dev_delta_bytes(g.side.dev); });
    }
    gk_changes_out& p = h->pub;
    memset(&p, 0, sizeof p);
    p.n_objects = R.n_live; p.n_constraints = nc; p.n_chunks = (uint32_t)R.chunks.size(); p.mask_words = mw;
    p.constraint_ids = h->ids.data();
    p.reset = reset ? 1u : 0u;
    p.total_entries = total;
    p.n_entries = (uint32_t)slots.size();
    p.paths = h->paths.empty() ? nullptr : h->paths.data();
    p.viol = h->viol.data(); p.err = h->err.data(); p.was_viol = h->was_viol.data(); p.was_err = h->was_err.data();
    p.entry_flags = h->entry_flags.data();
    p.results_json = h->results.empty() ? nullptr : h->results.data();
    p.beyond_limits = beyond;
    p.next_cursor = next_cursor;
    p.device_ms = device_ms;
    p.baseline_bytes = base_bytes;
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_changes_free(gk_changes_out* o) { if (o) delete reinterpret_cast<ChangesHolder*>(o); }

// ---- gk_table_violations: every review of a table with at least one result in its most recent evaluation, in pages (table_stream.hpp
// holds the pure part; the device compacts both bitmaps of all plan groups: dev_tviol_index / dev_tviol_entries)
namespace {
struct TableViolationsHolder {
  gk_table_violations_out pub;   // first member
  std::vector<uint32_t> ids, reviews;
  std::vector<uint64_t> viol, err;
  std::vector<std::string> result_text;
  std::vector<const char*> results;
};
const char* const k_table_stream_moved = "the table was evaluated again or the policies changed since the stream began: start again with cursor 0";

// the rows of one entry as gk_query's JSON: ascending bitmap row; an err bit gives gk_render_error's row, a viol bit gk_render's rows
std::string table_entry_json(gk_engine* e, gk_table* t, const std::vector<uint32_t>& ids, uint32_t r, const uint64_t* viol, const uint64_t* err) {
  ReviewDoc tmp;
  const ReviewDoc* doc = doc_for(e, t, r, &tmp);
  if (!doc) throw std::runtime_error("review document unavailable");
  std::string out = "[";
  std::shared_lock<std::shared_mutex> l(e->mu);
  for (uint32_t row = 0; row < ids.size(); row++) {
    const bool is_err = (err[row / 64] >> (row % 64)) & 1ull, is_viol = (viol[row / 64] >> (row % 64)) & 1ull;
    if (!is_err && !is_viol) continue;
    const uint32_t cid = ids[row];
    if (cid >= e->constraints.size()) throw std::runtime_error("unknown constraint id");
    const ConstraintRec& c = e->constraints[cid];
    if (is_err) {
      ValuePairs o{{Value::string("constraint"), Value::integer(cid)}, {Value::string("msg"), Value::string(autoreject_message(c.match, *doc))},
                   {Value::string("autoreject"), Value::boolean(true)}, {Value::string("details"), Value::object({})}};
      if (out.size() > 1) out += ",";
      out += to_json(Value::object(o));
    }
    if (!is_viol) continue;
    auto it = e->templates.find(lower_str(c.kind));
    // (as gk_query: a flagged pair that renders nothing is a disagreement between the plan and the evaluator, never "no results")
    if (it == e->templates.end()) throw std::runtime_error("device / renderer disagree: constraint " + c.kind + "/" + c.name + " has no template");
    const auto vs = it->second->render(doc->request, c.params, e->inventory);
    if (vs.empty()) throw std::runtime_error("device / renderer disagree: the plan reports a violation of " + c.kind + "/" + c.name + " that the evaluator does not render");
    for (auto& v : vs) {
      static const Value k_constraint = Value::string("constraint"), k_msg = Value::string("msg"), k_details = Value::string("details"), no_details = Value::object({});
      ValuePairs o{{k_constraint, Value::integer(cid)}, {k_details, v.details.defined() ? v.details : no_details}, {k_msg, Value::string(v.msg)}};
      if (out.size() > 1) out += ",";
      out += to_json(Value::object(o));
    }
  }
  return out + "]";
}
// The entries of a page rendered on the host workers (GK_HOST_THREADS): texts[i] = table_entry_json of entry i, for every entry or, with
// `todo`, for the listed ones (the others stay empty).  Returns the first error's text (the remaining entries are then not rendered).
std::string table_render_entries(gk_engine* e, gk_table* t, const std::vector<uint32_t>& ids, const std::vector<uint32_t>& reviews, const std::vector<uint64_t>& viol,
                                 const std::vector<uint64_t>& err, uint32_t mw, const std::vector<size_t>* todo, std::vector<std::string>* texts) {
  const size_t n = todo ? todo->size() : reviews.size();
  texts->assign(reviews.size(), std::string());
  std::string first_err;
  if (n == 0) return first_err;
  size_t n_threads = std::max<size_t>(1, std::min<size_t>(host_cpus(), n));
  if (const char* ht = getenv("GK_HOST_THREADS")) n_threads = std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, atoi(ht)), n));
  std::atomic<size_t> next{0};
  std::mutex err_mu;
  auto worker = [&](size_t) {   // one entry per task, handed out in page order
    for (;;) {
      const size_t k = next.fetch_add(1);
      if (k >= n) return;
      const size_t i = todo ? (*todo)[k] : k;
      try {
        (*texts)[i] = table_entry_json(e, t, ids, reviews[i], viol.data() + i * mw, err.data() + i * mw);
      } catch (const std::exception& ex) {
        std::lock_guard<std::mutex> l(err_mu);
        if (first_err.empty()) first_err = ex.what()[0] ? ex.what() : "rendering failed";
        next.store(n);   // (the call fails: the remaining entries are not rendered)
      }
    }
  };
  HostWorkers::get().run(n_threads, worker);
  return first_err;
}
}  // namespace

int gk_table_violations(gk_engine* e, gk_table* t, uint64_t cursor, uint32_t max_entries, uint32_t flags, gk_table_violations_out** out) {
  if (!e || !t || !out) return fail(GK_ERR_INVALID, "NULL argument");
  if ((flags & GK_VIOLATIONS_RENDER) && t->docs.size() != t->n_reviews && t->texts.size() != t->n_reviews)
    return fail(GK_ERR_INVALID, "gk_table_violations: GK_VIOLATIONS_RENDER needs a table created with GK_TABLE_KEEP_DOCS / GK_TABLE_KEEP_TEXT");
  try {
    if (const char* why = table_stale(e, t)) return fail(GK_ERR_INVALID, cursor ? k_table_stream_moved : why);   // (stale: the policies changed)
    std::unique_ptr<TableViolationsHolder> h(new TableViolationsHolder());
    const uint32_t pw = (t->n_reviews + 63u) / 64u;
    float device_ms = 0;
    uint64_t next_cursor = 0, beyond = 0;
    {
      std::shared_lock<std::shared_mutex> l(e->plan_rw);
      if (!t->sides.empty() && !t->sides[0].shard.shard_reviews.empty())
        return fail(GK_ERR_INVALID, "gk_table_violations: the table is set up as a shard (gk_table_sweep_sharded), its bitmaps live in the exchange buffer: stream a table of its own");
      if (t->ts_pending) return fail(GK_ERR_INVALID, "gk_table_violations: launches of the table are still to be collected (gk_table_eval without GK_EVAL_ASYNC)");
      if (t->ts_gen == 0 || t->eval_plan_gen == 0) return fail(GK_ERR_INVALID, "gk_table_violations: evaluate the table first (gk_table_eval)");
      if (e->plan_dirty || e->plan_gen != t->eval_plan_gen)
        return fail(GK_ERR_INVALID, cursor ? k_table_stream_moved : "gk_table_violations: the policies changed since the table was evaluated: evaluate it again (gk_table_eval)");
      h->ids = t->last_ids;
      const uint32_t nc = (uint32_t)h->ids.size(), mw = (nc + 63u) / 64u;
      std::vector<TviolSide> sides;
      uint32_t rows = 0;
      each_group(e, t, [&](const GroupAt& g) { sides.push_back(TviolSide{g.side.dev, g.nc, g.row0}); rows = g.row0 + g.nc; });
      if (rows != nc) return fail(GK_ERR_INVALID, "gk_table_violations: evaluate the table first (gk_table_eval)");
      // what the host evaluation of THIS evaluation added (another evaluation's, another policy set's: none of it)
      TablePairs hv, he;
      size_t n_done = 0;
      {
        std::lock_guard<std::mutex> hl(t->host_mu);
        if (t->host_gen == t->ts_gen && t->host_ids == h->ids) { hv = t->host_viol; he = t->host_err; n_done = t->host_done.size(); }
      }
      uint32_t w0 = 0;
      if (cursor == 0) {
        if (t->ts_index_gen != t->ts_gen || t->ts_prefix.size() != (size_t)pw + 1) {   // the index, once per evaluation
          std::vector<uint64_t> host_words;
          if (!hv.empty() || !he.empty()) host_words = table_host_words(hv, he, nc, t->n_reviews);
          std::vector<uint32_t> cnt;
          std::vector<uint64_t> any;
          uint64_t dev_beyond = 0;
          dev_tviol_index(sides, t->n_reviews, &cnt, host_words.empty() ? nullptr : &any, &dev_beyond, &device_ms);
          if (cnt.size() != pw || !table_prefix(cnt, any, host_words, &t->ts_prefix)) throw std::runtime_error("dev_tviol_index: wrong size");
          t->ts_dev_off.assign((size_t)pw + 1, 0);
          for (uint32_t w = 0; w < pw; w++) t->ts_dev_off[w + 1] = t->ts_dev_off[w] + cnt[w];
          t->ts_beyond = dev_beyond > n_done ? dev_beyond - n_done : 0;   // (every host-answered review had its too_big bit set)
          t->ts_index_gen = t->ts_gen;
        }
        w0 = viol_next_word(t->ts_prefix, 0);
      } else {
        if (t->ts_index_gen != t->ts_gen || t->ts_prefix.size() != (size_t)pw + 1 || !table_cursor_check(cursor, t->ts_gen, pw, &w0)) return fail(GK_ERR_INVALID, k_table_stream_moved);
        if (viol_next_word(t->ts_prefix, w0) != w0) return fail(GK_ERR_INVALID, k_table_stream_moved);   // (no page begins at a word without entries)
      }
      beyond = t->ts_beyond;
      h->pub.total_entries = t->ts_prefix.back();
      if (w0 < pw) {
        const uint32_t w1 = viol_page_end(t->ts_prefix, w0, max_entries);
        std::vector<uint32_t> rev;
        std::vector<uint64_t> dv, de;
        float ms = 0;
        dev_tviol_entries(sides, t->n_reviews, t->ts_dev_off, w0, w1, &rev, &dv, &de, &ms);
        device_ms += ms;
        if (!table_merge_page(rev, dv, de, mw, hv, he, nc, t->n_reviews, w0, w1, &h->reviews, &h->viol, &h->err))
          throw std::runtime_error("gk_table_violations: the device's entries do not fit the page");
        if (h->reviews.size() != t->ts_prefix[w1] - t->ts_prefix[w0]) throw std::runtime_error("gk_table_violations: the page's entries do not add up to the table's index");
        const uint32_t nx = viol_next_word(t->ts_prefix, w1);
        if (nx < pw) {
          next_cursor = table_cursor_pack(t->ts_gen, nx);
          if (!next_cursor) throw std::runtime_error("gk_table_violations: the position does not fit a cursor");
        }
      }
    }
    const uint32_t mw = ((uint32_t)h->ids.size() + 63u) / 64u;
    if ((flags & GK_VIOLATIONS_RENDER) && !h->reviews.empty()) {
      const std::string first_err = table_render_entries(e, t, h->ids, h->reviews, h->viol, h->err, mw, nullptr, &h->result_text);
      if (!first_err.empty()) return fail(GK_ERR_REGO, first_err);
      for (const std::string& r : h->result_text) h->results.push_back(r.c_str());
    }
    gk_table_violations_out& p = h->pub;
    const uint64_t total = p.total_entries;
    memset(&p, 0, sizeof p);
    p.n_reviews = t->n_reviews; p.n_constraints = (uint32_t)h->ids.size(); p.mask_words = mw;
    p.constraint_ids = h->ids.data();
    p.total_entries = total;
    p.n_entries = (uint32_t)h->reviews.size();
    p.reviews = h->reviews.data(); p.viol = h->viol.data(); p.err = h->err.data();
    p.results_json = h->results.empty() ? nullptr : h->results.data();
    p.beyond_limits = beyond;
    p.next_cursor = next_cursor;
    p.device_ms = device_ms;
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_table_violations_free(gk_table_violations_out* o) { if (o) delete reinterpret_cast<TableViolationsHolder*>(o); }

// ---- gk_table_snapshot / gk_table_changes: one list-based cycle's answer against a kept earlier one (table_delta.hpp holds the pure
// part; the device lines the snapshot up with the table and compacts the difference: dev_snap_take / dev_tchg_align / _index / _entries)
struct gk_snapshot {
  gk_engine* eng = nullptr;
  uint64_t serial = 0;                    // unique per snapshot of the process: what a stream remembers of its `then`
  uint32_t n_reviews = 0;
  std::vector<uint32_t> ids;              // constraint id per bitmap row
  DevSnap* dev = nullptr;
  TablePairs host_viol, host_err;         // what the host evaluation of the kept evaluation added
  std::vector<uint32_t> host_done;        // the reviews it answered, ascending
  uint64_t beyond = 0;
  std::string key_bytes;                  // the reviews' keys one after the other ...
  std::vector<std::pair<uint64_t, uint32_t>> key_span;   // ... (offset, length) per review
  // the reviews in key order (table_key_order).  A snapshot taken with GK_SNAPSHOT_DEVICE_KEYS does not sort: key_order() builds the
  // order when a host join first asks for it.  dkeys: the keys as packed records on the device (key_join.hpp), uploaded when the
  // snapshot is taken with that flag, else by the first device join against it (device_keys()); keys_unfit: they do not fit.  Both
  // are filled in once, under lazy_mu: a snapshot never changes otherwise, and any number of streams may read it.
  mutable std::vector<uint32_t> order;
  mutable DevKeys* dkeys = nullptr;
  mutable bool keys_unfit = false;
  mutable std::mutex lazy_mu;
  std::vector<uint64_t> versions;
  bool has_versions = false;
  std::string_view key(size_t i) const { return std::string_view(key_bytes.data() + key_span[i].first, key_span[i].second); }
  const std::vector<uint32_t>& key_order() const {
    std::lock_guard<std::mutex> l(lazy_mu);
    if (order.size() != n_reviews) {
      order.resize(n_reviews);
      for (uint32_t i = 0; i < n_reviews; i++) order[i] = i;
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    }
    return order;
  }
  // nullptr: the keys do not fit 32-bit offsets in 16-byte units
  const DevKeys* device_keys(int device) const {
    std::lock_guard<std::mutex> l(lazy_mu);
    if (!dkeys && !keys_unfit) {
      KjPacked pk;
      if (!kjoin_pack(n_reviews, [&](uint32_t i) { return key(i); }, &pk)) keys_unfit = true;
      else dkeys = dev_keys_put(device, pk.rec.data(), pk.rec.size(), pk.off.data(), n_reviews);
    }
    return dkeys;
  }
  ~gk_snapshot() { dev_snap_free(dev); dev_keys_free(dkeys); }
};

namespace {
struct TableChangesHolder {
  gk_table_changes_out pub;   // first member
  std::vector<uint32_t> ids, reviews, was_reviews, flags;
  std::vector<uint64_t> viol, err, was_viol, was_err;
  std::vector<std::string> key_text, result_text;
  std::vector<const char*> keys, results;
};
std::atomic<uint64_t> g_snapshot_serial{0};

// why the answer of the table's most recent evaluation cannot be read (empty: it can) -- gk_table_violations' refusals; plan_rw held
std::string table_answer_refusal(const gk_engine* e, const gk_table* t, const char* who, bool later_page) {
  const std::string w = std::string(who) + ": ";
  if (!t->sides.empty() && !t->sides[0].shard.shard_reviews.empty())
    return w + "the table is set up as a shard (gk_table_sweep_sharded), its bitmaps live in the exchange buffer: use a table of its own";
  if (t->ts_pending) return w + "launches of the table are still to be collected (gk_table_eval without GK_EVAL_ASYNC)";
  if (t->ts_gen == 0 || t->eval_plan_gen == 0) return w + "evaluate the table first (gk_table_eval)";
  if (e->plan_dirty || e->plan_gen != t->eval_plan_gen)
    return later_page ? std::string(k_table_stream_moved) : w + "the policies changed since the table was evaluated: evaluate it again (gk_table_eval)";
  return std::string();
}
// the table's sides as the device entries take them; false: the table was not evaluated under the plan groups there are now
bool table_tviol_sides(const gk_engine* e, gk_table* t, uint32_t nc, std::vector<TviolSide>* sides) {
  uint32_t rows = 0;
  each_group(e, t, [&](const GroupAt& g) { sides->push_back(TviolSide{g.side.dev, g.nc, g.row0}); rows = g.row0 + g.nc; });
  return rows == nc;
}
void append_key_json(std::string_view key, std::string& out) {
  out += '[';
  size_t at = 0;
  for (int part = 0; part < 5; part++) {
    size_t end = part == 4 ? key.size() : key.find('\0', at);
    if (end == std::string_view::npos) end = key.size();
    if (part) out += ',';
    json_escape(std::string(key.substr(std::min(at, key.size()), end - std::min(at, key.size()))), out);
    at = std::min(end + 1, key.size() + 1);
  }
  out += ']';
}
std::vector<uint32_t> narrow_slice(const std::vector<uint64_t>& prefix, uint32_t w0, uint32_t w1) {
  std::vector<uint32_t> off((size_t)(w1 - w0) + 1);
  for (uint32_t w = w0; w <= w1; w++) off[w - w0] = (uint32_t)(prefix[w] - prefix[w0]);
  return off;
}
std::vector<uint64_t> word_slice(const std::vector<uint64_t>& words, uint32_t w0, uint32_t w1) {
  return words.empty() ? std::vector<uint64_t>() : std::vector<uint64_t>(words.begin() + w0, words.begin() + w1);
}
// The key join of the table with a snapshot (delta_join's three arrays).  on_device: the exact hash join of the two sides' packed keys
// (dev_kjoin) -- the table's keys go up once and stay with the table, the snapshot's are its own; neither side is sorted.  When a side's
// keys do not fit, or the kernels report an error, the host join answers and st->fallback says why.  Else: table_key_order + delta_join.
// *keep (device join only): then_of on the device, for dev_tchg_align.
void table_join(gk_engine* e, gk_table* t, const gk_snapshot* then, bool on_device, std::vector<uint32_t>* then_of, std::vector<uint32_t>* now_of,
                std::vector<uint64_t>* unmatched, KjoinStats* st, float* ms, DevJoin** keep) {
  *ms = 0;
  if (keep) *keep = nullptr;
  uint32_t fallback = 0;
  float pack_ms = 0;
  if (on_device) {
    const DevKeys* dn = nullptr;
    {
      std::lock_guard<std::mutex> l(t->keys_mu);
      if (!t->dkeys && !t->keys_unfit) {
        const auto t0 = std::chrono::steady_clock::now();
        KjPacked pk;
        if (!kjoin_pack(t->n_reviews, [&](uint32_t i) { return t->obj_key(i); }, &pk)) t->keys_unfit = true;
        else t->dkeys = dev_keys_put(e->opts.device, pk.rec.data(), pk.rec.size(), pk.off.data(), t->n_reviews);
        pack_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
      }
      dn = t->dkeys;
    }
    const DevKeys* dt = dn ? then->device_keys(e->opts.device) : nullptr;
    if (!dn || !dt) fallback = 1;
    else {
      try {
        std::vector<uint64_t> flagged_now, flagged_then;
        const KjKeyFn key_now{[](const void* c, uint32_t i) { return static_cast<const gk_table*>(c)->obj_key(i); }, t};
        const KjKeyFn key_then{[](const void* c, uint32_t i) { return static_cast<const gk_snapshot*>(c)->key(i); }, then};
        dev_kjoin(dn, dt, g_debug_kjoin_hash_bits.load(), key_now, key_then, then_of, now_of, unmatched, &flagged_now, &flagged_then, st, ms, keep);
        st->pack_ms = pack_ms;
        return;
      } catch (const KjoinFault&) { fallback = 2; *ms = 0; }
    }
  }
  table_key_order(t);
  delta_join(t->order, [&](uint32_t i) { return t->obj_key(i); }, then->key_order(), [&](uint32_t i) { return then->key(i); }, then_of, now_of, unmatched);
  *st = KjoinStats();
  st->n_now = t->n_reviews; st->n_then = then->n_reviews; st->fallback = fallback; st->pack_ms = pack_ms;
}
void join_stats_out(const KjoinStats& st, float ms, struct gk_join_stats* out) {
  memset(out, 0, sizeof *out);
  out->n_now = st.n_now; out->n_then = st.n_then; out->capacity = st.capacity;
  out->host_resolved_now = st.host_resolved_now; out->host_resolved_then = st.host_resolved_then;
  out->device = st.device; out->fallback = st.fallback; out->join_ms = ms; out->pack_ms = st.pack_ms;
}
struct TableJoinHolder {
  gk_table_join_out pub;   // first member
  std::vector<uint32_t> then_of, now_of;
};
}  // namespace

int gk_table_join(gk_engine* e, gk_table* t, const gk_snapshot* then, uint32_t flags, gk_table_join_out** out) {
  if (!e || !t || !then || !out) return fail(GK_ERR_INVALID, "NULL argument");
  if (flags & ~GK_CHANGES_DEVICE_JOIN) return fail(GK_ERR_INVALID, "gk_table_join: unknown flags");
  if (then->eng != e || t->eng != e) return fail(GK_ERR_INVALID, "gk_table_join: the snapshot belongs to another engine");
  try {
    std::unique_ptr<TableJoinHolder> h(new TableJoinHolder());
    std::vector<uint64_t> unmatched;
    KjoinStats st;
    float ms = 0;
    table_join(e, t, then, (flags & GK_CHANGES_DEVICE_JOIN) != 0, &h->then_of, &h->now_of, &unmatched, &st, &ms, nullptr);
    memset(&h->pub, 0, sizeof h->pub);
    h->pub.n_now = t->n_reviews; h->pub.n_then = then->n_reviews;
    h->pub.then_of = h->then_of.data(); h->pub.now_of = h->now_of.data();
    join_stats_out(st, ms, &h->pub.stats);
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_table_join_free(gk_table_join_out* o) { if (o) delete reinterpret_cast<TableJoinHolder*>(o); }

int gk_table_changes_join(gk_engine* e, gk_table* t, struct gk_join_stats* out) {
  if (!e || !t || !out) return fail(GK_ERR_INVALID, "NULL argument");
  if (t->tc.gen == 0 || t->tc.gen != t->ts_gen) return fail(GK_ERR_INVALID, "gk_table_changes_join: the table has no changes stream (gk_table_changes with cursor 0)");
  KjoinStats none;   // (a stream without a snapshot joined nothing: all zero but the table's reviews)
  none.n_now = t->tc.n[0];
  join_stats_out(t->tc.joined ? t->tc.join : none, t->tc.joined ? t->tc.join_ms : 0.f, out);
  return GK_OK;
}

int gk_table_snapshot(gk_engine* e, gk_table* t, const uint64_t* versions, gk_snapshot** out) { return gk_table_snapshot_ex(e, t, versions, 0, out); }

int gk_table_snapshot_ex(gk_engine* e, gk_table* t, const uint64_t* versions, uint32_t flags, gk_snapshot** out) {
  if (!e || !t || !out) return fail(GK_ERR_INVALID, "NULL argument");
  if (flags & ~GK_SNAPSHOT_DEVICE_KEYS) return fail(GK_ERR_INVALID, "gk_table_snapshot_ex: unknown flags");
  try {
    if (const char* why = table_stale(e, t)) return fail(GK_ERR_INVALID, why);
    std::unique_ptr<gk_snapshot> s(new gk_snapshot());
    s->eng = e; s->n_reviews = t->n_reviews;
    {
      std::shared_lock<std::shared_mutex> l(e->plan_rw);
      const std::string why = table_answer_refusal(e, t, "gk_table_snapshot", false);
      if (!why.empty()) return fail(GK_ERR_INVALID, why);
      s->ids = t->last_ids;
      std::vector<TviolSide> sides;
      if (!table_tviol_sides(e, t, (uint32_t)s->ids.size(), &sides)) return fail(GK_ERR_INVALID, "gk_table_snapshot: evaluate the table first (gk_table_eval)");
      {
        std::lock_guard<std::mutex> hl(t->host_mu);
        if (t->host_gen == t->ts_gen && t->host_ids == s->ids) { s->host_viol = t->host_viol; s->host_err = t->host_err; s->host_done = t->host_done; }
      }
      std::sort(s->host_done.begin(), s->host_done.end());
      s->dev = dev_snap_take(sides, t->n_reviews);
      std::vector<uint32_t> cnt;
      uint64_t dev_beyond = 0;
      float ms = 0;
      dev_tviol_index(sides, t->n_reviews, &cnt, nullptr, &dev_beyond, &ms);
      s->beyond = dev_beyond > s->host_done.size() ? dev_beyond - s->host_done.size() : 0;
    }
    if (!(flags & GK_SNAPSHOT_DEVICE_KEYS)) {
      table_key_order(t);
      s->order = t->order;
    }
    s->key_span.resize(t->n_reviews);
    size_t bytes = 0;
    for (size_t i = 0; i < t->n_reviews; i++) bytes += t->obj_key(i).size();
    s->key_bytes.reserve(bytes);
    for (size_t i = 0; i < t->n_reviews; i++) {
      const std::string_view k = t->obj_key(i);
      s->key_span[i] = {s->key_bytes.size(), (uint32_t)k.size()};
      s->key_bytes.append(k.data(), k.size());
    }
    if (versions) { s->versions.assign(versions, versions + t->n_reviews); s->has_versions = true; }
    if (flags & GK_SNAPSHOT_DEVICE_KEYS) (void)s->device_keys(e->opts.device);   // (keys that do not fit: every join against it runs on the host)
    s->serial = ++g_snapshot_serial;
    *out = s.release();
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_snapshot_free(gk_snapshot* s) { delete s; }

int gk_snapshot_info(const gk_snapshot* s, struct gk_snapshot_info* out) {
  if (!s || !out) return fail(GK_ERR_INVALID, "NULL argument");
  memset(out, 0, sizeof *out);
  out->n_reviews = s->n_reviews; out->n_constraints = (uint32_t)s->ids.size();
  out->constraint_ids = s->ids.data();
  std::lock_guard<std::mutex> l(s->lazy_mu);
  out->device_bytes = dev_snap_bytes(s->dev) + dev_keys_bytes(s->dkeys);
  out->host_bytes = s->key_bytes.size() + s->key_span.size() * sizeof(s->key_span[0]) + (s->order.size() + s->ids.size() + s->host_done.size()) * 4u + s->versions.size() * 8u +
                    (s->host_viol.size() + s->host_err.size()) * 8u;
  out->beyond_limits = s->beyond;
  return GK_OK;
}

int gk_table_changes(gk_engine* e, gk_table* t, const gk_snapshot* then, const uint64_t* versions, uint64_t cursor, uint32_t max_entries, uint32_t flags,
                     gk_table_changes_out** out) {
  if (!e || !t || !out) return fail(GK_ERR_INVALID, "NULL argument");
  if (cursor == 0 && (flags & GK_CHANGES_RENDER) && t->docs.size() != t->n_reviews && t->texts.size() != t->n_reviews)
    return fail(GK_ERR_INVALID, "gk_table_changes: GK_CHANGES_RENDER needs a table created with GK_TABLE_KEEP_DOCS / GK_TABLE_KEEP_TEXT");
  if (then && then->eng != e) return fail(GK_ERR_INVALID, "gk_table_changes: the snapshot belongs to another engine");
  try {
    if (const char* why = table_stale(e, t)) return fail(GK_ERR_INVALID, cursor ? k_table_stream_moved : why);
    std::unique_ptr<TableChangesHolder> h(new TableChangesHolder());
    float align_ms = 0, index_ms = 0, emit_ms = 0;
    uint32_t stream_flags = 0;
    uint64_t next_cursor = 0, total = 0, beyond = 0;
    uint32_t page_side = 0;
    gk_table::Changes& C = t->tc;
    {
      std::shared_lock<std::shared_mutex> l(e->plan_rw);
      const std::string why = table_answer_refusal(e, t, "gk_table_changes", cursor != 0);
      if (!why.empty()) return fail(GK_ERR_INVALID, why);
      h->ids = t->last_ids;
      const uint32_t nc = (uint32_t)h->ids.size(), mw = (nc + 63u) / 64u, n_now = t->n_reviews, n_then = then ? then->n_reviews : 0u;
      const uint32_t words[2] = {(n_now + 63u) / 64u, (n_then + 63u) / 64u};
      std::vector<TviolSide> sides;
      if (!table_tviol_sides(e, t, nc, &sides)) return fail(GK_ERR_INVALID, "gk_table_changes: evaluate the table first (gk_table_eval)");
      uint32_t side = 0, word = 0;
      if (cursor == 0) {
        table_changes_drop(t);
        C.snap_serial = then ? then->serial : 0;
        C.flags = flags;
        C.n[0] = n_now; C.n[1] = n_then;
        // what the host evaluation of THIS evaluation added (another evaluation's, another policy set's: none of it)
        TablePairs hv, he;
        std::vector<uint32_t> done;
        {
          std::lock_guard<std::mutex> hl(t->host_mu);
          if (t->host_gen == t->ts_gen && t->host_ids == h->ids) { hv = t->host_viol; he = t->host_err; done = t->host_done; }
        }
        std::sort(done.begin(), done.end());
        std::vector<uint32_t> row_of(nc, DELTA_NONE), now_row_of, now_of;
        std::vector<uint64_t> unmatched;
        C.then_of.assign(n_now, DELTA_NONE);
        std::unique_ptr<DevJoin, void (*)(DevJoin*)> joined(nullptr, dev_join_free);   // then_of on the device, when the device joined
        if (then) {
          delta_row_map(h->ids, then->ids, &row_of, &now_row_of);
          DevJoin* keep = nullptr;
          table_join(e, t, then, (flags & GK_CHANGES_DEVICE_JOIN) != 0, &C.then_of, &now_of, &unmatched, &C.join, &C.join_ms, &keep);
          joined.reset(keep);
          C.joined = true;
          if (versions && then->has_versions) {
            C.moved.assign(words[0], 0);
            for (uint32_t r = 0; r < n_now; r++)
              if (C.then_of[r] != DELTA_NONE && then->versions[C.then_of[r]] != versions[r]) C.moved[r / 64u] |= 1ull << (r % 64u);
          }
          delta_known_build(done, hv, he, n_now, nc, then->host_done, then->host_viol, then->host_err, now_of, now_row_of, &C.known[0], &C.known[1]);
        } else {
          delta_known_build(done, hv, he, n_now, nc, {}, {}, {}, now_of, now_row_of, &C.known[0], &C.known[1]);
          for (auto& kv : C.known[0]) kv.second.was = true;   // (nothing then: zero)
        }
        float ms = 0;
        // side 0: the table's reviews against what the snapshot holds of them
        if (joined) C.aligned[0] = dev_tchg_align(e->opts.device, then->dev, n_now, *joined, row_of, C.moved.empty() ? nullptr : &C.moved, nullptr, &ms);
        else C.aligned[0] = dev_tchg_align(e->opts.device, then ? then->dev : nullptr, n_now, then ? &C.then_of : nullptr, row_of, C.moved.empty() ? nullptr : &C.moved, nullptr, &ms);
        align_ms += ms;
        std::vector<uint32_t> cnt;
        std::vector<uint64_t> changed, big, entries;
        uint64_t dev_beyond = 0;
        dev_tchg_index(sides, n_now, C.aligned[0], &cnt, &changed, &big, &dev_beyond, &ms);
        index_ms += ms;
        if (changed.size() != words[0] || big.size() != words[0]) throw std::runtime_error("dev_tchg_index: wrong size");
        C.beyond = dev_beyond > done.size() ? dev_beyond - done.size() : 0;   // (every host-answered review had its too_big bit set)
        if (!C.known[0].empty()) {
          C.drop[0] = delta_known_words(C.known[0], words[0]);
          for (uint32_t w = 0; w < words[0]; w++) {   // the device's masks of the sides the host does not know: word by word, they are few
            if (!C.drop[0][w]) continue;
            std::vector<uint32_t> rev;
            std::vector<uint64_t> v, er, wv, we;
            dev_tchg_entries(sides, n_now, C.aligned[0], {0u, (uint32_t)__builtin_popcountll(changed[w] | C.drop[0][w])}, w, w + 1, {}, {C.drop[0][w]}, &rev, &v, &er, &wv, &we, &ms);
            emit_ms += ms;
            if (!delta_known_fill(&C.known[0], rev, mw, v, er, wv, we)) throw std::runtime_error("gk_table_changes: the device's entries do not fit the host-known reviews");
          }
          std::vector<uint64_t> unanswered = big;
          for (uint32_t r : done) if (r / 64u < words[0]) unanswered[r / 64u] &= ~(1ull << (r % 64u));
          C.extra[0] = delta_known_decide(C.known[0], words[0], C.moved, unanswered);
        }
        if (!delta_prefix(changed, C.drop[0], C.extra[0], &entries, &C.prefix[0])) throw std::runtime_error("gk_table_changes: the index does not fit the host-known reviews");
        // side 1: the snapshot's reviews nothing in the table continues
        C.prefix[1].assign((size_t)words[1] + 1, 0);
        if (then && std::any_of(unmatched.begin(), unmatched.end(), [](uint64_t x) { return x != 0; })) {
          C.aligned[1] = dev_tchg_align(e->opts.device, then->dev, n_then, nullptr, row_of, nullptr, &unmatched, &ms);
          align_ms += ms;
          dev_tchg_index({}, n_then, C.aligned[1], &cnt, &changed, &big, &dev_beyond, &ms);
          index_ms += ms;
          if (changed.size() != words[1]) throw std::runtime_error("dev_tchg_index: wrong size");
          if (!C.known[1].empty()) {
            C.drop[1] = delta_known_words(C.known[1], words[1]);
            C.extra[1] = delta_known_decide(C.known[1], words[1], {}, {});
          }
          if (!delta_prefix(changed, C.drop[1], C.extra[1], &entries, &C.prefix[1])) throw std::runtime_error("gk_table_changes: the index does not fit the host-known reviews");
        }
        if (!delta_next(C.prefix, &side, &word)) side = 2;
        C.gen = t->ts_gen;   // (set last: a stream whose set-up threw answers no later page)
      } else {
        if (C.gen == 0 || C.gen != t->ts_gen || C.prefix[0].size() != (size_t)words[0] + 1) return fail(GK_ERR_INVALID, k_table_stream_moved);
        if (C.snap_serial != (then ? then->serial : 0) || C.n[1] != n_then)
          return fail(GK_ERR_INVALID, "gk_table_changes: a later page must name the snapshot the stream began with");
        if (C.prefix[1].size() != (size_t)words[1] + 1 || !delta_cursor_check(cursor, C.gen, words, &side, &word)) return fail(GK_ERR_INVALID, k_table_stream_moved);
        uint32_t s2 = side, w2 = word;
        if (!delta_next(C.prefix, &s2, &w2) || s2 != side || w2 != word) return fail(GK_ERR_INVALID, k_table_stream_moved);   // (no page begins at a word without entries)
      }
      stream_flags = C.flags;
      beyond = C.beyond;
      total = C.prefix[0].back() + C.prefix[1].back();
      if (side < 2u) {
        page_side = side;
        const uint32_t w0 = word, w1 = viol_page_end(C.prefix[side], w0, max_entries);
        if (C.prefix[side][w1] - C.prefix[side][w0] > 0xFFFFFFFFull) throw std::runtime_error("gk_table_changes: the page does not fit");
        std::vector<uint32_t> rev;
        float ms = 0;
        dev_tchg_entries(side == 0 ? sides : std::vector<TviolSide>(), C.n[side], C.aligned[side], narrow_slice(C.prefix[side], w0, w1), w0, w1, word_slice(C.drop[side], w0, w1),
                         word_slice(C.extra[side], w0, w1), &rev, &h->viol, &h->err, &h->was_viol, &h->was_err, &ms);
        emit_ms += ms;
        if (!delta_merge_page(C.known[side], rev, mw, C.n[side], w0, w1, &h->viol, &h->err, &h->was_viol, &h->was_err))
          throw std::runtime_error("gk_table_changes: the device's entries do not fit the page");
        if (rev.size() != C.prefix[side][w1] - C.prefix[side][w0]) throw std::runtime_error("gk_table_changes: the page's entries do not add up to the stream's index");
        const size_t n = rev.size();
        h->key_text.resize(n); h->flags.assign(n, 0);
        if (side == 0) {
          h->reviews = rev;
          h->was_reviews.resize(n);
          for (size_t i = 0; i < n; i++) {
            const uint32_t r = rev[i], p = C.then_of[r];
            h->was_reviews[i] = p;
            if (p == DELTA_NONE) h->flags[i] |= GK_CHANGE_NEW;
            else if (!C.moved.empty() && ((C.moved[r / 64u] >> (r % 64u)) & 1ull)) h->flags[i] |= GK_CHANGE_VERSION;
            append_key_json(t->obj_key(r), h->key_text[i]);
          }
        } else {
          h->was_reviews = rev;
          h->reviews.assign(n, DELTA_NONE);
          for (size_t i = 0; i < n; i++) { h->flags[i] = GK_CHANGE_GONE; append_key_json(then->key(rev[i]), h->key_text[i]); }
        }
        uint32_t s2 = side, w2 = w1;
        if (delta_next(C.prefix, &s2, &w2)) {
          next_cursor = delta_cursor_pack(C.gen, s2, w2);
          if (!next_cursor) throw std::runtime_error("gk_table_changes: the position does not fit a cursor");
        }
      }
    }
    const uint32_t mw = ((uint32_t)h->ids.size() + 63u) / 64u;
    for (const std::string& k : h->key_text) h->keys.push_back(k.c_str());
    if ((stream_flags & GK_CHANGES_RENDER) && page_side == 0 && !h->reviews.empty()) {
      const size_t n = h->reviews.size();
      std::vector<size_t> todo;   // the entries with a result now
      for (size_t i = 0; i < n; i++) {
        bool any = false;
        for (uint32_t k = 0; k < mw; k++) any = any || h->viol[i * mw + k] || h->err[i * mw + k];
        if (any) todo.push_back(i);
      }
      const std::string first_err = table_render_entries(e, t, h->ids, h->reviews, h->viol, h->err, mw, &todo, &h->result_text);
      if (!first_err.empty()) return fail(GK_ERR_REGO, first_err);
      h->results.assign(n, nullptr);
      for (size_t i : todo) h->results[i] = h->result_text[i].c_str();
    } else if ((stream_flags & GK_CHANGES_RENDER) && !h->was_reviews.empty()) h->results.assign(h->was_reviews.size(), nullptr);
    gk_table_changes_out& p = h->pub;
    memset(&p, 0, sizeof p);
    p.n_reviews = t->n_reviews; p.n_then = then ? then->n_reviews : 0u;
    p.n_constraints = (uint32_t)h->ids.size(); p.mask_words = mw;
    p.constraint_ids = h->ids.data();
    p.reset = then ? 0u : 1u;
    p.total_entries = total;
    p.n_entries = (uint32_t)h->flags.size();
    p.reviews = h->reviews.data(); p.was_reviews = h->was_reviews.data();
    p.keys = h->keys.data();
    p.viol = h->viol.data(); p.err = h->err.data(); p.was_viol = h->was_viol.data(); p.was_err = h->was_err.data();
    p.entry_flags = h->flags.data();
    p.results_json = h->results.empty() ? nullptr : h->results.data();
    p.beyond_limits = beyond;
    p.was_beyond_limits = then ? then->beyond : 0u;
    p.next_cursor = next_cursor;
    p.device_ms = align_ms + index_ms + emit_ms;
    p.align_ms = align_ms; p.index_ms = index_ms; p.emit_ms = emit_ms;
    *out = &h.release()->pub;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_DEVICE, ex.what()); }
}

void gk_table_changes_free(gk_table_changes_out* o) { if (o) delete reinterpret_cast<TableChangesHolder*>(o); }

// Driver.Query's `constraints` as a sorted id list; GK_ERR_NOT_FOUND for an id that is not loaded
static int wanted_ids(gk_engine* e, const uint32_t* ids, size_t n, std::vector<uint32_t>* out) {
  out->assign(ids, ids + n);
  std::sort(out->begin(), out->end());
  out->erase(std::unique(out->begin(), out->end()), out->end());
  std::shared_lock<std::shared_mutex> l(e->mu);
  for (uint32_t id : *out)
    if (id >= e->constraints.size() || !e->constraints[id].alive) return fail(GK_ERR_NOT_FOUND, "unknown constraint template validator: constraint id " + std::to_string(id) + " is not loaded");
  return GK_OK;
}
static int put_string(const std::string& js, char** out) {
  char* buf = (char*)malloc(js.size() + 1);
  if (!buf) return fail(GK_ERR_INTERNAL, "out of memory");
  memcpy(buf, js.c_str(), js.size() + 1);
  *out = buf;
  return GK_OK;
}

int gk_resident_review(gk_engine* e, const char* const* path, size_t npath, char** results_json) { return gk_resident_review_ex(e, path, npath, nullptr, 0, 0, results_json); }

int gk_resident_review_ex(gk_engine* e, const char* const* path, size_t npath, const uint32_t* constraint_ids, size_t n_constraints, uint32_t flags, char** results_json) {
  if (!e || !path || !npath || !results_json) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    std::vector<uint32_t> wanted;
    if (constraint_ids) { int rc = wanted_ids(e, constraint_ids, n_constraints, &wanted); if (rc != GK_OK) return rc; }
    gk_engine::Resident& R = e->resident;
    std::string key;
    for (size_t i = 0; i < npath; i++) { key += path[i]; key.push_back('/'); }
    if (flags & GK_QUERY_PRE_MATCHED) {
      // the sweep kept match AND violation: the caller's own match is answered by evaluating the resident text again, pre-matched
      // (copies: the resident set may change while the batcher works)
      std::string obj, ns;
      bool has_ns = false;
      {
        std::lock_guard<std::mutex> rl(R.mu);
        auto it = R.by_key.find(key);
        if (it == R.by_key.end() || !R.objs[it->second].alive) return fail(GK_ERR_NOT_FOUND, "object is not in the resident set");
        const gk_engine::ResObj& o = R.objs[it->second];
        obj = o.json;
        if (const gk_engine::ResObj* n = resident_namespace_of(R, o)) { has_ns = true; ns = n->json; }
      }
      gk_review_in in;
      memset(&in, 0, sizeof in);
      in.kind = GK_REVIEW_OBJECT; in.source = GK_SRC_EMPTY;
      in.json = obj.data(); in.json_len = obj.size();
      if (has_ns) { in.namespace_json = ns.data(); in.namespace_len = ns.size(); in.ns_object_json = ns.data(); in.ns_object_len = ns.size(); }
      return gk_query_ex2(e, &in, constraint_ids, n_constraints, GK_QUERY_PRE_MATCHED, results_json, nullptr, nullptr);
    }
    std::lock_guard<std::mutex> rl(R.mu);
    auto it = R.by_key.find(key);
    std::string js, err;
    int st = GK_OK;
    if (it == R.by_key.end() || !resident_answer(e, it->second, &js, &st, &err, true, constraint_ids ? &wanted : nullptr))
      return fail(GK_ERR_NOT_FOUND, "object is not in the swept resident set (unknown, changed since the last gk_resident_sweep, or policies / the process excluder changed)");
    if (st != GK_OK) return fail(st, err);
    char* buf = (char*)malloc(js.size() + 1);
    memcpy(buf, js.c_str(), js.size() + 1);
    *results_json = buf;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_REGO, ex.what()); }
}

int gk_batcher_start(gk_engine* e, const gk_batch_opts* opts) {
  if (!e) return fail(GK_ERR_INVALID, "NULL argument");
  gk_engine::Batcher& B = e->batcher;
  {
    std::unique_lock<std::mutex> l(B.mu);
    if (opts) { B.opts = *opts; if (!B.opts.max_batch) B.opts.max_batch = 64; }
    const uint32_t nw = std::max<uint32_t>(1, std::min<uint32_t>(16, B.opts.workers ? B.opts.workers : 2));
    if (B.running && B.workers.size() == nw) return GK_OK;
    if (B.running) { l.unlock(); gk_batcher_stop(e); l.lock(); }   // a different number of workers: restart them
    B.stop = false;
    B.running = true;
    for (uint32_t w = 0; w < nw; w++) B.workers.emplace_back(batcher_loop, e);
  }
  return GK_OK;
}

void gk_batcher_stop(gk_engine* e) {
  if (!e) return;
  gk_engine::Batcher& B = e->batcher;
  {
    std::lock_guard<std::mutex> l(B.mu);
    if (!B.running) return;
    B.stop = true;
  }
  B.cv.notify_all();
  for (auto& w : B.workers) w.join();
  std::lock_guard<std::mutex> l(B.mu);
  B.workers.clear();
  B.running = false;
  B.stop = false;
  for (auto* r : B.queue) { r->status = GK_ERR_INVALID; r->error = "the admission batcher was stopped"; r->done = true; r->cv.notify_one(); }
  B.queue.clear();
}

int gk_query(gk_engine* e, const gk_review_in* review, char** results_json, gk_query_stats* stats) { return gk_query_ex(e, review, 0, results_json, nullptr, stats); }

// the trace of one answered review (QueryResponse.Trace): where and how it was evaluated, what every constraint yielded
static std::string query_trace(gk_engine* e, const char* where, const std::string& results, const gk_query_stats* st, const std::vector<uint32_t>* wanted = nullptr) {
  std::ostringstream os;
  os << "gkgpu trace: evaluated " << where;
  if (st) os << "; batch of " << st->batch_size << " review(s), queued " << (long long)(st->queue_us * 1e3) << " ns, device " << (long long)(st->device_us * 1e3) << " ns";
  os << "\n";
  std::map<uint32_t, std::vector<std::string>> by;
  try {
    Value rows = parse_json(results.data(), results.size());
    if (rows.is_array()) for (const Value& r : rows.items()) {
      const Value* c = r.get("constraint"); const Value* m = r.get("msg"); const Value* ar = r.get("autoreject");
      if (c && c->is_number() && m && m->is_string()) by[(uint32_t)c->i].push_back(std::string(ar ? "autoreject: " : "violation: ") + m->str());
    }
  } catch (const std::exception&) {}
  std::shared_lock<std::shared_mutex> l(e->mu);
  for (const ConstraintRec& c : e->constraints) {
    if (!c.alive || (wanted && !std::binary_search(wanted->begin(), wanted->end(), c.id))) continue;
    os << "  constraint " << c.kind << "/" << c.name << " (id " << c.id << "): ";
    auto it = by.find(c.id);
    if (it == by.end()) { os << (wanted ? "no result\n" : "no result (does not match, or matches and is satisfied)\n"); continue; }
    os << it->second.size() << " result(s)\n";
    for (auto& m : it->second) os << "    " << m << "\n";
  }
  return os.str();
}

int gk_query_ex(gk_engine* e, const gk_review_in* review, uint32_t qflags, char** results_json, char** trace_out, gk_query_stats* stats) {
  return gk_query_ex2(e, review, nullptr, 0, qflags, results_json, trace_out, stats);
}

int gk_query_ex2(gk_engine* e, const gk_review_in* review, const uint32_t* constraint_ids, size_t n_constraints, uint32_t qflags,
                 char** results_json, char** trace_out, gk_query_stats* stats) {
  if (!e || !review || !results_json) return fail(GK_ERR_INVALID, "NULL argument");
  if (trace_out) *trace_out = nullptr;
  const bool pre_matched = (qflags & GK_QUERY_PRE_MATCHED) != 0;
  std::vector<uint32_t> wanted_v;
  const std::vector<uint32_t>* wanted = nullptr;
  if (constraint_ids) {
    int rc = wanted_ids(e, constraint_ids, n_constraints, &wanted_v);
    if (rc != GK_OK) return rc;
    wanted = &wanted_v;
    if (wanted_v.empty()) {   // Driver.Query with no constraints: nothing to evaluate
      if (stats) memset(stats, 0, sizeof *stats);
      return put_string("[]", results_json);
    }
  }
  const bool want_trace = trace_out && ((qflags & GK_QUERY_TRACE) || (e->opts.flags & GK_OPT_TRACE));
  auto put_trace = [&](const char* where, const std::string& js, const gk_query_stats* st) {
    if (!want_trace) return;
    const std::string t = query_trace(e, where, js, st, wanted);
    char* b = (char*)malloc(t.size() + 1);
    memcpy(b, t.c_str(), t.size() + 1);
    *trace_out = b;
  };
  // a review that is byte for byte a swept resident object (same object text, the Namespace the sweep used, no Source --
  // what pkg/audit's auditFromCache sends, manager.go:611-614) is answered from the sweep's bitmap column: no flatten, no launch
  if (!pre_matched && review->kind == GK_REVIEW_OBJECT && review->source == GK_SRC_EMPTY && review->json && !(review->operation && *review->operation)) {
    gk_engine::Resident& R = e->resident;
    std::unique_lock<std::mutex> rl(R.mu, std::try_to_lock);
    if (rl.owns_lock() && R.swept) {
      auto it = R.by_text.find(text_hash(review->json, review->json_len));
      if (it != R.by_text.end()) {
        const gk_engine::ResObj& o = R.objs[it->second];
        const gk_review_in want = resident_review_in(R, o);
        auto same = [](const char* a, size_t an, const char* b, size_t bn) { return (an == 0 && bn == 0) || (a && b && an == bn && memcmp(a, b, an) == 0); };
        if (o.alive && same(o.json.data(), o.json.size(), review->json, review->json_len) &&
            same(want.namespace_json, want.namespace_len, review->namespace_json, review->namespace_len) &&
            same(want.ns_object_json, want.ns_object_len, review->ns_object_json, review->ns_object_len)) {
          std::string js, err;
          int st = GK_OK;
          try {
            if (resident_answer(e, it->second, &js, &st, &err, false, wanted)) {
              if (stats) { stats->batch_size = 0; stats->queue_us = 0; stats->device_us = 0; stats->total_us = 0; }
              if (st != GK_OK) return fail(st, err);
              char* buf = (char*)malloc(js.size() + 1);
              memcpy(buf, js.c_str(), js.size() + 1);
              *results_json = buf;
              put_trace("from the resident sweep's bitmaps (the review is a swept object: no flatten, no launch)", js, nullptr);
              return GK_OK;
            }
          } catch (const std::exception&) { /* fall through to the regular path */ }
        }
      }
    }
  }
  gk_engine::Request req;
  req.in = review;
  req.pre_matched = pre_matched;
  req.arrived = std::chrono::steady_clock::now();
  gk_engine::Batcher& B = e->batcher;
  for (;;) {
    // enqueue only while workers that will serve the queue exist -- decided under the batcher's lock: a request queued
    // between gk_batcher_stop's `stop = true` and the moment the workers have gone would wait for ever
    std::unique_lock<std::mutex> l(B.mu);
    if (B.running && !B.stop) {
      B.queue.push_back(&req);
      B.cv.notify_all();
      req.cv.wait(l, [&] { return req.done; });
      break;
    }
    if (B.stop) return fail(GK_ERR_INVALID, "the admission batcher is shutting down");
    l.unlock();
    int rc = gk_batcher_start(e, nullptr);
    if (rc != GK_OK) return rc;
  }
  // render this review's results from its column of the batch's bitmaps -- in the caller's thread
  std::string results;
  bool on_host = false;
  if (req.status == GK_OK && req.batch) {
    try {
      bool too_big = false;
      for (uint32_t k = 0; k < req.batch->ev->n_host_evaluated; k++) on_host = on_host || req.batch->ev->host_evaluated[k] == req.index;
      results = query_results_json(e, req.batch->table, *req.batch->ev, req.index, *review, &too_big, wanted);
      if (too_big) { req.status = GK_ERR_LIMIT; req.error = "review is beyond the engine's limits (more than 255 elements in an array that constraint predicates iterate, or an object where they iterate array elements)"; }
    } catch (const RegoError& ex) { req.status = GK_ERR_REGO; req.error = ex.what();
    } catch (const std::exception& ex) { req.status = GK_ERR_INTERNAL; req.error = ex.what(); }
    req.batch.reset();
  }
  if (stats) {
    stats->batch_size = req.batch_size;
    stats->queue_us = req.queue_us;
    stats->device_us = req.device_us;
    stats->total_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - req.arrived).count();
  }
  if (req.status != GK_OK) return fail(req.status, req.error);
  char* buf = (char*)malloc(results.size() + 1);
  memcpy(buf, results.c_str(), results.size() + 1);
  *results_json = buf;
  gk_query_stats mine{};
  mine.batch_size = req.batch_size; mine.queue_us = req.queue_us; mine.device_us = req.device_us;
  put_trace(on_host ? (pre_matched ? "by the host evaluator (the review is beyond the device's limits; pre-matched by the caller: violation sets by the concrete evaluator)"
                                   : "by the host evaluator (the review is beyond the device's limits: match layer from the stripped review on the device, violation sets by the concrete evaluator)")
                    : (pre_matched ? "on the device (pre-matched by the caller: violation bitmaps of the batch's one launch; messages rendered by the host evaluator for the flagged pairs)"
                                   : "on the device (match + violation bitmaps of the batch's one launch; messages rendered by the host evaluator for the flagged pairs)"), results, &mine);
  return GK_OK;
}

int gk_debug_set(const char* key, int64_t value) {
  if (!key) return fail(GK_ERR_INVALID, "NULL argument");
  if (strcmp(key, "dict_facts") == 0) { g_debug_dict_facts.store(value != 0); return GK_OK; }
  if (strcmp(key, "group_max") == 0) { g_debug_group_max.store((int)std::max<int64_t>(0, std::min<int64_t>(value, 1 << 20))); return GK_OK; }
  if (strcmp(key, "verify_flip") == 0) { g_debug_verify_flip.store(value < 0 ? -1 : value); return GK_OK; }
  if (strcmp(key, "kjoin_hash_bits") == 0) { g_debug_kjoin_hash_bits.store(value < 0 || value > 64 ? 64u : (uint32_t)value); return GK_OK; }
  if (strcmp(key, "fold_match_labels") == 0) { g_test_fold_match_labels.store(value != 0); return GK_OK; }
  if (strcmp(key, "keep_slot_index") == 0) { g_debug_keep_slot_index.store(value != 0); return GK_OK; }
  return fail(GK_ERR_NOT_FOUND, std::string("gk_debug_set: unknown key ") + key);
}

void gk_jit_quiesce(void) { dev_jit_quiesce(); }
void gk_jit_cache_drop_memory(void) { dev_jit_cache_drop_memory(); }
const char* gk_jit_cache_dir(void) { return dev_jit_cache_dir(); }
void gk_jit_cache_stats(uint64_t* cache_hits, uint64_t* compiles) {
  uint64_t h = 0, c = 0;
  dev_jit_cache_stats(&h, &c);
  if (cache_hits) *cache_hits = h;
  if (compiles) *compiles = c;
}

// Debug: what binding the primary plan to this table with review words does (review_words.hpp), computed on the host from the plan and
// the table's slot index exactly as kernels.hip bind_chunks / bind_review_words compute it: one "key=value" per line.
int gk_table_review_words(gk_engine* e, const gk_table* t, char** text_out) {
  if (!e || !t || !text_out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    ensure_plan(e);
    std::shared_lock<std::shared_mutex> l(e->plan_rw);
    const HostPlan& p = e->groups[0]->fast;
    const HostTable& h = t->host;
    const uint32_t n_groups = h.n_tiles(), S = h.n_slots();
    if (h.tile_idx.size() != (size_t)n_groups * (S + 1u)) return fail(GK_ERR_INVALID, "the table did not keep its slot index: gk_debug_set(\"keep_slot_index\", 1) before it is created");
    std::vector<std::vector<Pred>> classes;
    const std::vector<uint32_t> cls = jit_path_classes(p, &classes);
    const ReviewWords rw = analyse_review_words(classes, p.dims.n_gwords);
    std::vector<BoundPath> bound, kept, hoisted;
    for (uint32_t s = 0; s < S; s++) {
      const uint32_t path = h.slot_path[s];
      if (path >= cls.size() || !cls[path]) continue;
      const uint32_t ent = p.ptab[path];
      bound.push_back(BoundPath{s, cls[path], pred_list_cost<Pred>(&p.path_preds[ent >> 8], ent & 0xFF, [](const Pred& q) { return pred_needs_str(q); })});
    }
    split_bound(bound, rw, &kept, &hoisted);
    const int block = gk_block_of((int)h.rpt);
    const uint32_t list_cap = (uint32_t)std::min(block / GK_TILE, 8) * GK_WAVE_CHUNKS, n_waves = (uint32_t)(block / GK_TILE);
    const ChunkLists full = build_chunk_lists(h.tile_idx.data(), n_groups, S, bound, list_cap, n_waves);
    const ChunkLists part = build_chunk_lists(h.tile_idx.data(), n_groups, S, kept, list_cap, n_waves);
    // groups that hold rows of hoisted paths only: their filtered list must be a valid list of zero chunks
    uint32_t only = 0, only_ok = 0;
    for (uint32_t g = 0; g < n_groups; g++) {
      const uint32_t* ix = h.tile_idx.data() + (size_t)g * (S + 1u);
      bool any_h = false, any_k = false;
      for (const BoundPath& b : hoisted) any_h = any_h || ix[b.slot + 1u] > ix[b.slot];
      for (const BoundPath& b : kept) any_k = any_k || ix[b.slot + 1u] > ix[b.slot];
      if (!any_h || any_k) continue;
      only++;
      const ChunkDesc& hd = part.d[(size_t)g * part.capg];
      if (hd.st == 0u && hd.info == 0u) only_ok++;
    }
    uint32_t n_hoisted_classes = 0;
    for (size_t c = 1; c < rw.hoisted.size(); c++) n_hoisted_classes += rw.hoisted[c] ? 1u : 0u;
    std::ostringstream os;
    os << "n_gwords=" << p.dims.n_gwords << "\nclasses=" << (classes.size() ? classes.size() - 1 : 0) << "\nhoisted_classes=" << n_hoisted_classes << "\nk=" << rw.k() << "\nwords=";
    for (uint32_t k = 0; k < rw.k(); k++) os << (k ? "," : "") << rw.words[k];
    os << "\nrpt=" << h.rpt << "\ngroups=" << n_groups << "\nbound_paths=" << bound.size() << "\nkept_paths=" << kept.size() << "\nhoisted_paths=" << hoisted.size()
       << "\nchunks_full=" << full.n_chunks << "\nchunks_kept=" << part.n_chunks << "\ncapg_full=" << full.capg << "\ncapg_kept=" << part.capg
       << "\noverflow_groups_full=" << full.n_overflow_groups << "\noverflow_groups_kept=" << part.n_overflow_groups
       << "\ngroups_only_hoisted=" << only << "\ngroups_only_hoisted_with_empty_list=" << only_ok << "\n";
    const std::string s = os.str();
    char* buf = (char*)malloc(s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    *text_out = buf;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_INTERNAL, ex.what()); }
}

int gk_dump(gk_engine* e, char** text_out) {
  if (!e || !text_out) return fail(GK_ERR_INVALID, "NULL argument");
  try {
    ensure_plan(e);
    std::ostringstream os;
    std::shared_lock<std::shared_mutex> l(e->plan_rw);
    const HostPlan& p = e->groups[0]->fast;
    os << "constraints=" << p.dims.n_constraints << " viol_formulas=" << p.n_viol << " match_formulas=" << p.n_match
       << " preds=" << p.dims.n_preds << " scopes=" << p.dims.n_scopes << " code_words=" << p.dims.n_code
       << " gwords=" << p.dims.n_gwords << " acc_words=" << p.dims.acc_words << " lds_bytes_per_64_reviews=" << p.dims.acc_words * 256
       << " paths=" << p.dims.n_paths << "\n";
    for (size_t i = 0; i < p.preds.size(); i++)
      os << "pred " << i << " op=" << (int)p.preds[i].op << " dst=" << (int)p.preds[i].dst << " scope=" << (int)p.preds[i].scope
         << " bit=" << p.preds[i].bit << " " << pattern_to_string(p.pred_patterns[i]) << "\n";
    {
      std::shared_lock<std::shared_mutex> rl(e->mu);
      for (auto& c : e->constraints) if (c.alive) os << "constraint " << c.id << " " << c.kind << "/" << c.name << " viol: " << f_to_string(c.viol) << "\n";
    }
    // value expressions (flatten.hpp DictRegistry::add_vexpr): "<leaf pattern> $v<id> = <expression>[ ordered]", one line each
    if (e->dict_reg.has_vexprs()) os << "value expressions:\n" << e->dict_reg.dump_vexprs();
    std::string s = os.str();
    char* buf = (char*)malloc(s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    *text_out = buf;
    return GK_OK;
  } catch (const std::exception& ex) { return fail(GK_ERR_INTERNAL, ex.what()); }
}

}  // extern "C"
