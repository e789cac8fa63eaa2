// The cache of compiled plan kernels (host only: no HIP, no other header of the project).  The text handed to the compiler is a pure
// function of (plan, geometry, table statistics) (jit_source.hpp); identical text -- the same constraints loaded again, another engine
// with the same policies, a variant rebuilt after an unrelated change -- reuses the code object: in memory for the life of the process,
// and on disk under cache_dir() (a restarted pod then loads its kernels instead of compiling them).
//
// One entry point, code_cache_get(text, compiler version, compile): kernels.hip (jit_compile) hands it the compiler as a function, and
// tests/native/code_cache_test.cpp a stub -- directory rule, file name, header, refusal of wrong files, LRU, the in-flight set and the
// compile slots are tested on a CPU (tests/test_code_cache.py).  File name and header decide whether the caches already on users'
// disks stay valid: they do not change without a reason.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace gk {

// FNV-1a with the PROJECT's offset basis, 1469598103934665603: one digit short of the textbook 14695981039346656037.  It is in the
// name of every cached file (and in JitKernel::source_hash), so it stays: fnv64("abc") == 0xe16801510db89efd, where the standard
// FNV-1a gives 0xe71fa2190541574b.
inline uint64_t fnv64(const std::string& s) { uint64_t h = 1469598103934665603ull; for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; } return h; }

using CodeKey = std::pair<uint64_t, size_t>;   // (hash, length) of the source
using CodeObject = std::shared_ptr<const std::vector<char>>;
struct CodeCache {
  std::mutex mu;
  std::map<CodeKey, CodeObject> mem;
  std::list<CodeKey> order;
  std::atomic<uint64_t> hits{0}, compiles{0}, disk_hits{0};
  CodeObject find(const CodeKey& key) {   // counts the hit
    std::lock_guard<std::mutex> l(mu);
    auto it = mem.find(key);
    if (it == mem.end()) return nullptr;
    hits++;
    return it->second;
  }
  void insert(const CodeKey& key, const CodeObject& code) {   // the 64 most recently ADDED texts stay
    std::lock_guard<std::mutex> l(mu);
    if (mem.emplace(key, code).second) { order.push_back(key); if (order.size() > 64) { mem.erase(order.front()); order.pop_front(); } }
  }
};
inline CodeCache& code_cache() { static CodeCache c; return c; }

// The disk cache is ON by default: $GK_JIT_CACHE_DIR, else $XDG_CACHE_HOME/gkgpu-jit, else $HOME/.cache/gkgpu-jit, else
// /tmp/gkgpu-jit-<uid>; GK_JIT_CACHE_DIR="", "off" or "0" switches it off.  A file is named by the hash and length of the SOURCE TEXT
// (which holds the whole kernel: plan.hpp, vm_core.hpp, the generated plan code, kernel_body.inc and every tuning define), the
// target (gfx950) and the version of the compiler that made it -- another compiler never loads this one's code objects.
inline std::string cache_dir() {   // (resolved again when the environment changes: the tests point it at a directory of their own)
  static std::mutex mu;
  static std::string asked = "\x01", resolved;
  std::string d;
  bool off = false;
  if (const char* v = getenv("GK_JIT_CACHE_DIR")) { if (!*v || strcmp(v, "off") == 0 || strcmp(v, "0") == 0) off = true; else d = v; }
  else if (const char* x = getenv("XDG_CACHE_HOME"); x && *x) d = std::string(x) + "/gkgpu-jit";
  else if (const char* h = getenv("HOME"); h && *h && strcmp(h, "/") != 0) d = std::string(h) + "/.cache/gkgpu-jit";
  else d = "/tmp/gkgpu-jit-" + std::to_string((unsigned long long)getuid());
  std::lock_guard<std::mutex> l(mu);
  if (d == asked) return resolved;
  asked = d;
  resolved.clear();
  if (off) return resolved;
  // mkdir -p; a directory that cannot be made or written simply means no disk cache
  for (size_t i = 1; i <= d.size(); i++) if (i == d.size() || d[i] == '/') { const std::string part = d.substr(0, i); if (mkdir(part.c_str(), 0700) != 0 && errno != EEXIST) break; }
  // The code objects in there decide admission results: the directory must be OURS -- a real directory (no symbolic link), owned by
  // this user, writable by nobody else.  Anything else (a directory somebody pre-created under /tmp, a shared cache with group write)
  // means no disk cache, said once on stderr.
  struct stat st;
  if (lstat(d.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || st.st_uid != geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH)) != 0) {
    if (lstat(d.c_str(), &st) == 0) fprintf(stderr, "[gkgpu] code-object cache %s is not a private directory of uid %u (owner %u, mode %o): disk cache off\n", d.c_str(), (unsigned)geteuid(), (unsigned)st.st_uid, (unsigned)(st.st_mode & 07777));
    return resolved;
  }
  if (access(d.c_str(), W_OK | X_OK) == 0) resolved = d;
  return resolved;
}
// the one place the key of a cached file is put together ("" = no disk cache)
inline std::string cache_file(int compiler_version, uint64_t h, size_t n) {
  const std::string dir = cache_dir();
  if (dir.empty()) return "";
  char name[96];
  snprintf(name, sizeof name, "/gk_gfx950_rtc%d_%016llx_%zu.co", compiler_version, (unsigned long long)h, n);
  return dir + name;
}

// ---- SHA-256 of the source text: a cached file names the text it was compiled from by a strong digest, checked on load (the file
// name's FNV-64 is a look-up key, not an identity)
struct Sha256 {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const unsigned char* p) {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu,
        0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u,
        0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu,
        0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[64];
    for (int i = 0; i < 16; i++) w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
    for (int i = 16; i < 64; i++) w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  static std::array<unsigned char, 32> of(const std::string& s) {
    Sha256 c;
    size_t i = 0;
    for (; i + 64 <= s.size(); i += 64) c.block(reinterpret_cast<const unsigned char*>(s.data()) + i);
    unsigned char tail[128] = {0};
    const size_t rem = s.size() - i;
    memcpy(tail, s.data() + i, rem);
    tail[rem] = 0x80;
    const size_t tl = rem + 9 <= 64 ? 64 : 128;
    const uint64_t bits = (uint64_t)s.size() * 8;
    for (int k = 0; k < 8; k++) tail[tl - 1 - k] = (unsigned char)(bits >> (8 * k));
    c.block(tail);
    if (tl == 128) c.block(tail + 64);
    std::array<unsigned char, 32> out;
    for (int k = 0; k < 8; k++) { out[4 * k] = (unsigned char)(c.h[k] >> 24); out[4 * k + 1] = (unsigned char)(c.h[k] >> 16); out[4 * k + 2] = (unsigned char)(c.h[k] >> 8); out[4 * k + 3] = (unsigned char)c.h[k]; }
    return out;
  }
};
// a cached file: [8 bytes "GKCO\x01\0\0\0"][u64 length of the source][32 bytes SHA-256 of the source][the code object]
constexpr size_t CACHE_HDR = 48;
inline void cache_header(const std::string& src, char* hdr) {
  memcpy(hdr, "GKCO\x01\0\0\0", 8);
  const uint64_t sl = src.size();
  memcpy(hdr + 8, &sl, 8);
  const auto dg = Sha256::of(src);
  memcpy(hdr + 16, dg.data(), 32);
}
inline bool read_whole(const std::string& path, std::vector<char>* buf) {   // O_NOFOLLOW: a planted symbolic link is not followed
  const int fd = open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
  if (fd < 0) return false;
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_uid != geteuid()) { close(fd); return false; }
  char tmp[65536];
  ssize_t n;
  while ((n = read(fd, tmp, sizeof tmp)) > 0) buf->insert(buf->end(), tmp, tmp + n);
  close(fd);
  return n == 0;
}
inline bool write_new(const std::string& path, const void* a, size_t an, const void* b, size_t bn) {   // O_EXCL | O_NOFOLLOW: never through somebody else's file or link
  const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
  if (fd < 0) return false;
  auto put = [&](const void* p, size_t n) { const char* c = (const char*)p; while (n) { const ssize_t w = write(fd, c, n); if (w <= 0) return false; c += w; n -= (size_t)w; } return true; };
  const bool ok = put(a, an) && put(b, bn);
  close(fd);
  if (!ok) unlink(path.c_str());
  return ok;
}

// Compiles of DIFFERENT programs run concurrently (measured in the build container: the four plan groups of the 200-template
// corpus 7.7 s side by side against 23 s one after the other); at most `cap` at once -- code_cache_set_compile_slots, one until then
struct CompileSlots {
  std::mutex mu; std::condition_variable cv; size_t cap = 1, used = 0;
  void acquire() { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return used < cap; }); used++; }
  void release() { { std::lock_guard<std::mutex> l(mu); used--; } cv.notify_one(); }
};
// the same text compiled by one thread at a time: the others wait for its code object instead of compiling it again
struct InFlight { std::mutex mu; std::condition_variable cv; std::set<CodeKey> keys; };
// (both never destroyed: a background build may still hold a slot or a key when exit() destroys the statics -- see quiesce_at_exit,
//  kernels.hip)
inline CompileSlots& compile_slots() { static CompileSlots* s = new CompileSlots(); return *s; }
inline InFlight& in_flight() { static InFlight* f = new InFlight(); return *f; }
inline void code_cache_set_compile_slots(size_t n) {
  CompileSlots& s = compile_slots();
  { std::lock_guard<std::mutex> l(s.mu); s.cap = std::max<size_t>(1, n); }
  s.cv.notify_all();
}

// The code object of `src`: from memory, else from the file (ignored unless it is ours, regular, names THIS text by its SHA-256 and
// holds an ELF image), else from compile(src) -- which runs in one thread per text and in at most `cap` threads at once, and whose
// exception reaches the caller with the text's in-flight key and the slot released.
inline CodeObject code_cache_get(const std::string& src, int compiler_version, const std::function<std::vector<char>(const std::string&)>& compile) {
  CodeCache& C = code_cache();
  const CodeKey key(fnv64(src), src.size());
  if (CodeObject hit = C.find(key)) return hit;
  const std::string file = cache_file(compiler_version, key.first, key.second);
  char hdr[CACHE_HDR];
  if (!file.empty()) {
    cache_header(src, hdr);
    std::vector<char> buf;
    if (read_whole(file, &buf) && buf.size() > CACHE_HDR + 64 && memcmp(buf.data(), hdr, CACHE_HDR) == 0 && memcmp(buf.data() + CACHE_HDR, "\x7f" "ELF", 4) == 0) {
      C.disk_hits++;
      const CodeObject code = std::make_shared<const std::vector<char>>(buf.begin() + CACHE_HDR, buf.end());
      C.insert(key, code);
      return code;
    }
  }
  InFlight& F = in_flight();
  {   // (several plans with the same text: one compiles, the others take its code object)
    std::unique_lock<std::mutex> fl(F.mu);
    F.cv.wait(fl, [&] { return !F.keys.count(key); });
    if (CodeObject hit = C.find(key)) return hit;
    F.keys.insert(key);
  }
  struct Done { InFlight& F; const CodeKey& k; ~Done() { { std::lock_guard<std::mutex> l(F.mu); F.keys.erase(k); } F.cv.notify_all(); } } done{F, key};
  compile_slots().acquire();
  struct Rel { ~Rel() { compile_slots().release(); } } rel;
  const CodeObject code = std::make_shared<const std::vector<char>>(compile(src));
  C.compiles++;
  C.insert(key, code);   // (before the in-flight key is released)
  if (!file.empty()) {   // write-then-rename: a reader never sees half a file
    const std::string tmp = file + ".tmp" + std::to_string((long long)getpid()) + "_" + std::to_string((unsigned long long)(uintptr_t)code.get());
    unlink(tmp.c_str());
    if (write_new(tmp, hdr, CACHE_HDR, code->data(), code->size())) { if (rename(tmp.c_str(), file.c_str()) != 0) unlink(tmp.c_str()); }
  }
  return code;
}

inline void code_cache_stats(uint64_t* hits, uint64_t* compiles) { *hits = code_cache().hits.load() + code_cache().disk_hits.load(); *compiles = code_cache().compiles.load(); }
// forget the code objects held in memory (the disk cache stays): the next build of a known text is served the way a restarted
// process would be -- from the file
inline void code_cache_drop_memory() { CodeCache& C = code_cache(); std::lock_guard<std::mutex> l(C.mu); C.mem.clear(); C.order.clear(); }
inline const char* code_cache_dir() { static thread_local std::string d; d = cache_dir(); return d.c_str(); }   // "" = no disk cache

}  // namespace gk
