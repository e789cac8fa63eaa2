// TEST-ONLY stand-alone program over csrc/code_cache.hpp with a stub in place of the compiler (tests/test_code_cache.py builds and
// runs it, plain and under the sanitizers).  It works in the CURRENT directory, prints `ok <case>` or `FAIL <case>: ...` per case and
// exits non-zero on any failure.  What it leaves for the Python side, which knows the digests from hashlib:
//   `sha256 <length> <hex>` lines for sha_text(length), `fnv64 abc <hex>`, and the file of the cold-then-warm case under cw/.
// Not made here: a directory or a file of ANOTHER owner (st_uid != geteuid(), cache_dir and read_whole) needs a second user, and the
// access(W_OK | X_OK) test of cache_dir says yes to uid 0 whatever the mode -- those two branches are left to reading.
#include "code_cache.hpp"

#include <dirent.h>

#include <chrono>
#include <stdexcept>
#include <thread>

using namespace gk;

namespace {
const int RTC = 7002;   // the "compiler version" of the stub
std::string cwd;

struct Fail : std::runtime_error { using std::runtime_error::runtime_error; };
#define REQUIRE(c)                                                                         \
  do {                                                                                     \
    if (!(c)) throw Fail(std::string(#c) + " (line " + std::to_string(__LINE__) + ")");   \
  } while (0)

// ---- the stub compiler
std::atomic<int> g_calls{0}, g_now{0}, g_most{0}, g_throws{0}, g_sleep_ms{0};
std::vector<char> payload(const std::string& src) {   // "\x7fELF" + the text's FNV as 16 hex digits, six times: 100 bytes
  char hex[17];
  snprintf(hex, sizeof hex, "%016llx", (unsigned long long)fnv64(src));
  std::string s = "\x7f" "ELF";
  for (int i = 0; i < 6; i++) s += hex;
  return std::vector<char>(s.begin(), s.end());
}
std::vector<char> stub(const std::string& src) {
  g_calls++;
  const int now = ++g_now;
  int most = g_most.load();
  while (now > most && !g_most.compare_exchange_weak(most, now)) {}
  if (g_sleep_ms.load()) std::this_thread::sleep_for(std::chrono::milliseconds(g_sleep_ms.load()));
  g_now--;
  int t = g_throws.load();
  while (t > 0 && !g_throws.compare_exchange_weak(t, t - 1)) {}
  if (t > 0) throw std::runtime_error("stub compiler: no");
  return payload(src);
}
CodeObject get(const std::string& src) { return code_cache_get(src, RTC, stub); }

struct Stats { uint64_t hits, compiles; int calls; };
Stats stats() { Stats s; code_cache_stats(&s.hits, &s.compiles); s.calls = g_calls.load(); return s; }

// ---- files
std::string sha_text(size_t n) { std::string s(n, 0); for (size_t i = 0; i < n; i++) s[i] = (char)('a' + i % 26); return s; }
std::string hex(const unsigned char* p, size_t n) { std::string s; char b[3]; for (size_t i = 0; i < n; i++) { snprintf(b, sizeof b, "%02x", p[i]); s += b; } return s; }
bool slurp(const std::string& path, std::string* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char tmp[4096];
  size_t n;
  out->clear();
  while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) out->append(tmp, n);
  fclose(f);
  return true;
}
void spit(const std::string& path, const std::string& bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) throw Fail("cannot write " + path);
  fclose(f);
}
std::string header_of(const std::string& src) {   // written out here, not taken from cache_header: the layout is pinned
  std::string h("GKCO\x01\0\0\0", 8);
  const uint64_t n = src.size();
  h.append(reinterpret_cast<const char*>(&n), 8);
  const auto dg = Sha256::of(src);
  h.append(reinterpret_cast<const char*>(dg.data()), 32);
  return h;
}
std::string good_file(const std::string& src) { const auto p = payload(src); return header_of(src) + std::string(p.begin(), p.end()); }
std::string name_of(const std::string& src) {
  char name[96];
  snprintf(name, sizeof name, "gk_gfx950_rtc%d_%016llx_%zu.co", RTC, (unsigned long long)fnv64(src), src.size());
  return name;
}
std::vector<std::string> list_dir(const std::string& dir) {
  std::vector<std::string> v;
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d)) if (strcmp(e->d_name, ".") != 0 && strcmp(e->d_name, "..") != 0) v.push_back(e->d_name);
    closedir(d);
  }
  return v;
}
unsigned mode_of(const std::string& path) { struct stat st; return lstat(path.c_str(), &st) == 0 ? (unsigned)(st.st_mode & 07777) : ~0u; }
bool is_regular(const std::string& path) { struct stat st; return lstat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode); }
void use_dir(const char* value) {   // nullptr: GK_JIT_CACHE_DIR unset
  if (value) setenv("GK_JIT_CACHE_DIR", value, 1); else unsetenv("GK_JIT_CACHE_DIR");
}
bool same(const CodeObject& c, const std::string& src) { return c && *c == payload(src); }

// ---- the cases
void sha256_and_fnv() {
  for (size_t n : {0, 3, 55, 56, 63, 64, 119, 120, 1000}) {
    const auto dg = Sha256::of(sha_text(n));
    printf("sha256 %zu %s\n", n, hex(dg.data(), 32).c_str());
  }
  REQUIRE(hex(Sha256::of("").data(), 32) == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855");
  REQUIRE(hex(Sha256::of("abc").data(), 32) == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
  printf("fnv64 abc %016llx\n", (unsigned long long)fnv64("abc"));
  REQUIRE(fnv64("abc") == 0xe16801510db89efdull);   // the project's offset basis, not the textbook one (0xe71fa2190541574b)
}

void cold_then_warm() {
  const std::string dir = cwd + "/cw", src = "cold, then warm";
  use_dir(dir.c_str());
  const Stats s0 = stats();
  const CodeObject a = get(src);
  const Stats s1 = stats();
  REQUIRE(same(a, src) && s1.calls == s0.calls + 1 && s1.compiles == s0.compiles + 1 && s1.hits == s0.hits);
  REQUIRE(list_dir(dir) == std::vector<std::string>{name_of(src)});
  std::string bytes;
  REQUIRE(slurp(dir + "/" + name_of(src), &bytes) && bytes.size() == CACHE_HDR + 100);
  REQUIRE(bytes.substr(0, 48) == header_of(src));
  REQUIRE(bytes.substr(48) == std::string(a->begin(), a->end()));
  REQUIRE(mode_of(dir + "/" + name_of(src)) == 0600);
  const CodeObject b = get(src);   // memory
  const Stats s2 = stats();
  REQUIRE(b == a && s2.calls == s1.calls && s2.compiles == s1.compiles && s2.hits == s1.hits + 1);
  code_cache_drop_memory();
  const CodeObject c = get(src);   // the file
  const Stats s3 = stats();
  REQUIRE(c != a && *c == *a && s3.calls == s1.calls && s3.compiles == s1.compiles && s3.hits == s2.hits + 1);
  REQUIRE(get(src) == c && stats().hits == s3.hits + 1);   // a disk hit is kept in memory
}

// a wrong file under the right name is never trusted: the stub runs, and the good file takes its place
void wrong_file(const std::string& kind) {
  const std::string dir = cwd + "/wrong", src = "text behind a wrong file: " + kind, file = dir + "/" + name_of(src);
  use_dir(dir.c_str());
  REQUIRE(code_cache_dir() == dir);
  const std::string other = good_file(std::string(src.size(), 'x')), elsewhere = cwd + "/elsewhere_" + kind;
  std::string planted = header_of(src) + "\x7f" "ELF" + std::string(96, 'Z');   // right in every respect, but not what the stub makes
  if (kind == "other_text") spit(file, other);   // the same length (and, by its name, the same FNV), another SHA-256
  else if (kind == "truncated") spit(file, good_file(src).substr(0, 20));
  else if (kind == "no_elf") spit(file, header_of(src) + "XELF" + std::string(96, 'Z'));
  else if (kind == "symlink") { spit(elsewhere, planted); REQUIRE(symlink(elsewhere.c_str(), file.c_str()) == 0); }
  else throw Fail("unknown kind");
  const Stats s0 = stats();
  const CodeObject a = get(src);
  const Stats s1 = stats();
  REQUIRE(same(a, src) && s1.calls == s0.calls + 1 && s1.compiles == s0.compiles + 1 && s1.hits == s0.hits);
  std::string bytes;
  REQUIRE(is_regular(file) && slurp(file, &bytes) && bytes == good_file(src));
  if (kind == "symlink") REQUIRE(is_regular(elsewhere) && slurp(elsewhere, &bytes) && bytes == planted);   // not followed, not written through
  code_cache_drop_memory();
  REQUIRE(same(get(src), src) && stats().calls == s1.calls);   // and the good file is served
}

bool private_dir(const std::string& d) {
  struct stat st;
  return lstat(d.c_str(), &st) == 0 && S_ISDIR(st.st_mode) && st.st_uid == geteuid() && !(st.st_mode & (S_IWGRP | S_IWOTH)) && access(d.c_str(), W_OK | X_OK) == 0;
}
void directory_rule() {
  // 1. GK_JIT_CACHE_DIR
  use_dir((cwd + "/d1").c_str());
  setenv("XDG_CACHE_HOME", (cwd + "/xdg").c_str(), 1);
  setenv("HOME", (cwd + "/home").c_str(), 1);
  REQUIRE(code_cache_dir() == cwd + "/d1" && mode_of(cwd + "/d1") == 0700);
  // ... and its three ways to say no: nothing is written anywhere, the compiler's result is returned all the same
  for (const char* off : {"", "off", "0"}) {
    use_dir(off);
    REQUIRE(code_cache_dir() == std::string());
    const Stats s0 = stats();
    const std::string src = std::string("disk cache off: '") + off + "'";
    REQUIRE(same(get(src), src) && stats().calls == s0.calls + 1);
    REQUIRE(list_dir(cwd + "/d1").empty() && list_dir(cwd + "/xdg").empty() && list_dir(cwd + "/home").empty());
  }
  // 2. $XDG_CACHE_HOME/gkgpu-jit
  use_dir(nullptr);
  REQUIRE(code_cache_dir() == cwd + "/xdg/gkgpu-jit" && mode_of(cwd + "/xdg/gkgpu-jit") == 0700);
  // 3. $HOME/.cache/gkgpu-jit (an empty XDG_CACHE_HOME counts as none)
  setenv("XDG_CACHE_HOME", "", 1);
  REQUIRE(code_cache_dir() == cwd + "/home/.cache/gkgpu-jit");
  unsetenv("XDG_CACHE_HOME");
  REQUIRE(code_cache_dir() == cwd + "/home/.cache/gkgpu-jit" && mode_of(cwd + "/home/.cache") == 0700);
  // 4. /tmp/gkgpu-jit-<uid>, for HOME=/ and for no HOME.  /tmp is not this test's: the directory may be there already and need not be
  //    ours, so the expectation follows what is found (and a directory made here goes again)
  const std::string tmp = "/tmp/gkgpu-jit-" + std::to_string((unsigned long long)getuid());
  struct stat st;
  const bool was_there = lstat(tmp.c_str(), &st) == 0;
  setenv("HOME", "/", 1);
  const std::string got_root = code_cache_dir();
  REQUIRE(got_root == (private_dir(tmp) ? tmp : std::string()));
  unsetenv("HOME");
  use_dir("off");   // (asked again: the answer above is remembered per directory asked for)
  REQUIRE(code_cache_dir() == std::string());
  use_dir(nullptr);
  REQUIRE(code_cache_dir() == got_root);
  if (!was_there) rmdir(tmp.c_str());
  setenv("HOME", (cwd + "/home").c_str(), 1);
  // refused, one line on stderr each (counted by the Python side): group write, a symbolic link to a good directory, a file
  REQUIRE(mkdir((cwd + "/shared").c_str(), 0700) == 0 && chmod((cwd + "/shared").c_str(), 0770) == 0);
  use_dir((cwd + "/shared").c_str());
  REQUIRE(code_cache_dir() == std::string());
  const Stats s0 = stats();
  REQUIRE(same(get("into a shared directory"), "into a shared directory") && stats().calls == s0.calls + 1 && list_dir(cwd + "/shared").empty());
  REQUIRE(mkdir((cwd + "/real").c_str(), 0700) == 0 && symlink((cwd + "/real").c_str(), (cwd + "/link").c_str()) == 0);
  use_dir((cwd + "/link").c_str());
  REQUIRE(code_cache_dir() == std::string());
  REQUIRE(same(get("through a link"), "through a link") && list_dir(cwd + "/real").empty());
  spit(cwd + "/plainfile", "not a directory");
  use_dir((cwd + "/plainfile").c_str());
  REQUIRE(code_cache_dir() == std::string());
  // a path whose parents do not exist: made, all of it private
  use_dir((cwd + "/deep/er/still").c_str());
  REQUIRE(code_cache_dir() == cwd + "/deep/er/still");
  REQUIRE(mode_of(cwd + "/deep") == 0700 && mode_of(cwd + "/deep/er") == 0700 && mode_of(cwd + "/deep/er/still") == 0700);
  // the variable changes between two requests: the next request uses the new directory
  const std::string src = "one text, two directories";
  use_dir((cwd + "/s1").c_str());
  REQUIRE(same(get(src), src) && list_dir(cwd + "/s1") == std::vector<std::string>{name_of(src)});
  use_dir((cwd + "/s2").c_str());
  code_cache_drop_memory();
  const Stats s1 = stats();
  REQUIRE(same(get(src), src) && stats().calls == s1.calls + 1 && list_dir(cwd + "/s2") == std::vector<std::string>{name_of(src)});
}

void lru() {
  use_dir("off");
  code_cache_drop_memory();
  const Stats s0 = stats();
  for (int i = 1; i <= 65; i++) REQUIRE(same(get("lru " + std::to_string(i)), "lru " + std::to_string(i)));
  REQUIRE(stats().calls == s0.calls + 65 && stats().hits == s0.hits);
  get("lru 65");
  REQUIRE(stats().calls == s0.calls + 65 && stats().hits == s0.hits + 1);   // the 65th is held
  get("lru 2");
  REQUIRE(stats().calls == s0.calls + 65 && stats().hits == s0.hits + 2);   // ... as is the second
  get("lru 1");
  REQUIRE(stats().calls == s0.calls + 66 && stats().compiles == s0.compiles + 66);   // the first went when the 65th came
}

void same_text_from_8_threads() {
  use_dir((cwd + "/mt").c_str());
  code_cache_set_compile_slots(8);
  g_sleep_ms = 50;
  const std::string src = "one text, eight threads";
  const Stats s0 = stats();
  std::vector<CodeObject> got(8);
  std::vector<std::thread> th;
  for (int i = 0; i < 8; i++) th.emplace_back([&, i] { got[i] = get(src); });
  for (auto& t : th) t.join();
  g_sleep_ms = 0;
  const Stats s1 = stats();
  REQUIRE(s1.calls == s0.calls + 1 && s1.compiles == s0.compiles + 1 && s1.hits == s0.hits + 7);
  for (int i = 0; i < 8; i++) REQUIRE(same(got[i], src));
}

void two_slots_16_threads() {
  use_dir((cwd + "/mt").c_str());
  code_cache_set_compile_slots(2);
  g_sleep_ms = 20;
  g_most = 0;
  const Stats s0 = stats();
  std::vector<CodeObject> got(16);
  std::vector<std::thread> th;
  for (int i = 0; i < 16; i++) th.emplace_back([&, i] { got[i] = get("slots " + std::to_string(i)); });
  for (auto& t : th) t.join();
  g_sleep_ms = 0;
  REQUIRE(stats().calls == s0.calls + 16 && stats().compiles == s0.compiles + 16);
  REQUIRE(g_most.load() >= 1 && g_most.load() <= 2);
  for (int i = 0; i < 16; i++) REQUIRE(same(got[i], "slots " + std::to_string(i)));
  REQUIRE(list_dir(cwd + "/mt").size() == 17);   // these and the one of the eight threads; no temporary file stays
}

void stub_throws() {
  use_dir((cwd + "/mt").c_str());
  code_cache_set_compile_slots(1);   // (a slot that is not given back would stop the second request for good)
  const std::string src = "a text the compiler refuses once";
  const Stats s0 = stats();
  g_throws = 1;
  std::string what;
  try { get(src); } catch (const std::runtime_error& ex) { what = ex.what(); }
  REQUIRE(what == "stub compiler: no");
  REQUIRE(stats().calls == s0.calls + 1 && stats().compiles == s0.compiles);
  REQUIRE(same(get(src), src));
  REQUIRE(stats().calls == s0.calls + 2 && stats().compiles == s0.compiles + 1 && stats().hits == s0.hits);
}

void waiter_of_a_compile_that_throws() {
  use_dir((cwd + "/mt").c_str());
  code_cache_set_compile_slots(2);
  const std::string src = "a text whose first compile throws under a waiting thread";
  const Stats s0 = stats();
  g_sleep_ms = 50;
  g_throws = 1;
  std::string what;
  CodeObject b;
  std::thread first([&] { try { get(src); } catch (const std::runtime_error& ex) { what = ex.what(); } });
  while (g_calls.load() == s0.calls) std::this_thread::sleep_for(std::chrono::milliseconds(1));   // the first is inside the compiler
  std::thread second([&] { b = get(src); });
  first.join();
  second.join();
  g_sleep_ms = 0;
  REQUIRE(what == "stub compiler: no" && same(b, src));
  REQUIRE(stats().calls == s0.calls + 2 && stats().compiles == s0.compiles + 1 && stats().hits == s0.hits);
}

int run(const char* name, void (*fn)()) {
  try { fn(); }
  catch (const std::exception& ex) { printf("FAIL %s: %s\n", name, ex.what()); g_sleep_ms = 0; g_throws = 0; return 1; }
  printf("ok %s\n", name);
  return 0;
}
}  // namespace

int main() {
  char buf[4096];
  if (!getcwd(buf, sizeof buf)) return 2;
  cwd = buf;
  setvbuf(stdout, nullptr, _IOLBF, 0);
  int bad = 0;
  bad += run("sha256_and_fnv", sha256_and_fnv);
  bad += run("cold_then_warm", cold_then_warm);
  bad += run("wrong_file_other_text", [] { wrong_file("other_text"); });
  bad += run("wrong_file_truncated", [] { wrong_file("truncated"); });
  bad += run("wrong_file_no_elf", [] { wrong_file("no_elf"); });
  bad += run("wrong_file_symlink", [] { wrong_file("symlink"); });
  bad += run("directory_rule", directory_rule);
  bad += run("lru", lru);
  bad += run("same_text_from_8_threads", same_text_from_8_threads);
  bad += run("two_slots_16_threads", two_slots_16_threads);
  bad += run("stub_throws", stub_throws);
  bad += run("waiter_of_a_compile_that_throws", waiter_of_a_compile_that_throws);
  return bad ? 1 : 0;
}
