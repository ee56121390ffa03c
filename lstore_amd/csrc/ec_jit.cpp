// ec_jit.cpp -- the process-wide service of the run-time compiled networks (their source:
// ec_netgen.cpp): one entry per matrix, compiled once in the background by a child process
// (lsec_jitc, hipRTC for gfx950), bound to the device images of the plans that use it, and
// launched through hipModuleLaunchKernel once ready; the generic kernels serve until then.
#include <dlfcn.h>
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <signal.h>
#include <spawn.h>
#include <sys/socket.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/lstore_ec.h"
#include "ec_hiperr.h"
#include "ec_host.h"
#include "ec_jit.h"

namespace lsec {
namespace jit {

namespace {

struct Entry {
  Net net;
  std::vector<uint32_t> mat;  // its matrix: R x K coefficients (GF(2^w) elements), or the packet network's row masks
  enum State { kCompiling, kReady, kFailed } state = kCompiling;
  std::vector<char> code;                 // code object
  std::map<int, hipModule_t> modules;     // device -> module
  std::map<int, hipFunction_t> functions; // device -> kernel
  std::string err;
  std::vector<uint32_t> key;  // its g_by_matrix key
};

// leaked on purpose: a compile worker still waiting on its compiler when the process exits may
// touch them
std::mutex &g_mu = *new std::mutex();
std::condition_variable &g_cv = *new std::condition_variable();
// Compiles run in child processes (lsec_jitc, ec_jitc.cpp), started by at most kWorkers threads
// fed from a queue.  hipRTC never runs in this process: its compiler's global state, destroyed
// by the process's exit under a compile still running, corrupted the heap in round 4, and the
// wait for running compiles that fixed it held exit for as long as a compile takes (30 s for the
// widest w = 32 networks on the build host).  At exit no queued compile starts and the running
// compilers are killed; nothing is waited for (tests/test_jit_queue.py).
constexpr int kWorkers = 2;
auto &g_queue = *new std::deque<std::shared_ptr<struct Entry>>();
int g_running = 0, g_workers = 0;
bool g_exiting = false;
// bumped whenever an image is bound or unbound: invalidates the threads' ready() caches
std::atomic<uint64_t> g_gen{1};
// the compiler processes running now (their own lock: the exit handler may run while a worker
// holds g_mu)
std::mutex &g_child_mu = *new std::mutex();
auto &g_children = *new std::set<pid_t>();
bool g_children_killed = false;

void stop_compiles() {
  {
    std::lock_guard<std::mutex> lk(g_child_mu);
    g_children_killed = true;
    for (pid_t p : g_children) kill(p, SIGKILL);
  }
  std::lock_guard<std::mutex> lk(g_mu);
  g_exiting = true;
  g_cv.notify_all();
}
auto &g_by_matrix = *new std::map<std::vector<uint32_t>, std::shared_ptr<Entry>>();  // key: R, K, w, matrix
auto &g_by_image = *new std::map<const void *, std::shared_ptr<Entry>>();           // device image -> entry

// lsec_jitc beside this library (LSEC_JITC overrides)
const std::string &compiler_path() {
  // leaked: a compile worker may still report a failure while the process exits
  static const std::string &path = *new std::string([] {
    if (const char *e = getenv("LSEC_JITC")) return std::string(e);
    Dl_info info;
    if (dladdr(reinterpret_cast<void *>(&compiler_path), &info) && info.dli_fname) {
      std::string f(info.dli_fname);
      const size_t slash = f.rfind('/');
      return (slash == std::string::npos ? std::string(".") : f.substr(0, slash)) + "/lsec_jitc";
    }
    return std::string("lsec_jitc");
  }());
  return path;
}

// The exit handler is registered by the first compile (a handler that runs while no compile
// exists has nothing to do).
void register_exit_handler() {
  static std::once_flag once;
  std::call_once(once, [] { atexit(stop_compiles); });
}

// gfx950 code object of `src` from a compiler process (protocol in ec_jitc.cpp), or the reason in
// err.  Sockets, not pipes: a write to a compiler that died must return EPIPE, not raise SIGPIPE
// in the caller's process.
void compile_source(const std::string &src, std::string &err, std::vector<char> &code) {
  register_exit_handler();
  int in[2], out[2];
  if (socketpair(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0, in) != 0) {
    err = "socketpair failed";
    return;
  }
  if (socketpair(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0, out) != 0) {
    close(in[0]);
    close(in[1]);
    err = "socketpair failed";
    return;
  }
  posix_spawn_file_actions_t fa;
  posix_spawn_file_actions_init(&fa);
  posix_spawn_file_actions_adddup2(&fa, in[1], 0);
  posix_spawn_file_actions_adddup2(&fa, out[1], 1);
  posix_spawn_file_actions_addopen(&fa, 2, "/dev/null", O_WRONLY, 0);
  const std::string ppid = std::to_string(getpid());
  char *argv[] = {const_cast<char *>(compiler_path().c_str()), const_cast<char *>(ppid.c_str()), nullptr};
  pid_t pid = -1;
  int rc;
  {
    std::lock_guard<std::mutex> lk(g_child_mu);
    rc = g_children_killed ? -1 : posix_spawn(&pid, argv[0], &fa, nullptr, argv, ::environ);
    if (rc == 0) g_children.insert(pid);
  }
  posix_spawn_file_actions_destroy(&fa);
  close(in[1]);
  close(out[1]);
  if (rc != 0) {
    close(in[0]);
    close(out[0]);
    err = rc < 0 ? "exiting" : "cannot start the network compiler " + compiler_path() + ": " + strerror(rc);
    return;
  }
  for (size_t o = 0; o < src.size();) {
    const ssize_t w = send(in[0], src.data() + o, src.size() - o, MSG_NOSIGNAL);
    if (w <= 0) break;  // the compiler died: its missing reply says so below
    o += static_cast<size_t>(w);
  }
  close(in[0]);
  std::vector<char> reply;
  char buf[1 << 16];
  for (;;) {
    const ssize_t r = read(out[0], buf, sizeof(buf));
    if (r <= 0) break;
    reply.insert(reply.end(), buf, buf + r);
  }
  close(out[0]);
  // Wait for the exit without reaping (WNOWAIT), take the pid out of g_children, and only then
  // reap: until the reap the pid stays a zombie of ours, so stop_compiles can never SIGKILL a pid
  // the system has already handed to another process
  siginfo_t si;
  while (waitid(P_PID, static_cast<id_t>(pid), &si, WEXITED | WNOWAIT) < 0 && errno == EINTR) {
  }
  {
    std::lock_guard<std::mutex> lk(g_child_mu);
    g_children.erase(pid);
  }
  int status = 0;
  while (waitpid(pid, &status, 0) < 0 && errno == EINTR) {
  }
  uint64_t n = 0;
  if (reply.size() >= 13)
    for (int i = 0; i < 8; ++i) n |= static_cast<uint64_t>(static_cast<uint8_t>(reply[5 + i])) << (8 * i);
  if (reply.size() < 13 || std::memcmp(reply.data(), "LSJC", 4) != 0 || reply.size() != 13 + n) {
    std::lock_guard<std::mutex> lk(g_child_mu);
    err = g_children_killed ? "exiting" : "the network compiler " + compiler_path() + " gave no answer";
    return;
  }
  if (reply[4] != 0) {
    err.assign(reply.begin() + 13, reply.end());
    return;
  }
  code.assign(reply.begin() + 13, reply.end());
}

void compile(std::shared_ptr<Entry> e) {
  const auto t0 = std::chrono::steady_clock::now();
  std::string err;
  std::vector<char> code;
  compile_source(e->net.source(e->mat.data()), err, code);
  static const bool trace = getenv("LSEC_TRACE") != nullptr;
  if ((trace || !err.empty()) && err != "exiting")
    fprintf(stderr, "[lsec jit] %dx%d w=%d xor network: %s (%.2f s)\n", e->net.R, e->net.K, e->net.w, err.empty() ? "compiled" : err.c_str(),
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  std::lock_guard<std::mutex> lk(g_mu);
  e->code.swap(code);
  e->err = err;
  e->state = err.empty() ? Entry::kReady : Entry::kFailed;
  --g_running;
  g_cv.notify_all();
}

void compile_worker() {
  for (;;) {
    std::shared_ptr<Entry> e;
    {
      std::unique_lock<std::mutex> lk(g_mu);
      g_cv.wait(lk, [] { return g_exiting || !g_queue.empty(); });
      if (g_exiting) return;
      e = g_queue.front();
      g_queue.pop_front();
      // a network whose every image was unbound (its plans destroyed before the compile started)
      // is dropped: a later bind of the same matrix queues it afresh
      bool bound = false;
      for (const auto &kv : g_by_image)
        if (kv.second == e) {
          bound = true;
          break;
        }
      if (!bound) {
        g_by_matrix.erase(e->key);
        e->state = Entry::kFailed;
        e->err = "dropped: no longer bound";
        g_cv.notify_all();
        continue;
      }
      ++g_running;
    }
    compile(e);
  }
}

// the kernel of a ready entry on device `dev` (loads the module once per device; under g_mu)
hipFunction_t function_locked(Entry &e, int dev) {
  if (e.state != Entry::kReady) return nullptr;
  auto it = e.functions.find(dev);
  if (it != e.functions.end()) return it->second;
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  if (quiet([&] {
        const hipError_t r = hipModuleLoadData(&mod, e.code.data());
        return r != hipSuccess ? r : hipModuleGetFunction(&fn, mod, "lsec_xornet");
      }) != hipSuccess) {
    e.state = Entry::kFailed;
    e.err = "module load failed";
    return nullptr;
  }
  e.modules[dev] = mod;
  e.functions[dev] = fn;
  return fn;
}

// bind `image` to the entry of `net` over `mat`, queueing its compile if the matrix is new
void bind_net(const void *image, const Net &net, const uint32_t *mat) {
  const std::vector<uint32_t> key = net.key(mat);
  std::shared_ptr<Entry> e;
  bool start = false;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_by_matrix.find(key);
    if (it == g_by_matrix.end()) {
      e = std::make_shared<Entry>();
      e->net = net;
      e->mat.assign(mat, mat + net.words());
      e->key = key;
      g_by_matrix.emplace(key, e);
      start = true;
      g_queue.push_back(e);
      if (g_workers < kWorkers) {
        ++g_workers;
        std::thread(compile_worker).detach();
      }
    } else {
      e = it->second;
    }
    g_by_image[image] = e;
    g_gen.fetch_add(1, std::memory_order_acq_rel);
  }
  if (start) g_cv.notify_all();
}

}  // namespace

void bind(const void *image, const uint8_t *mat, int R, int K) {
  if (!image || !wants_xornet(R, K)) return;
  std::vector<uint32_t> m32(mat, mat + static_cast<size_t>(R) * K);
  bind_net(image, Net::matrix(R, K, 8), m32.data());
}

void bind_w(const void *image, const uint32_t *mat, int R, int K, int w) {
  if (!image || !wants_gfw_net(R, K, w)) return;
  bind_net(image, Net::matrix(R, K, w), mat);
}

void bind_pkt(const void *image, const uint32_t *masks, int R, int K, int w, int packet) {
  if (!image || !wants_pktnet(R, K, w)) return;
  const Net net = Net::packets(R, K, w, packet);
  if (net.D == 0) return;
  bind_net(image, net, masks);
}

void bind_pkt_field(const void *image, const uint32_t *coef, int R, int K, int w, int packet) {
  if (!image || !wants_pktnet(R, K, w) || (w != 8 && w != 16 && w != 32)) return;
  // w = 8: Cauchy's bit-sliced GF(2^8) (k_gf8_bitsliced's layout): Cauchy-good(10+4) at 4 MiB
  // 0.72 -> 0.74, (6+3) level (profiles/r04_v17_pktnet_cauchy8.txt); LSEC_JIT_VARIANT bit 27: off
  if (w == 8 && variant().cauchy8_pkt_off) return;
  bind_pkt(image, coef_masks(coef, R, K, w).data(), R, K, w, packet);
}

void unbind(const void *image) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_by_image.erase(image);
  g_gen.fetch_add(1, std::memory_order_acq_rel);
}

int wait(const void *image, int timeout_ms) {
  std::unique_lock<std::mutex> lk(g_mu);
  auto it = g_by_image.find(image);
  if (it == g_by_image.end()) return 0;
  std::shared_ptr<Entry> e = it->second;
  // a network someone waits for compiles next
  auto q = std::find(g_queue.begin(), g_queue.end(), e);
  if (q != g_queue.end() && q != g_queue.begin()) {
    g_queue.erase(q);
    g_queue.push_front(e);
  }
  g_cv.wait_for(lk, std::chrono::milliseconds(timeout_ms), [&] { return e->state != Entry::kCompiling; });
  return e->state == Entry::kReady ? 1 : 0;
}

hipFunction_t ready(const void *image, int R, int K) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  // per-thread cache of ready kernels: per-stripe launches from hundreds of pool threads take no
  // lock once their network is loaded (a bind or unbind anywhere empties every cache)
  struct Key {
    const void *image;
    int dev, R, K;
    bool operator<(const Key &o) const {
      return image != o.image ? image < o.image : dev != o.dev ? dev < o.dev : R != o.R ? R < o.R : K < o.K;
    }
  };
  thread_local std::map<Key, hipFunction_t> cache;
  thread_local uint64_t cache_gen = 0;
  const uint64_t gen = g_gen.load(std::memory_order_acquire);
  if (cache_gen != gen) {
    cache.clear();
    cache_gen = gen;
  }
  const Key key{image, dev, R, K};
  auto c = cache.find(key);
  if (c != cache.end()) return c->second;
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_by_image.find(image);
  if (it == g_by_image.end() || it->second->net.R != R || it->second->net.K != K) return nullptr;
  hipFunction_t fn = function_locked(*it->second, dev);
  if (fn && g_gen.load(std::memory_order_acquire) == gen) cache[key] = fn;  // not yet ready: ask again next time
  return fn;
}

namespace {

// One block per tile of `net` over every stripe, on the generated kernel's
// struct Args { long long size; int nstripes; int int2; Ref in[K]; Ref out[R]; unsigned phase; }
// (8-byte aligned size; int2: the packet size of a packet network, else padding)
hipError_t launch_net(hipFunction_t fn, const Net &net, const ShardRef *in, const ShardRef *out, int nstripes, int64_t size,
                      int int2, hipStream_t st) {
  const size_t refs = sizeof(ShardRef) * (net.K + net.R);
  std::vector<uint8_t> args(16 + refs + 8, 0);
  std::memcpy(args.data(), &size, 8);
  std::memcpy(args.data() + 8, &nstripes, 4);
  std::memcpy(args.data() + 12, &int2, 4);
  std::memcpy(args.data() + 16, in, sizeof(ShardRef) * net.K);
  std::memcpy(args.data() + 16 + sizeof(ShardRef) * net.K, out, sizeof(ShardRef) * net.R);
  const uint64_t tps = net.tiles_per_stripe(size);
  const uint32_t phase = lsec::tile_phase_net_on() ? static_cast<uint32_t>(tps / 8) : 0;
  std::memcpy(args.data() + 16 + refs, &phase, 4);
  size_t bytes = args.size();
  void *cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args.data(), HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
  const uint64_t ntiles = tps * static_cast<uint64_t>(nstripes);
  if (ntiles == 0) return hipSuccess;
  if (ntiles >= (1ull << 31)) return hipErrorInvalidValue;
  return hipModuleLaunchKernel(fn, static_cast<unsigned>(ntiles), 1, 1, 256, 1, 1,
                               static_cast<unsigned>(lsec::occupancy_lds_bytes(size)), st, nullptr, cfg);
}

}  // namespace

hipError_t launch(hipFunction_t fn, int R, int K, const ShardRef *in, const ShardRef *out, int nstripes, int64_t size,
                  hipStream_t st, int w) {
  return launch_net(fn, Net::matrix(R, K, w), in, out, nstripes, size, 0, st);
}

hipError_t launch_pkt(hipFunction_t fn, int R, int K, const ShardRef *in, const ShardRef *out, int nstripes, int64_t size,
                      int packet, int w, hipStream_t st) {
  return launch_net(fn, Net::packets(R, K, w, packet), in, out, nstripes, size, packet, st);  // the shape as bind_pkt
}

bool pkt_aligned(const ShardRef *in, int K, const ShardRef *out, int R, int w, int packet) {
  const int d = Net::packets(R, K, w, packet).D;
  if (d == 0) return false;
  const uint64_t a = 4u * static_cast<uint64_t>(d);
  for (int j = 0; j < K; ++j)
    if (in[j].base % a || static_cast<uint64_t>(in[j].stride) % a) return false;
  for (int r = 0; r < R; ++r)
    if (out[r].base % a || static_cast<uint64_t>(out[r].stride) % a) return false;
  return true;
}

}  // namespace jit
}  // namespace lsec

extern "C" {

// Test hook, not in include/ (no GPU): generate and compile, synchronously (lsec_jitc), the
// network of a pseudo-random matrix for each generator shape -- shape 0: w = 8 XOR network
// (R x K bytes), 1: w = 16 / 32 bit-sliced network (one wave, or the wave-pair split from 4 rows
// at w = 32 / 5 rows at w = 16), 2: packet network over bitmatrix masks (w <= 32), 3: packet
// network over GF(2^w) coefficients.  Returns 0, or -1 with the compiler's reason.
int lsec_test_jit_compile(int shape, int R, int K, int w, int packet, unsigned seed) {
  if (R < 1 || R > 8 || K < 1 || K > 32 || shape < 0 || shape > 3) return lsec::set_error("lsec_test_jit_compile: bad arguments");
  unsigned x = seed * 2654435761u + 12345u;
  auto rnd = [&x] {
    x = x * 1103515245u + 12345u;
    return x >> 7;
  };
  std::string src;
  if (shape == 0) {
    std::vector<uint8_t> m(static_cast<size_t>(R) * K);
    for (auto &v : m) v = static_cast<uint8_t>(rnd() | 1u);
    src = lsec::jit::xornet_source(m.data(), R, K);
  } else if (shape == 1) {
    if (w != 16 && w != 32) return lsec::set_error("lsec_test_jit_compile: w %d", w);
    std::vector<uint32_t> m(static_cast<size_t>(R) * K);
    for (auto &v : m) v = (rnd() ^ (rnd() << 16)) & (w == 16 ? 0xFFFFu : 0xFFFFFFFFu);
    src = lsec::jit::gfw_source(m.data(), R, K, w);
  } else {
    if (w < 2 || w > 32 || packet < 4) return lsec::set_error("lsec_test_jit_compile: w %d packet %d", w, packet);
    std::vector<uint32_t> masks(static_cast<size_t>(R) * w * K);
    if (shape == 2) {
      for (auto &v : masks) v = rnd() & rnd() & (w == 32 ? 0xFFFFFFFFu : (1u << w) - 1u);
    } else {
      if (w != 16 && w != 32) return lsec::set_error("lsec_test_jit_compile: w %d", w);
      std::vector<uint32_t> coef(static_cast<size_t>(R) * K);
      for (auto &v : coef) v = (rnd() ^ (rnd() << 16)) & (w == 16 ? 0xFFFFu : 0xFFFFFFFFu);
      masks = lsec::jit::coef_masks(coef.data(), R, K, w);
    }
    const lsec::jit::Net net = lsec::jit::Net::packets(R, K, w, packet);
    if (net.D == 0) return lsec::set_error("lsec_test_jit_compile: packet %d", packet);
    src = net.source(masks.data());
  }
  std::string err;
  std::vector<char> code;
  lsec::jit::compile_source(src, err, code);
  if (!err.empty()) return lsec::set_error("lsec_test_jit_compile: %s", err.c_str());
  return code.empty() ? lsec::set_error("lsec_test_jit_compile: no code object") : 0;
}

// Test hook, not in include/ (no GPU; the compiler runs on the host): bind n distinct pseudo-random
// R x K GF(2^w) matrices (w = 16 / 32) to stand-in image addresses (never dereferenced), wait up to
// wait_ms for the first compile, unbind them all, and return how many compiles were ready by then.
// A process that returns right after leaves compiles queued and running at its exit
// (tests/test_jit_queue.py).
int lsec_test_jit_queue(int n, int wait_ms, int R, int K, int w, unsigned seed) {
  if (n < 1 || n > 64 || wait_ms < 0 || R < 1 || R > 8 || K < 1 || K > 32 || (w != 16 && w != 32)) return -1;
  static char stand_in[64];
  std::vector<uint32_t> mat(static_cast<size_t>(R) * K);
  unsigned x = seed * 2654435761u + 777u;
  for (int i = 0; i < n; ++i) {
    for (auto &c : mat) {
      x = x * 1103515245u + 12345u;
      c = ((x >> 5) ^ (x << 11)) & (w == 16 ? 0xFFFFu : 0xFFFFFFFFu);
      c |= 2u;  // not an XOR-only row
    }
    lsec::jit::bind_net(stand_in + i, lsec::jit::Net::matrix(R, K, w), mat.data());
  }
  (void)lsec::jit::wait(stand_in, wait_ms);
  int ready = 0;
  {
    std::lock_guard<std::mutex> lk(lsec::jit::g_mu);
    for (int i = 0; i < n; ++i) {
      auto it = lsec::jit::g_by_image.find(stand_in + i);
      if (it != lsec::jit::g_by_image.end() && it->second->state == lsec::jit::Entry::kReady) ++ready;
    }
  }
  for (int i = 0; i < n; ++i) lsec::jit::unbind(stand_in + i);
  return ready;
}

namespace {

// The network of a test hook's shape (as lsec_test_jit_compile numbers them), or false with the
// reason recorded under the hook's name `who`.  packet is read for the packet shapes only.
bool test_net(const char *who, int shape, int R, int K, int w, int packet, lsec::jit::Net *net) {
  using lsec::jit::Net;
  if (shape < 0 || shape > 3) return lsec::set_error("%s: shape %d: 0 .. 3", who, shape), false;
  if (R < 1 || R > lsec::jit::kMaxRows) return lsec::set_error("%s: R %d: 1 .. %d rows", who, R, lsec::jit::kMaxRows), false;
  if (K < 1 || K > lsec::jit::kMaxCols) return lsec::set_error("%s: K %d: 1 .. %d inputs", who, K, lsec::jit::kMaxCols), false;
  if (shape == 0 ? w != 8 : shape == 1 ? w != 16 && w != 32 : shape == 2 ? w < 2 || w > 32 : w != 8 && w != 16 && w != 32)
    return lsec::set_error("%s: w %d: shape %d takes %s", who, w, shape,
                           shape == 0 ? "8" : shape == 1 ? "16 or 32" : shape == 2 ? "2 .. 32" : "8, 16 or 32"),
           false;
  if (shape < 2) {
    *net = Net::matrix(R, K, w);
    return true;
  }
  if (packet < 4 || packet > (1 << 20)) return lsec::set_error("%s: packet %d: 4 .. %d bytes", who, packet, 1 << 20), false;
  *net = Net::packets(R, K, w, packet);
  if (net->D == 0) return lsec::set_error("%s: packet %d: no lane width (pkt_shape: a multiple of 4 bytes)", who, packet), false;
  return true;
}

}  // namespace

// Test hook, not in include/ (no GPU): the bytes of a shard (packet networks: column bytes) one
// block of the shape's network covers per tile (Net::tile_bytes), or -1 on bad arguments, so that
// tests size their inputs from the engine.
int lsec_test_jit_tile(int shape, int R, int K, int w, int packet) {
  lsec::jit::Net net;
  return test_net("lsec_test_jit_tile", shape, R, K, w, packet, &net) ? net.tile_bytes() : -1;
}

// Test hook, not in include/ (GPU): run the network of any matrix, alone, by the production route:
// bound to a stand-in image (never dereferenced), compiled, fetched with ready() and launched
// through launch / launch_pkt over `in` (K shards) and `out` (R shards); `stream` is synchronised
// before it returns 0.  `mat`: R*K coefficients (shapes 0, 1, 3; shape 3 expands them by
// coef_masks as bind_pkt_field does) or R*w*K row masks [(r*w+l)*K + j] (shape 2).  At w = 16 / 32
// the network covers whole tiles only and nothing follows it.  Every refusal is -1 with a message
// naming the limit, before the first HIP call; a failed compile is -1 with the compiler's text.
int lsec_test_jit_run(int shape, int R, int K, int w, int packet, const unsigned *mat, const lsec_shard_t *in,
                      const lsec_shard_t *out, int nstripes, long long size, void *stream) {
  static const char *who = "lsec_test_jit_run";
  lsec::jit::Net net;
  if (!test_net(who, shape, R, K, w, packet, &net)) return -1;
  if (!mat || !in || !out) return lsec::set_error("%s: NULL %s", who, !mat ? "mat" : !in ? "in" : "out");
  if (nstripes < 0) return lsec::set_error("%s: nstripes %d: negative", who, nstripes);
  if (shape != 2 && w < 32)
    for (int i = 0; i < R * K; ++i)
      if (mat[i] >> w) return lsec::set_error("%s: coefficient %d is %u: above %u at w = %d", who, i, mat[i], (1u << w) - 1u, w);
  const long long unit = shape < 2 ? 8 : static_cast<long long>(w) * packet;
  if (size < 0 || size % unit)
    return lsec::set_error("%s: size %lld: not a multiple of %lld bytes (%s)", who, size, unit, shape < 2 ? "8" : "w * packet");
  std::vector<lsec::ShardRef> bi(K), bo(R);
  for (int j = 0; j < K; ++j) bi[j] = {reinterpret_cast<uint64_t>(in[j].base), in[j].stride};
  for (int r = 0; r < R; ++r) bo[r] = {reinterpret_cast<uint64_t>(out[r].base), out[r].stride};
  if (shape >= 2 && !lsec::jit::pkt_aligned(bi.data(), K, bo.data(), R, w, packet))
    return lsec::set_error("%s: a base or stride is not a multiple of the lane width, %d bytes (pkt_aligned)", who, 4 * net.D);
  const std::vector<uint32_t> m = shape == 3 ? lsec::jit::coef_masks(mat, R, K, w) : std::vector<uint32_t>(mat, mat + net.words());
  char stand_in;  // this call's own image address
  lsec::jit::bind_net(&stand_in, net, m.data());
  int rc = 0;
  if (!lsec::jit::wait(&stand_in, 900 * 1000)) {
    std::lock_guard<std::mutex> lk(lsec::jit::g_mu);
    const auto &e = lsec::jit::g_by_image.at(&stand_in);
    rc = lsec::set_error("%s: %s", who, e->state == lsec::jit::Entry::kCompiling ? "the compile took too long" : e->err.c_str());
  } else if (hipFunction_t fn = lsec::jit::ready(&stand_in, R, K)) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t err = shape < 2 ? lsec::jit::launch(fn, R, K, bi.data(), bo.data(), nstripes, size, st, w)
                               : lsec::jit::launch_pkt(fn, R, K, bi.data(), bo.data(), nstripes, size, packet, w, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) rc = lsec::set_error("%s: launch failed: %s", who, hipGetErrorString(err));
  } else {
    rc = lsec::set_error("%s: the compiled network did not load on this device", who);
  }
  lsec::jit::unbind(&stand_in);
  return rc;
}

}  // extern "C"
