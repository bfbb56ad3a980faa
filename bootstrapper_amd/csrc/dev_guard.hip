// Guarded device allocations (dev_guard.h): the registry, the checker, the allocator hook for torch and the self-test.
#include <hip/hip_runtime.h>
#include <sys/types.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/bsmi.h"

namespace bsmi {

namespace {
struct GuardRec {
  char* base;
  size_t bytes;
  const char* file;  // nullptr: a tensor of torch's (bsmi_debug_torch_malloc)
  int line;
  int device;
};
// what one zone holds that is not 0xFF: the number of such bytes, the first and the last of them as offsets into the zone
struct ZoneHit {
  size_t n, first, last;
};
// The registry outlives every static destructor: torch releases its last tensors while the process exits, after this library's
// statics would have been destroyed.
std::mutex& guard_mu() {
  static std::mutex* m = new std::mutex;
  return *m;
}
std::map<void*, GuardRec>& guards() {
  static auto* g = new std::map<void*, GuardRec>;
  return *g;
}
// damaged zones of allocations that were released since the last bsmi_debug_check_guards()
std::atomic<int> g_released_bad{0};

size_t guard_bytes() {
  static const size_t g = [] {
    const char* e = getenv("BSMI_GUARD_MB");
    return e ? (size_t)atol(e) << 20 : (size_t)0;  // whole MiB: a multiple of 256 bytes, so p = base + g keeps hipMalloc's alignment
  }();
  return g;
}

// One launch looks at both zones of an allocation (blockIdx.y: 0 the zone before the buffer, 1 the one behind it) and leaves, per
// zone, the number of bytes that are not 0xFF and the first and last of them in out[3 * zone ..]; the host presets {0, ~0, 0}.  It
// reads the zones only: [z, z + g) each.  The zone behind begins at any byte, so whole 8-byte words are read from the first aligned
// address on and one thread takes the bytes before and behind them.
__global__ void zone_scan_kernel(const unsigned char* z0, const unsigned char* z1, size_t g, unsigned long long* out) {
  const int zone = blockIdx.y;
  const unsigned char* z = zone ? z1 : z0;
  const size_t head = (8 - ((uintptr_t)z & 7)) & 7;  // g is a multiple of 256: head < g
  const size_t words = (g - head) / 8;
  const uint64_t* w = (const uint64_t*)(z + head);
  unsigned long long n = 0, first = ~0ull, last = 0;
  auto look = [&](size_t i, unsigned v) {
    if (v != 0xFF) {
      ++n;
      if (i < first) first = i;
      if (i > last) last = i;
    }
  };
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < words; k += (size_t)gridDim.x * blockDim.x) {
    const uint64_t v = w[k];
    if (v != ~(uint64_t)0)
      for (int b = 0; b < 8; ++b) look(head + 8 * k + b, (unsigned)(v >> (8 * b)) & 0xFF);  // little endian: byte b lies at +b
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (size_t i = 0; i < head; ++i) look(i, z[i]);
    for (size_t i = head + 8 * words; i < g; ++i) look(i, z[i]);
  }
  if (n) {
    atomicAdd(&out[3 * zone], n);
    atomicMin(&out[3 * zone + 1], first);
    atomicMax(&out[3 * zone + 2], last);
  }
}

// Says what is not 0xFF in the two zones of `r`: hit[0] the zone before the buffer, hit[1] the one behind it.  The number of damaged
// zones (0..2), -1 after a HIP error.  The zones are reduced on the device (a read-back of both took longer than most tests);
// 48 bytes per device hold the result, one scan at a time.
int scan_zones(const GuardRec& r, size_t g, ZoneHit hit[2]) {
  static std::mutex* mu = new std::mutex;
  static auto* result = new std::map<int, unsigned long long*>;
  std::lock_guard<std::mutex> lk(*mu);
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess) return -1;
  if (prev != r.device && hipSetDevice(r.device) != hipSuccess) return -1;  // the kernel runs where the zones are
  struct Back {
    int prev, dev;
    ~Back() {
      if (prev != dev) (void)hipSetDevice(prev);
    }
  } back{prev, r.device};
  unsigned long long*& out = (*result)[r.device];
  if (!out && ::hipMalloc((void**)&out, 6 * sizeof(unsigned long long)) != hipSuccess) {
    out = nullptr;
    return -1;
  }
  unsigned long long h[6] = {0, ~0ull, 0, 0, ~0ull, 0};
  if (hipMemcpy(out, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) return -1;
  hipLaunchKernelGGL(zone_scan_kernel, dim3(128, 2), dim3(256), 0, 0, (const unsigned char*)r.base, (const unsigned char*)r.base + g + r.bytes,
                     g, out);
  if (hipGetLastError() != hipSuccess || hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  int bad = 0;
  for (int side = 0; side < 2; ++side) {
    const size_t n = (size_t)h[3 * side];
    hit[side] = ZoneHit{n, n ? (size_t)h[3 * side + 1] : g, (size_t)h[3 * side + 2]};
    bad += n != 0;
  }
  return bad;
}

// The line for each damaged zone (empty if it is intact): line[0] the zone before the buffer, line[1] the one behind it, offsets
// relative to the buffer's start and end.
void format_zones(const GuardRec& r, size_t g, const ZoneHit hit[2], char line[2][640]) {
  char site[512];
  if (r.file)
    snprintf(site, sizeof site, "%s:%d buffer of %zu bytes", r.file, r.line, r.bytes);
  else
    snprintf(site, sizeof site, "torch tensor of %zu bytes", r.bytes);
  line[0][0] = line[1][0] = 0;
  if (hit[0].n)
    snprintf(line[0], 640, "guard: %s: %zu bytes written BEFORE its start, at -%zu .. -%zu\n", site, hit[0].n, g - hit[0].first, g - hit[0].last);
  if (hit[1].n)
    snprintf(line[1], 640, "guard: %s: %zu bytes written PAST its end, at +%zu .. +%zu beyond the end\n", site, hit[1].n, hit[1].first, hit[1].last);
}

void report_zones(const GuardRec& r, size_t g, const ZoneHit hit[2]) {
  char line[2][640];
  format_zones(r, g, hit, line);
  fputs(line[0], stderr);
  fputs(line[1], stderr);
}

// Damaged zones of the live allocations (-1 = a HIP error), each reported on stderr if `report`.  The device is idle.
// One launch and two 48-byte copies per allocation, with the registry locked: a release on another thread waits meanwhile.  Fine for
// the few hundred allocations of a test run; a batched scan (a table of zone addresses, one launch) is the step after this.
int check_live(size_t g, bool report) {
  std::lock_guard<std::mutex> lk(guard_mu());
  int bad = 0;
  for (const auto& kv : guards()) {
    ZoneHit hit[2];
    const int b = scan_zones(kv.second, g, hit);
    if (b < 0) return -1;
    if (b && report) report_zones(kv.second, g, hit);
    bad += b;
  }
  return bad;
}

hipError_t malloc_between_zones(void** p, size_t bytes, const char* file, int line) {
  const size_t g = guard_bytes();
  if (!g) return ::hipMalloc(p, bytes);
  char* base = nullptr;
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return e;
  if ((e = ::hipMalloc((void**)&base, bytes + 2 * g)) != hipSuccess) return e;
  if ((e = hipMemset(base, 0xFF, g)) != hipSuccess || (e = hipMemset(base + g + bytes, 0xFF, g)) != hipSuccess ||
      (e = hipDeviceSynchronize()) != hipSuccess) {
    (void)::hipFree(base);
    return e;
  }
  std::lock_guard<std::mutex> lk(guard_mu());
  guards()[base + g] = GuardRec{base, bytes, file, line, device};
  *p = base + g;
  return hipSuccess;
}

// Releases a guarded allocation after the work on `s` (the whole device if `whole_device`) has ended and its zones were read:
// the damaged ones are reported (if `report`) and added to the process-wide count.  Never aborts; after a HIP error the check is
// given up quietly (the runtime may be gone: torch releases tensors while the interpreter shuts down).
hipError_t free_checked(void* p, hipStream_t s, bool whole_device, bool report) {
  const size_t g = guard_bytes();
  if (!g || !p) return ::hipFree(p);
  GuardRec r;
  {
    std::lock_guard<std::mutex> lk(guard_mu());
    auto it = guards().find(p);
    if (it == guards().end()) return ::hipFree(p);
    r = it->second;
    guards().erase(it);
  }
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  const bool hop = prev >= 0 && prev != r.device;
  if (prev >= 0 && (!hop || hipSetDevice(r.device) == hipSuccess) &&
      (whole_device ? hipDeviceSynchronize() : hipStreamSynchronize(s)) == hipSuccess) {
    ZoneHit hit[2];
    const int bad = scan_zones(r, g, hit);
    if (bad > 0) {
      if (report) report_zones(r, g, hit);
      g_released_bad.fetch_add(bad);
    }
  }
  const hipError_t e = ::hipFree(r.base);
  if (hop) (void)hipSetDevice(prev);
  return e;
}
}  // namespace

bool guards_on() { return guard_bytes() != 0; }

hipError_t guarded_malloc(void** p, size_t bytes, const char* file, int line) { return malloc_between_zones(p, bytes, file, line); }

hipError_t guarded_free(void* p) {
  if (!guard_bytes() || !p) return ::hipFree(p);
  std::lock_guard<std::mutex> lk(guard_mu());
  auto it = guards().find(p);
  if (it == guards().end()) return ::hipFree(p);
  void* base = it->second.base;
  guards().erase(it);
  return ::hipFree(base);
}

hipError_t guarded_free_checked(void* p, hipStream_t s) { return free_checked(p, s, false, true); }

}  // namespace bsmi

// Number of guard zones found written to (0 = all intact; -1 = a HIP error): those of the live allocations, each reported on
// stderr with the allocation site, the buffer's size and the first / last touched offset relative to the buffer, plus those that
// the checked releases (torch tensors, stream scratch) have counted since the last call.
extern "C" int bsmi_debug_check_guards(void) {
  using namespace bsmi;
  const size_t g = guard_bytes();
  if (!g) return 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  const int live = check_live(g, true);
  if (live < 0) return -1;
  return live + g_released_bad.exchange(0);
}

// The allocator pair for torch.cuda.memory.CUDAPluggableAllocator (`stream` is a hipStream_t, a pointer): exactly `size` bytes between two zones, the far one beginning at
// byte `size` (torch's own allocator rounds up to 512 bytes and packs blocks side by side, which hides short overruns).
extern "C" void* bsmi_debug_torch_malloc(ssize_t size, int device, void* stream) {
  using namespace bsmi;
  (void)stream;
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess) return nullptr;
  if (prev != device && hipSetDevice(device) != hipSuccess) return nullptr;
  void* p = nullptr;
  const hipError_t e = malloc_between_zones(&p, size > 0 ? (size_t)size : 0, nullptr, 0);
  if (prev != device) (void)hipSetDevice(prev);
  if (e != hipSuccess) {
    fprintf(stderr, "bsmi_debug_torch_malloc: %zd bytes on device %d: %s\n", size, device, hipGetErrorString(e));
    return nullptr;
  }
  return p;
}

extern "C" void bsmi_debug_torch_free(void* ptr, ssize_t size, void* stream) {
  (void)size;
  (void)bsmi::free_checked(ptr, (hipStream_t)stream, true, true);
}

// Does the checker see what it must?  One guarded buffer of 1000 bytes; single bytes written with hipMemset -- into the buffer's own
// zones, memory that it owns -- just past the end, just before the start and at the outermost byte of each zone; after each write
// the scan must name exactly the zones and offsets written so far, the report's lines must print them relative to the buffer, the
// walk over the live allocations must count them and a checked release must count them too.  0 = all of this holds, -1 = BSMI_GUARD_MB
// unset or a HIP error, > 0 = the step that failed.
namespace bsmi {
namespace {
int selftest_buffer(size_t n) {
  const size_t g = guard_bytes();
  if (!g) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  const int live0 = check_live(g, false);
  if (live0 < 0) return -1;
  char* p = nullptr;
  if (malloc_between_zones((void**)&p, n, "selftest", 0) != hipSuccess) return -1;
  GuardRec r;
  {
    std::lock_guard<std::mutex> lk(guard_mu());
    auto it = guards().find(p);
    if (it == guards().end()) {  // not registered: nothing to check, and no zones to hand to the checked release
      (void)::hipFree(p);
      return 1;
    }
    r = it->second;
  }
  ZoneHit hit[2];
  int rc = 0;
  // {where the byte goes, then what the scan must say: before-zone n / first / last, behind-zone n / first / last}
  const struct {
    char* at;
    ZoneHit before, behind;
  } steps[4] = {
      {p + n, {0, g, 0}, {1, 0, 0}},                   // the byte just past the end
      {p - 1, {1, g - 1, g - 1}, {1, 0, 0}},           // the byte just before the start
      {p + n + g - 1, {1, g - 1, g - 1}, {2, 0, g - 1}},  // the outermost byte behind
      {p - g, {2, 0, g - 1}, {2, 0, g - 1}},           // the outermost byte before
  };
  if (scan_zones(r, g, hit) != 0) rc = 2;
  for (int i = 0; i < 4 && !rc; ++i) {
    if (hipMemset(steps[i].at, 0, 1) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
      rc = -1;
      break;
    }
    const int want = (steps[i].before.n != 0) + (steps[i].behind.n != 0);
    if (scan_zones(r, g, hit) != want) rc = 10 + i;
    else if (memcmp(&hit[0], &steps[i].before, sizeof(ZoneHit)) || memcmp(&hit[1], &steps[i].behind, sizeof(ZoneHit))) rc = 20 + i;
  }
  if (!rc) {  // ... and the two lines that a report of this state prints, offsets as the reader sees them
    char line[2][640], want[2][640];
    format_zones(r, g, hit, line);
    snprintf(want[0], 640, "guard: selftest:0 buffer of %zu bytes: 2 bytes written BEFORE its start, at -%zu .. -1\n", n, g);
    snprintf(want[1], 640, "guard: selftest:0 buffer of %zu bytes: 2 bytes written PAST its end, at +0 .. +%zu beyond the end\n", n, g - 1);
    if (strcmp(line[0], want[0]) || strcmp(line[1], want[1])) rc = 25;
  }
  // bsmi_debug_check_guards() is check_live() plus the count of the checked releases, both held here; it is not called itself, for it
  // would print this buffer's lines and take the caller's count
  if (!rc && check_live(g, false) != live0 + 2) rc = 30;
  const int before = g_released_bad.load();
  (void)free_checked(p, nullptr, true, false);
  const int counted = g_released_bad.load() - before;
  if (counted > 0) g_released_bad.fetch_sub(counted);  // the self-test's own damage is not the caller's
  if (!rc && counted != 2) rc = 40;
  if (!rc) {
    std::lock_guard<std::mutex> lk(guard_mu());
    if (guards().count(p)) rc = 41;
  }
  return rc;
}
}  // namespace
}  // namespace bsmi

// ... and the same with 1003 bytes (+ 100 to the failed step), where the zone behind begins at no multiple of 8 bytes.
extern "C" int bsmi_debug_guard_selftest(void) {
  int rc = bsmi::selftest_buffer(1000);
  if (!rc && (rc = bsmi::selftest_buffer(1003)) > 0) rc += 100;
  return rc;
}
