// The owner of every device (and pinned host) allocation of the library: gp::DevBuf<T>.  This header is the only place that allocates or frees
// GPU memory (tests/test_device_ownership.py); a context's buffers are DevBuf members of gp_ctx, so deleting the context frees them all.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <vector>
#include "../../include/gparml_hip.h"

struct gp_ctx;

namespace gp {

int fail(gp_ctx* ctx, int code, const char* fmt, ...);
hipStream_t ctx_stream(const gp_ctx* c);   // the context's stream; the null stream without a context (api.hip)

// Test mode (GPARML_POISON=1 at load time or gp_debug_set_option("poison_alloc", 1)): every device allocation that does not carry a documented
// zero-initialisation contract is filled with 0xFF bytes (a NaN as a double, -1 as an int) instead of zeros, and gp_set_globals refills the
// per-evaluation scratch and output buffers with it: a kernel that reads a region this evaluation did not write, or that relies on zeros nobody
// promised, then fails deterministically (NaN in the outputs) instead of once in a thousand runs.  DA_ZERO marks the buffers whose zeros ARE part of the
// design (padding nobody writes; each such call site says which region that is), DA_INIT the ones that were zeroed for tidiness only, DA_RAW the
// ones that are not initialised at all outside the test mode (every element is written before it is read).
extern std::atomic<int> g_opt_poison;
enum { DA_ZERO = 0, DA_INIT = 1, DA_RAW = 2 };
// test hook (gp_debug_set_option("alloc_fail_after", k)): the k-th allocation from then on fails with GP_ERR_HIP ("injected"); 0: off
extern std::atomic<int> g_alloc_fail_after;

// The one allocation function: `bytes` (at least 8) of device memory initialised by `mode` on the context's stream, or of pinned, mapped host
// memory (not initialised).  On failure *p is NULL and nothing is left allocated.
inline int alloc_bytes(gp_ctx* c, void** p, size_t bytes, int mode, bool pinned) {
  *p = nullptr;
  int k = g_alloc_fail_after.load();
  while (k > 0 && !g_alloc_fail_after.compare_exchange_weak(k, k - 1)) {}
  if (k == 1) return fail(c, GP_ERR_HIP, "allocation of %zu bytes failed: injected (alloc_fail_after)", bytes);
  bytes = std::max<size_t>(bytes, 8);
  hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocMapped) : hipMalloc(p, bytes);
  const bool poison = g_opt_poison.load() && mode != DA_ZERO;
  if (e == hipSuccess && !pinned && (poison || mode != DA_RAW) && (e = hipMemsetAsync(*p, poison ? 0xFF : 0, bytes, ctx_stream(c))) != hipSuccess) {
    (void)hipFree(*p);
    *p = nullptr;
  }
  if (e != hipSuccess) return fail(c, GP_ERR_HIP, "%s of %zu bytes failed: %s", pinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
  return GP_OK;
}

// Move-only owner of n elements of T: device memory, or pinned host memory with Pinned (PinnedBuf).  It converts to T*, so it is passed to kernel
// launches and argument structs as the raw pointer.  Never give one static storage duration: hipFree during process teardown is unsafe.
template <typename T, bool Pinned = false>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); std::swap(p_, o.p_); std::swap(n_, o.n_); } return *this; }
  ~DevBuf() { reset(); }
  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t size() const { return n_; }                 // elements
  size_t bytes() const { return n_ * sizeof(T); }
  void reset() { if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; n_ = 0; }
  // frees what the owner holds, then allocates n elements (left empty on failure)
  int alloc(gp_ctx* c, size_t n, int mode = DA_INIT) {
    reset();
    void* p = nullptr;
    const int rc = alloc_bytes(c, &p, n * sizeof(T), mode, Pinned);
    if (rc == GP_OK) { p_ = static_cast<T*>(p); n_ = n; }
    return rc;
  }
  // at least n elements: the buffer is kept when it is large enough, else replaced by a fresh one of n (the old one stays when that fails)
  int grow(gp_ctx* c, size_t n, int mode = DA_INIT) {
    if (p_ && n_ >= n) return GP_OK;
    DevBuf t;
    const int rc = t.alloc(c, n, mode);
    if (rc == GP_OK) *this = std::move(t);
    return rc;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};
template <typename T> using PinnedBuf = DevBuf<T, true>;

// replaces b by a fresh device table holding v (b stays as it was when that fails).  The copy is asynchronous on the context's stream: the
// caller synchronises before v goes.
template <typename T>
int upload(gp_ctx* c, DevBuf<T>& b, const std::vector<T>& v) {
  DevBuf<T> t;
  if (const int rc = t.alloc(c, v.size(), DA_RAW); rc != GP_OK) return rc;
  const hipError_t e = hipMemcpyAsync(t.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx_stream(c));
  if (e != hipSuccess) return fail(c, GP_ERR_HIP, "table upload failed: %s", hipGetErrorString(e));
  b = std::move(t);
  return GP_OK;
}

// The one rule for borrowed workspace.  A stage that needs scratch only for the length of its own launches (the split-k / split-n partial tiles of
// every phase-1 form, the global step's split-k products) takes it from the context's Workspace instead of owning it.  `capacity` is a pure
// function of the context's shape (workspace_capacity, api.hip), set once by gp_create: a consumer whose decomposition follows the room there is
// (p1i8.hip's slice count, linalg.hip's split-k factors) reads `capacity`, never the allocation's size, so its summation order cannot depend on
// what ran on the context before.  reserve() is for the one plan whose need can exceed the capacity (regime B's pair kernel, psi2.hip): called
// when the plan is built, it may replace the allocation by a larger one and leaves `capacity` where it is.  take() never allocates.
struct Workspace {
  DevBuf<double> buf;
  size_t capacity = 0;
  int alloc(gp_ctx* c);                                      // api.hip: capacity from the shape, then the buffer
  int reserve(gp_ctx* c, size_t n) { return buf.grow(c, n, DA_RAW); }
  // *out = the workspace, for n doubles; GP_ERR_UNSUPPORTED with a message naming `who` when n exceeds what is allocated
  int take(gp_ctx* c, size_t n, const char* who, double** out) {
    *out = nullptr;
    if (n > buf.size()) return fail(c, GP_ERR_UNSUPPORTED, "%s: needs %zu doubles of workspace, %zu are allocated", who, n, buf.size());
    *out = buf.get();
    return GP_OK;
  }
};

}  // namespace gp
