// ltr_lease.h -- the pool of device blocks a context recycles, and DevLease, the owner of everything ONE call takes from its
// context for as long as it runs: pooled device blocks, events, host staging memory.  Seen by every unit that queues work on the
// GPU per call: the units of ltr_ctx.h (which includes this) and, with a context they cannot look into, ltr_short.hip and ltr_nw.hip.
#ifndef LTR_LEASE_H_
#define LTR_LEASE_H_

#include <hip/hip_runtime.h>

#include <map>
#include <memory>

#include "ltr_internal.h"                                       // (+ <algorithm>, <mutex>, <string>, <vector>)

// Device allocations of a context are recycled: a plan for one locus needs ten small buffers, and
// hipMalloc / hipFree (a device-wide synchronisation each) would dominate the per-locus call.
// Blocks up to 64 MB are rounded to a power of two and parked here on release (at most 512 MB);
// larger ones go straight back to the runtime.
struct DevPool {
  // (sized for 288 GB of HBM: the blocks of a 10 k-locus plan -- 130 MB of reads, 180 MB of haplotype codes -- are
  // parked too, so a pipeline of large plans never waits in hipMalloc / hipFree, which synchronise the device)
  static constexpr size_t kMaxBlock = (size_t)2 << 30, kMaxCached = (size_t)8 << 30;
  std::multimap<size_t, void*> idle;
  std::map<void*, size_t> live;
  size_t cached = 0;
  std::mutex mu;
  static size_t size_class(size_t n) { size_t c = 256; while (c < n) c <<= 1; return c; }
  hipError_t alloc(void** out, size_t n) {
    std::lock_guard<std::mutex> lk(mu);
    size_t c = n;
    if (n <= kMaxBlock) {
      c = size_class(n);
      auto it = idle.find(c);
      if (it != idle.end()) { *out = it->second; idle.erase(it); cached -= c; live[*out] = c; return hipSuccess; }
    }
    hipError_t e = hipMalloc(out, c);
    if (e == hipErrorOutOfMemory) {                             // give the parked blocks (up to 8 GB) back and try once more
      for (auto& kv : idle) (void)hipFree(kv.second);
      idle.clear(); cached = 0;
      (void)hipGetLastError();
      e = hipMalloc(out, c);
    }
    if (e == hipSuccess) live[*out] = c;
    return e;
  }
  void release(void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(mu);
    auto it = live.find(p);
    if (it == live.end()) { (void)hipFree(p); return; }
    const size_t c = it->second;
    live.erase(it);
    if (c <= kMaxBlock && cached + c <= kMaxCached) { idle.emplace(c, p); cached += c; }
    else (void)hipFree(p);
  }
  void clear() {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& kv : idle) (void)hipFree(kv.second);
    idle.clear(); cached = 0;
  }
};

// how a lease reaches its context (ltr_ctx.hip): the pool, and the recycled events (see ltr_ctx: compact plans)
#pragma GCC visibility push(hidden)
DevPool& ctx_pool(ltr_ctx* ctx);
hipEvent_t ctx_take_event(ltr_ctx* ctx, bool timing);
void ctx_give_event(ltr_ctx* ctx, hipEvent_t e, bool timing);
#pragma GCC visibility pop

// The device blocks and events of ONE call, the streams it queues on, and the host staging memory its queued copies read or write.
// Invariant: on every way out of the call -- a normal return, an error return, an exception on its way to LTR_GUARD_END -- every
// stream is drained before any block goes back to the pool, before any event goes back to the cache and before any host memory
// handed out here is freed.  Host memory of the call's own that queued copies touch must outlive the lease: declare it BEFORE the
// lease (members of a per-call struct with the lease last), or take it from host().  The same holds for a lock the call borrows a
// resource of the context under: taken before the lease in that struct, it is released after the drain.
struct DevLease {
  ltr_ctx* const ctx;
  const hipStream_t st;
  std::vector<hipStream_t> side;                                // further streams the call queues on (also())
  std::vector<void*> blocks;
  std::vector<std::pair<hipEvent_t, bool>> events;              // (event, timing)
  std::vector<std::unique_ptr<char[]>> staging;
  bool drained = false;
  DevLease(ltr_ctx* c, hipStream_t s) : ctx(c), st(s) {}
  DevLease(const DevLease&) = delete;
  template <class T> hipError_t alloc(T** out, size_t bytes) {
    blocks.push_back(nullptr);                                  // (the slot first: growing the list may throw, and must not lose a block)
    const hipError_t e = ctx_pool(ctx).alloc(&blocks.back(), bytes);
    *out = static_cast<T*>(blocks.back());
    return e;
  }
  hipError_t event(hipEvent_t* out, bool timing) {              // from the context's cache, and back to it on the way out
    events.emplace_back(nullptr, timing);
    *out = events.back().first = ctx_take_event(ctx, timing);
    return *out ? hipSuccess : hipErrorOutOfMemory;
  }
  // tell the lease of a stream BEFORE the first thing is queued on it; the call itself joins it into st (by an event) before drain()
  void also(hipStream_t s) { if (s != st && std::find(side.begin(), side.end(), s) == side.end()) side.push_back(s); }
  template <class T> T* host(size_t n) {                        // n zeroed objects
    std::unique_ptr<char[]> m(new char[std::max<size_t>(n, 1) * sizeof(T)]());
    staging.push_back(std::move(m));
    return reinterpret_cast<T*>(staging.back().get());
  }
  // the call's last wait, after everything has been queued: the destructor does not wait again
  hipError_t drain() { const hipError_t e = hipStreamSynchronize(st); drained = e == hipSuccess; return e; }
  ~DevLease() {
    if (!drained && !(blocks.empty() && staging.empty())) {     // (nothing handed out: nothing queued on it)
      (void)hipStreamSynchronize(st);
      for (hipStream_t s : side) (void)hipStreamSynchronize(s);
    }
    for (void* p : blocks) ctx_pool(ctx).release(p);
    for (const auto& e : events) ctx_give_event(ctx, e.first, e.second);
  }
};

// hipError_t -> status of the calls that hold a DevLease (which drains the streams and gives everything back on the way out)
#define DEV_TRY(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { ltr::set_error(ctx, std::string(#call) + ": " + hipGetErrorString(e_)); return LTR_ERR_HIP; } } while (0)

#endif
