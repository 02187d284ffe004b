// hbx_host.hip -- host plumbing: the pools of device-mapped host buffers and the waits on what the device
// publishes into them (hbx_host.h), hbx_fetch, the timing events and hbx_stream_order.
#include "hbx_host.h"

#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

static std::atomic<int64_t> g_mapped_live{0};  // device-mapped host buffers allocated (hbx_mapped_host_buffers)

// One pool of mapped buffers of one layout (hbx_host.h).  Never destroyed: thread exits at process end may
// still return buffers.
struct MappedPool {
  const int64_t min_cap;  // data bytes of the smallest buffer
  const int64_t tail;     // bytes after the data
  std::mutex mu;
  std::vector<MappedBuf> free;
};
// a thread's buffer of one pool, returned at thread exit
struct MappedHolder {
  MappedPool* const pool;
  MappedBuf b;
  explicit MappedHolder(MappedPool* p) : pool(p) {}
  ~MappedHolder() {
    if (b.p && !b.pending) {
      std::lock_guard<std::mutex> g(pool->mu);
      pool->free.push_back(b);
    }  // (a pending buffer is left to the process: its words may still be in flight)
  }
};
static MappedPool* const refit_pool = new MappedPool{16384, 256};
static MappedPool* const acq_pool = new MappedPool{PUB_OFF + PUB_BYTES, 0};
static thread_local MappedHolder t_refit(refit_pool);
static thread_local MappedHolder t_acq(acq_pool);

// the holder's buffer with at least `bytes` of data, this call's sequence number (>= 1) in it
static int mapped_get(MappedHolder& h, int64_t bytes, MappedBuf** out) {
  MappedBuf& b = h.b;
  MappedPool& pool = *h.pool;
  if (b.pending) {  // the last call failed after its launches: let them land before the buffer is reused
    HBX_HIP(hipDeviceSynchronize());
    b.pending = false;
  }
  if (bytes > b.cap) {
    MappedBuf nb;
    {
      std::lock_guard<std::mutex> g(pool.mu);
      for (size_t i = 0; i < pool.free.size(); ++i)
        if (pool.free[i].cap >= bytes) {
          nb = pool.free[i];
          pool.free.erase(pool.free.begin() + i);
          break;
        }
    }
    if (!nb.p) {
      int64_t cap = b.cap > 0 ? b.cap : pool.min_cap;
      while (cap < bytes) cap *= 2;
      void* p = nullptr;
      HBX_HIP(hipHostMalloc(&p, (size_t)(cap + pool.tail),
                            hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable));
      void* dp = nullptr;
      HBX_HIP(hipHostGetDevicePointer(&dp, p, 0));
      if (dp != p) {
        (void)hipHostFree(p);
        return hbx_fail(HBX_ERR_UNSUPPORTED, "mapped host memory has a different device address");
      }
      memset(p, 0, (size_t)(cap + pool.tail));  // (no stale tag can match: sequence numbers start at 1)
      nb.p = (char*)p;
      nb.cap = cap;
      g_mapped_live.fetch_add(1, std::memory_order_relaxed);
    }
    if (b.p) {  // the smaller buffer (every call on it completed) back to the pool
      std::lock_guard<std::mutex> g(pool.mu);
      pool.free.push_back(b);
    }
    b = nb;
  }
  b.seq = b.seq == INT32_MAX ? 1 : b.seq + 1;
  *out = &b;
  return HBX_OK;
}

int hbx_mapped_refit(int64_t bytes, MappedBuf** out) { return mapped_get(t_refit, bytes, out); }
int hbx_mapped_acq(MappedBuf** out) { return mapped_get(t_acq, PUB_OFF + PUB_BYTES, out); }

int wait_tagged(const volatile uint64_t* w, int64_t n, int32_t seq, uint32_t* out, hipStream_t s, int64_t spin_limit,
                const char* who) {
  const uint32_t sq = (uint32_t)seq;
  int64_t i = 0;
  auto take = [&] {  // the words from i on whose tag is the call's
    for (; i < n; ++i) {
      const uint64_t v = __atomic_load_n((const uint64_t*)(w + i), __ATOMIC_ACQUIRE);
      if ((uint32_t)(v >> 32) != sq) return;
      if (out) out[i] = (uint32_t)v;
    }
  };
  for (int64_t it = 0; it < spin_limit && i < n; ++it) take();
  if (i < n) {
    HBX_HIP(hipStreamSynchronize(s));
    take();
    if (i < n) return hbx_fail(HBX_ERR_HIP, "%s: the device did not publish word %lld", who, (long long)i);
  }
  return HBX_OK;
}

// spin on hbx_fetch's completion word (one untagged word: bounded ~0.1 s, then the stream is synchronised)
static int wait_done(int32_t* done, int32_t seq, hipStream_t s, const char* who) {
  bool seen = false;
  for (int64_t i = 0; i < 20000000 && !seen; ++i) seen = __atomic_load_n(done, __ATOMIC_ACQUIRE) == seq;
  if (!seen) {
    HBX_HIP(hipStreamSynchronize(s));
    if (__atomic_load_n(done, __ATOMIC_ACQUIRE) != seq)
      return hbx_fail(HBX_ERR_HIP, "%s: the device did not store its completion word", who);
  }
  return HBX_OK;
}

extern "C" {

// A small device buffer (an acquisition's result record) to the host with no copy engine and no blocking
// synchronisation: one wave copies it into this thread's device-mapped coherent host buffer, then stores a
// completion word last (system scope, after a system fence); the host spins on that word (bounded: then
// the stream is synchronised) and copies the bytes out.  A DMA copy + stream synchronisation of the
// 48-byte record cost ~28 us per acquisition (tools/step_breakdown.py)
__global__ void fetch_publish_kernel(const uint32_t* __restrict__ src, int32_t words, uint32_t* dst, int32_t* done,
                                     int32_t seq) {
  for (int i = threadIdx.x; i < words; i += 64) hbx_publish_store(dst + i, src[i]);
  __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every lane's words acknowledged (one wave)
  if (threadIdx.x == 0) hbx_publish_done(done, seq);
}

int64_t hbx_mapped_host_buffers(void) { return g_mapped_live.load(std::memory_order_relaxed); }

int hbx_fetch(void* host_dst, const void* dev_src, int64_t bytes, void* stream) {
  if (bytes < 0 || (bytes > 0 && (!host_dst || !dev_src))) return hbx_fail(HBX_ERR_ARG, "hbx_fetch: bad arguments");
  const hipStream_t s = (hipStream_t)stream;
  const bool small = bytes <= FETCH_MAPPED_BYTES && (bytes & 3) == 0 && ((uintptr_t)dev_src & 3) == 0;
  if (!small) {  // larger or unaligned: a copy, then the stream polled to completion
    if (bytes > 0) HBX_HIP(hipMemcpyAsync(host_dst, dev_src, (size_t)bytes, hipMemcpyDeviceToHost, s));
    hipError_t e;
    while ((e = hipStreamQuery(s)) == hipErrorNotReady) {
    }
    if (e != hipSuccess) return hbx_fail(HBX_ERR_HIP, "hbx_fetch: %s", hipGetErrorString(e));
    return HBX_OK;
  }
  MappedBuf* mb = nullptr;
  int rc = hbx_mapped_acq(&mb);
  if (rc) return rc;
  int32_t* done = (int32_t*)(mb->p + FETCH_MAPPED_BYTES);
  hipLaunchKernelGGL(fetch_publish_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)dev_src, (int32_t)(bytes / 4),
                     (uint32_t*)mb->p, done, mb->seq);
  HBX_LAUNCH_CHECK();
  rc = wait_done(done, mb->seq, s, "hbx_fetch");
  if (rc) return rc;
  memcpy(host_dst, mb->p, (size_t)bytes);
  return HBX_OK;
}

// Timing events (hipEvent_t) for hbx_kde_acquire's `events` argument.
int hbx_event_create(void** ev) {
  HBX_HIP(hipEventCreate((hipEvent_t*)ev));
  return HBX_OK;
}
int hbx_event_destroy(void* ev) {
  HBX_HIP(hipEventDestroy((hipEvent_t)ev));
  return HBX_OK;
}
int hbx_event_elapsed_ms(void* start, void* stop, float* ms) {
  HBX_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return HBX_OK;
}

// Order stream `waiter` after everything enqueued on stream `signaller` so far (an event recorded on the
// signaller, waited for by the waiter; no host wait): a model refit or prepared on one stream and used from
// another (KDEPair / DeviceKDE call it when the calling stream is not the model's)
int hbx_stream_order(void* waiter, void* signaller) {
  if (waiter == signaller) return HBX_OK;
  thread_local hipEvent_t ev = nullptr;
  if (!ev) HBX_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HBX_HIP(hipEventRecord(ev, (hipStream_t)signaller));
  HBX_HIP(hipStreamWaitEvent((hipStream_t)waiter, ev, 0));
  return HBX_OK;
}

}  // extern "C"
