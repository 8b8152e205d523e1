// Host offset arrays of a C-ABI call, staged to the device without a host wait: shared by the entry points that take per-utterance
// host offsets and launch on the caller's stream (asv_ingest_frames, asv_ingest_windows, asv_decode_compressed).  Each of them keeps its OWN thread_local
// ring, so the offsets of one do not evict the other's.
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "asv_internal.h"

namespace asv {

// The two (or three: `c`) host offset arrays of a call, one behind the other on the device.  Per calling thread: a ring of page-locked staging slots, each with its device
// twin.  Unchanged contents (fixed batch shapes) reuse the last upload, changed ones take the next slot and copy asynchronously - the
// host never waits for the stream either way (the extraction loops submit new offsets per batch, alternating between two streams).
// Ordering is by events, whichever streams the calls of a thread use:
//   * `uploaded` is recorded behind a slot's copy on the stream that made it; a call on ANOTHER stream that reuses the slot makes its
//     stream wait for that event (a device-side wait) before its kernel reads the slot;
//   * every stream that has launched a reader of a slot has its own `read` event there, recorded behind its latest launch; a slot is
//     overwritten only after all of them have completed - in practice the launches of kRing changes of the offsets ago.
// A thread's slots live as long as the process, like the offset cache of frontend.hip (a destructor would call into a HIP runtime that
// may already be gone at exit).
struct OffsetRing {
  static constexpr int kRing = 8;
  struct Reader { hipStream_t stream; hipEvent_t read; };
  struct Slot {
    long long *host = nullptr, *dev = nullptr;
    size_t cap = 0, count = 0;
    hipStream_t stream = nullptr;          // the stream the current contents were copied on
    hipEvent_t uploaded = nullptr;         // behind that copy
    std::vector<Reader> readers;           // one event per stream that has read this slot since it was filled (events are kept and reused)
    size_t n_readers = 0;                  // entries of `readers` in use
  };
  Slot slot[kRing];
  int at = 0, device = -1;
  static int drain(Slot &k) {              // every launch that reads the slot has finished
    for (size_t i = 0; i < k.n_readers; ++i) ASV_HIP_CHECK(hipEventSynchronize(k.readers[i].read));
    k.n_readers = 0;
    return ASV_OK;
  }
  int get(const long long *a, const long long *b, size_t each, hipStream_t s, const long long **out, const long long *c = nullptr) {
    int cur = 0;
    ASV_HIP_CHECK(hipGetDevice(&cur));
    if (device != cur) {                                                      // (another device: start over there)
      for (Slot &k : slot) {
        { const int rc = drain(k); if (rc) return rc; }
        for (Reader &r : k.readers) ASV_HIP_CHECK(hipEventDestroy(r.read));
        if (k.uploaded) ASV_HIP_CHECK(hipEventDestroy(k.uploaded));
        if (k.host) ASV_HIP_CHECK(hipHostFree(k.host));
        if (k.dev) ASV_HIP_CHECK(hipFree(k.dev));
        k = Slot();
      }
      device = cur;
    }
    const size_t count = (c ? 3 : 2) * each;
    Slot &l = slot[at];
    if (l.dev && l.count == count && memcmp(l.host, a, each * 8) == 0 && memcmp(l.host + each, b, each * 8) == 0 &&
        (!c || memcmp(l.host + 2 * each, c, each * 8) == 0)) {
      if (s != l.stream) ASV_HIP_CHECK(hipStreamWaitEvent(s, l.uploaded, 0));   // the copy was queued on another stream: this one waits for it
      *out = l.dev;
      return ASV_OK;
    }
    at = (at + 1) % kRing;
    Slot &k = slot[at];
    { const int rc = drain(k); if (rc) return rc; }
    if (!k.uploaded) ASV_HIP_CHECK(hipEventCreateWithFlags(&k.uploaded, hipEventDisableTiming));
    if (count > k.cap) {
      if (k.host) ASV_HIP_CHECK(hipHostFree(k.host));
      if (k.dev) ASV_HIP_CHECK(hipFree(k.dev));
      k.host = k.dev = nullptr; k.cap = k.count = 0;
      ASV_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&k.host), count * 16, hipHostMallocDefault));
      ASV_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&k.dev), count * 16));
      k.cap = count * 2;
    }
    memcpy(k.host, a, each * 8);
    memcpy(k.host + each, b, each * 8);
    if (c) memcpy(k.host + 2 * each, c, each * 8);
    k.count = 0;                                                              // (not reusable until the copy is queued and marked)
    ASV_HIP_CHECK(hipMemcpyAsync(k.dev, k.host, count * 8, hipMemcpyHostToDevice, s));
    ASV_HIP_CHECK(hipEventRecord(k.uploaded, s));
    k.count = count;
    k.stream = s;
    *out = k.dev;
    return ASV_OK;
  }
  // behind the launch on stream s that reads the current slot
  int launched(hipStream_t s) {
    Slot &k = slot[at];
    size_t i = 0;
    while (i < k.n_readers && k.readers[i].stream != s) ++i;
    if (i == k.n_readers) {
      if (i == k.readers.size()) {
        Reader r = {s, nullptr};
        ASV_HIP_CHECK(hipEventCreateWithFlags(&r.read, hipEventDisableTiming));
        k.readers.push_back(r);
      }
      k.readers[i].stream = s;
      ++k.n_readers;
    }
    ASV_HIP_CHECK(hipEventRecord(k.readers[i].read, s));
    return ASV_OK;
  }
};

}  // namespace asv
