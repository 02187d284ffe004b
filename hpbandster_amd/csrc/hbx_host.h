// hbx_host.h -- host plumbing for results published to device-mapped host memory.  Users: hbx_host.hip (defines
// it; hbx_fetch), hbx_refit.hip (hbx_kde_refit_sync's output block) and hbx_kde.hip (hbx_kde_acquire_bound's
// record, flag and row).
#pragma once
#include "hbx_common.h"

// A device-mapped coherent host buffer (device address == host address): `cap` bytes of data, then the pool's
// tail.  A thread holds one per pool for its lifetime; when the thread ends the buffer goes back to its
// process-wide pool for the next thread (no HIP call from a thread-exit destructor, no pinned memory lost per
// short-lived result thread).  The sequence number travels with the buffer, so a pooled buffer's old tags and
// completion word never match a new owner's calls.  The two pools never exchange buffers: their layouts
// differ, and stale tags are only safe within one layout.
struct MappedBuf {
  char* p = nullptr;
  int64_t cap = 0;
  int32_t seq = 0;       // the last call's sequence number (calls count from 1)
  bool pending = false;  // set by a caller whose launches may still write into the buffer; cleared when they
                         // have landed.  A pending buffer is synchronised before reuse, never pooled
};

// Refit output blocks: `bytes` of flagged words (grown by doubling from 16 KiB), then the 16 flagged info words
// at p + cap.  Acquisition / fetch: FETCH_MAPPED_BYTES of hbx_fetch's data, its completion word, then (apart,
// at PUB_OFF: untagged bytes could pass for a later call's tags) PUB_BYTES of the final kernel's tagged words.
#define FETCH_MAPPED_BYTES 4096
#define PUB_OFF (FETCH_MAPPED_BYTES + 64)
#define PUB_BYTES (8 * (16 + 2 * HBX_MAX_D))
// this thread's buffer of the pool, its sequence number advanced for this call
int hbx_mapped_refit(int64_t bytes, MappedBuf** out);
int hbx_mapped_acq(MappedBuf** out);

// Spin until the `n` tagged words at w (seq << 32 | word, 8 bytes each, stored by the device in any order) all
// carry this call's sequence number, each word accepted on its own tag; their low halves go to out (nullable).
// Bounded: after spin_limit looks the stream is synchronised once and the remaining words looked at once more.
int wait_tagged(const volatile uint64_t* w, int64_t n, int32_t seq, uint32_t* out, hipStream_t s, int64_t spin_limit,
                const char* who);
