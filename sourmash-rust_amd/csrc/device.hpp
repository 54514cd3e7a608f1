// device.hpp -- HIP device context of the host library: lazy initialisation (so that the
// shared object loads and every C-ABI symbol resolves on a machine without a GPU), the
// library's own stream, grow-only device buffers and per-kernel HIP-event timers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "common.hpp"

namespace smh {

[[noreturn]] void throw_hip(hipError_t e, const char* what, const char* file, int line);

#define HIP_CHECK(expr)                                                  \
  do {                                                                   \
    hipError_t e_ = (expr);                                              \
    if (e_ != hipSuccess) ::smh::throw_hip(e_, #expr, __FILE__, __LINE__); \
  } while (0)

// Device blocks come from a pool of freed blocks kept by size class (device.cpp).  `cap` is the
// block's real size; give it back with the same value.  sync = wait for the device first, as
// hipFree would (for blocks that work still in flight may be using).
void* device_pool_alloc(size_t need, size_t* cap);
void device_pool_free(void* ptr, size_t cap, bool sync);
void device_pool_trim();   // hipFree everything the pool holds
void device_pool_set_limit(size_t bytes);   // cap on the bytes parked in the pool (default 1 GiB, SOURMASH_AMD_POOL_MB)
size_t device_pool_bytes();
// A test knob (smh_set_pool_fill; -1: off, the default): with a byte 0 .. 255 every block device_pool_alloc hands out, fresh
// or recycled, and every block device_pool_free parks is first filled with that byte over its whole size, and counted as
// "pool_filled".  Work space that is read before it is written, and pointers kept into a block that was given back, then
// read the pattern instead of zeros or the last call's -- often right -- values.  Off, the two functions do nothing more
// than test this word.
extern int32_t g_pool_fill;

// A block of the device pool owned by a long-lived object (Records' sequence and names) or by a call that keeps no account of
// its stream (records.cpp): work in flight may still be using it, so it waits for the device when it goes back.
struct PoolBlock {
  void* ptr = nullptr;
  size_t cap = 0;
  explicit PoolBlock(size_t bytes) { ptr = device_pool_alloc(bytes ? bytes : 1, &cap); }
  PoolBlock(const PoolBlock&) = delete; PoolBlock& operator=(const PoolBlock&) = delete;
  ~PoolBlock() { device_pool_free(ptr, cap, true); }
  template <class T> T* as() const { return reinterpret_cast<T*>(ptr); }
};

// The device blocks of one call -- or of one chunk, fold or operand of it -- on one stream.  take() borrows a block from the
// pool; every block lives until the workspace dies.  The destructor waits for the stream and then gives the blocks back, last
// taken first, without the device-wide wait: whatever was queued on the stream behind the last wait the caller made -- on a
// success path nothing (the call has just read its results back, and the wait is a query), on an error path the kernels of
// the statement that threw -- is over before a block can reach another stream.  There is no state to keep in step with the
// stream and so none to get wrong; lifetimes are scopes.  If the wait itself reports an error the blocks go back behind the
// device-wide wait instead.  Only for work the call completes: the two entry points that leave work open on purpose
// (Device::leave_open) use no pool blocks and must not start to.
class Workspace {
 public:
  explicit Workspace(hipStream_t s) : stream_(s) {}
  Workspace(Workspace&& o) noexcept : stream_(o.stream_), blocks_(std::move(o.blocks_)) { o.blocks_.clear(); }
  Workspace& operator=(Workspace&& o) noexcept {
    if (this != &o) { release(); stream_ = o.stream_; blocks_ = std::move(o.blocks_); o.blocks_.clear(); }
    return *this;
  }
  ~Workspace() { release(); }
  // `count` elements of T in a block of their own (one device_pool_alloc; a count of 0 still yields a valid pointer)
  template <class T> T* take(size_t count) { return static_cast<T*>(take_bytes(count * sizeof(T))); }

 private:
  struct Block { void* ptr; size_t cap; };
  void* take_bytes(size_t bytes);
  void release();
  hipStream_t stream_;
  std::vector<Block> blocks_;
};

// grow-only device allocation (never shrinks; released with the context or explicitly)
struct DeviceBuffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  void ensure(size_t need);
  void release();
  void release_after_sync();   // the caller has just waited for the device: no second wait
  template <class T> T* as() const { return reinterpret_cast<T*>(ptr); }
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer();
};

// grow-only page-locked host staging area: D2H at link speed instead of through a bounce buffer
struct PinnedBuffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  void ensure(size_t need);
  template <class T> T* as() const { return reinterpret_cast<T*>(ptr); }
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  ~PinnedBuffer();
};

struct KernelTimes {
  double ms = 0.0;
  uint64_t launches = 0;
};

class Device {
 public:
  // Throws Error(kInternal) when no HIP device is usable: the product path never falls
  // back to the CPU.
  static Device& get();
  static bool available();  // true when a GPU can be initialised (no throw)

  int id() const { return device_; }
  int cu_count() const { return cus_; }
  uint64_t grid_limit() const { return (uint64_t)cus_ * 8; }   // eight workgroups per CU: the limit of most grid-stride launches (grid_for)
  // the library's own stream (ordered after work an earlier entry point left open on another stream, see leave_open)
  hipStream_t stream() { order_after_open(stream_); return stream_; }
  hipStream_t copy_stream() const { return copy_stream_; }   // host->device chunks that overlap the hashing; the block compare's fill
  // the pair of events with which a call forks work onto copy_stream() and joins it again (under mutex())
  hipEvent_t fork_event() const { return ev_fork_; }
  hipEvent_t join_event() const { return ev_join_; }
  // Every entry point returns with its device work complete -- except the few that say so (smh_collection_begin with
  // world == 1, smh_collection_finish without a gathered buffer: a single owner's dictionary is only ever used by later
  // calls of this library).  Those call leave_open(s) last: an event is recorded behind their work, and EVERY later entry
  // point, whatever stream it works on, first makes its stream wait for that event (order_after_open, called by stream()
  // and user_stream()).  So the library's shared scratch buffers (tiled_scratch(), scratch) are never rewritten by a call
  // on stream B while the open work on stream A still reads them; calls on the same stream are ordered anyway.
  void leave_open(hipStream_t s);
  void order_after_open(hipStream_t s);
  // The stream an entry point with a `void *stream` argument works on.  Non-null: the caller's.
  // Null: the library's own (non-blocking) stream, first ordered after everything already queued
  // on the legacy default stream -- a caller whose "current stream" is the default one (torch's
  // usual state, handle 0) may have produced the inputs there, e.g. an all-gather it just waited on.
  hipStream_t user_stream(void* given);
  std::recursive_mutex& mutex() { return mu_; }

  // scratch shared by the fold / sort primitives (guarded by mutex())
  DeviceBuffer scratch;
  // per-tile record numbers of the running sketch launch (guarded by mutex(); see k_tile_records)
  DeviceBuffer tile_rec;
  // A zeroed 32-bit word for one launch of a tiled sketch kernel that hands its tiles out dynamically (the kernel's
  // workgroups atomicAdd it for their next tile).  The zeroing is queued on `s`, in front of the launch.  Words come
  // from a ring of kTileCounters: a word is zeroed again only behind kTileCounters - 1 later launches.  Reuse is safe
  // because every caller holds mutex() from here until its launch is queued and every sketching entry point waits for
  // its stream before it returns, so the launches that can be in flight together are those of ONE call, all on that
  // call's stream -- where zeroing, kernel and the next zeroing run in that order; the ring keeps launches apart even
  // if a future caller were to spread a call's launches over several streams.
  static constexpr uint32_t kTileCounters = 64;
  uint32_t* tile_counter(hipStream_t s);
  // Gives the ring back (smh_release_workspace; the caller holds mutex() and has waited for the device).  The next
  // tile_counter() allocates it anew; that is safe whatever the new block holds, because every word is zeroed on the
  // launch's stream in front of the launch that uses it and no word is read otherwise.
  void release_tile_counters() { tile_counters_.release_after_sync(); tile_counter_next_ = 0; }

  // HIP-event timing of named kernels (enabled by smh_profile_enable)
  void profile_enable(bool on);
  bool profiling() const { return profiling_; }
  void prof_begin(hipStream_t s);
  void prof_end(const char* name, hipStream_t s);
  void count(const char* name);                   // an event counter under the same names (launches += 1, always on)
  KernelTimes prof_get(const std::string& name);  // synchronises pending events
  void prof_reset();

 private:
  Device();
  int device_ = 0;
  int cus_ = 256;
  hipStream_t stream_ = nullptr;
  hipStream_t copy_stream_ = nullptr;
  hipEvent_t fence_ = nullptr;
  hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
  hipEvent_t open_event_ = nullptr;
  hipStream_t open_stream_ = nullptr;
  bool open_ = false;
  std::recursive_mutex mu_;
  DeviceBuffer tile_counters_;
  uint32_t tile_counter_next_ = 0;
  bool profiling_ = false;
  struct Pending { std::string name; hipEvent_t a, b; };
  std::vector<Pending> pending_;
  hipEvent_t cur_start_ = nullptr;
  std::map<std::string, KernelTimes> times_;
  void drain();
};

// The grid of a kernel that walks its items in a gridDim-stride loop: ceil(items / per_block) workgroups, at most `limit`
// (the launch's own: a multiple of the CU count or a constant), at least one.  g_grid_cap (smh_set_grid_cap; 0: none) lowers
// it further, so that tests reach the loops' later trips at small shapes; every lowered grid is counted as "grid_capped".
// Only for kernels that stride by gridDim: one that indexes by blockIdx alone needs its exact grid.
extern uint32_t g_grid_cap;
uint32_t grid_for(uint64_t items, uint32_t per_block, uint64_t limit, Device& dev);

}  // namespace smh
