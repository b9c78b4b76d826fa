// Host launch layer for libtecogan_hip.so (KERNELS.md, "Launch layer"): what a launcher has to know about the device
// it launches on -- the CU count, whether a kernel has been opted into its dynamic LDS, how many workgroups of a
// persistent kernel fit at once -- asked in one place and remembered per DEVICE, not per process: a process that uses a
// second device (a partitioned card's logical devices differ in CU count) gets that device's answers.
#pragma once
#include <atomic>
#include <climits>
#include <mutex>

namespace tg {

// ---- the table --------------------------------------------------------------
// "Already done / the cached value" per (device id, slot).  It makes no HIP call -- the device id and the action are
// passed in -- so a host-only program can drive it (tests/test_launch_table_cpu.py).  Safe against concurrent host threads.
class LaunchTable {
 public:
  static constexpr int DEVICES = 64;    // 8 cards x 8 partitions
  static constexpr int SLOTS = 128;     // one per (question, kernel) the library asks; about 45 are in use
  // a slot of its own for a call site (kept in a function-local static); -1 once they are used up
  int new_slot() {
    const int s = next_.fetch_add(1, std::memory_order_relaxed);
    return s < SLOTS ? s : -1;
  }
  // action() for (device, slot), run once: a result >= 0 is kept and returned from then on; a negative one is a failure,
  // returned but not kept, so that the next call runs the action again.  A device id or slot outside the table (an unknown
  // device: -1) is never cached: the action runs every time.  The action must not call once() itself (one plain mutex).
  template <class Action> int once(int device, int slot, Action&& action) {
    if (device < 0 || device >= DEVICES || slot < 0 || slot >= SLOTS) return action();
    std::atomic<int>& cell = cell_[device][slot];                 // 0: not yet; else the value + 1
    if (const int v = cell.load(std::memory_order_acquire)) return v - 1;
    std::lock_guard<std::mutex> lock(mu_);
    if (const int v = cell.load(std::memory_order_relaxed)) return v - 1;
    const int r = action();
    if (r >= 0 && r < INT_MAX) cell.store(r + 1, std::memory_order_release);
    return r;
  }

 private:
  std::atomic<int> next_{0};
  std::mutex mu_;
  std::atomic<int> cell_[DEVICES][SLOTS] = {};
};

inline LaunchTable& launch_table() {
  static LaunchTable t;
  return t;
}

}  // namespace tg

#ifdef __HIPCC__
#include "tg_common.h"

namespace tg {

// the calling thread's current device, -1 where the runtime does not say (no device: nothing is cached then)
inline int current_device() {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return dev;
}

inline int device_cus_of(int dev) {                  // -1 on failure
  static const int slot = launch_table().new_slot();
  return launch_table().once(dev, slot, [dev] {
    int ncu = 0;
    if (dev < 0 || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1) {
      (void)hipGetLastError();
      return -1;
    }
    return ncu;
  });
}

// CU count of the calling thread's current device; 256 where the runtime does not say
inline int device_cus() {
  const int ncu = device_cus_of(current_device());
  return ncu > 0 ? ncu : 256;
}

// Opts Kernel into `bytes` of dynamic LDS, once per (device, kernel).  TG_OK, or TG_E_HIP with the error text set and
// the runtime's sticky error cleared; `what` names the kernel in that text.
template <auto Kernel> int ensure_dynamic_lds(size_t bytes, const char* what) {
  static const int slot = launch_table().new_slot();
  hipError_t e = hipSuccess;
  const int rc = launch_table().once(current_device(), slot, [&e, bytes] {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e == hipSuccess ? 0 : -1;
  });
  if (rc == 0) return TG_OK;
  (void)hipGetLastError();
  set_error("%s: %d bytes of dynamic LDS per workgroup: %s", what, (int)bytes, hipGetErrorString(e));
  return TG_E_HIP;
}

// Workgroups of Kernel (`threads` threads, `lds_bytes` of dynamic LDS) that the current device holds at once: the
// kernel is opted into its LDS, then occupancy x CUs; cached per (device, kernel), 0 on error ("not supported here": the
// callers fall back).  For the launches whose workgroups wait for each other this is a correctness input: a grid
// above it never finishes.  A capacity above 0 says that the opt-in is made on this device.
template <auto Kernel> int resident_capacity(int threads, size_t lds_bytes) {
  static const int slot = launch_table().new_slot();
  const int dev = current_device(), ncu = device_cus_of(dev);      // (asked outside the action: once() does not nest)
  if (ncu < 1) return 0;
  const int cap = launch_table().once(dev, slot, [=] {
    const void* fn = reinterpret_cast<const void*>(Kernel);
    int per_cu = 0;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds_bytes) != hipSuccess) {
      (void)hipGetLastError();
      return -1;
    }
    return per_cu * ncu;
  });
  return cap > 0 ? cap : 0;
}

}  // namespace tg
#endif  // __HIPCC__
