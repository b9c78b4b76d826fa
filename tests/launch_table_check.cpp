// Stand-alone check of the launch layer's (device id, slot) table (csrc/tg_launch.h), built with the host compiler by
// tests/test_launch_table_cpu.py.  Without hipcc the header is the HIP-free table alone; the actions here are counting
// fakes.  One line per check ("ok <name>" / "FAILED <name>: ..."), exit status 1 on any failure.
#include <atomic>
#include <climits>
#include <cstdio>
#include <thread>
#include <vector>

#include "tg_launch.h"

using tg::LaunchTable;

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("  line %d: %s\n", __LINE__, #cond);            \
      ok = false;                                                 \
    }                                                             \
  } while (0)
static void report(bool ok, const char* name) {
  std::printf("%s %s\n", ok ? "ok" : "FAILED", name);
  failures += !ok;
}

static LaunchTable table;        // (static: 32 KB of cells)

// the action runs exactly once per (device, slot) for devices 0 and 1, in either order, and its value is what later calls get
static void once_per_device_and_slot() {
  bool ok = true;
  const int slots[2] = {table.new_slot(), table.new_slot()};
  const int order[2][2] = {{0, 1}, {1, 0}};
  EXPECT(slots[0] >= 0 && slots[1] >= 0 && slots[0] != slots[1]);
  for (int k = 0; k < 2; ++k) {
    int runs[2] = {0, 0};
    for (int round = 0; round < 3; ++round)
      for (int i = 0; i < 2; ++i) {
        const int dev = order[k][i];
        const int v = table.once(dev, slots[k], [&] { ++runs[dev]; return 100 * k + dev; });   // (device 0 of k = 0 caches the value 0)
        EXPECT(v == 100 * k + dev);
      }
    EXPECT(runs[0] == 1 && runs[1] == 1);
  }
  report(ok, "once_per_device_and_slot");
}

// a failing action (negative result) is not recorded as done: it runs again on the next call, until one succeeds
static void failure_is_not_recorded() {
  bool ok = true;
  const int slot = table.new_slot();
  int runs = 0;
  for (int i = 0; i < 3; ++i) EXPECT(table.once(0, slot, [&] { ++runs; return -7; }) == -7);
  EXPECT(runs == 3);
  EXPECT(table.once(0, slot, [&] { ++runs; return 5; }) == 5);
  EXPECT(table.once(0, slot, [&] { ++runs; return -7; }) == 5);
  EXPECT(runs == 4);
  int other = 0;                                         // the failures on device 0 left device 1 alone
  EXPECT(table.once(1, slot, [&] { ++other; return 6; }) == 6 && other == 1);
  report(ok, "failure_is_not_recorded");
}

// a device id (or slot) outside the table is never cached and never indexes the cells (the sanitizer builds would say)
static void out_of_range_is_never_cached() {
  bool ok = true;
  const int slot = table.new_slot();
  const int devices[] = {-1, LaunchTable::DEVICES, LaunchTable::DEVICES + 1, INT_MAX, INT_MIN};
  for (const int dev : devices) {
    int runs = 0;
    for (int i = 0; i < 3; ++i) EXPECT(table.once(dev, slot, [&] { ++runs; return 9; }) == 9);
    EXPECT(runs == 3);
  }
  const int bad_slots[] = {-1, LaunchTable::SLOTS, INT_MAX, INT_MIN};
  for (const int s : bad_slots) {
    int runs = 0;
    for (int i = 0; i < 3; ++i) EXPECT(table.once(0, s, [&] { ++runs; return 9; }) == 9);
    EXPECT(runs == 3);
  }
  int runs = 0;                                          // the last device id of the table is cached like any other
  for (int i = 0; i < 3; ++i) EXPECT(table.once(LaunchTable::DEVICES - 1, slot, [&] { ++runs; return 3; }) == 3);
  EXPECT(runs == 1);
  LaunchTable small;                                     // slots run out: -1 from then on, distinct before
  std::vector<bool> seen(LaunchTable::SLOTS, false);
  for (int i = 0; i < LaunchTable::SLOTS; ++i) {
    const int s = small.new_slot();
    EXPECT(s >= 0 && s < LaunchTable::SLOTS && !seen[s]);
    if (s >= 0 && s < LaunchTable::SLOTS) seen[s] = true;
  }
  for (int i = 0; i < 5; ++i) EXPECT(small.new_slot() == -1);
  report(ok, "out_of_range_is_never_cached");
}

// eight threads hammering one slot run the action once, and all of them get its value
static void eight_threads_one_slot() {
  bool ok = true;
  const int slot = table.new_slot();
  std::atomic<int> runs{0}, wrong{0}, ready{0};
  std::vector<std::thread> threads;
  for (int t = 0; t < 8; ++t)
    threads.emplace_back([&] {
      ready.fetch_add(1);
      while (ready.load() < 8) std::this_thread::yield();       // start together
      for (int i = 0; i < 20000; ++i)
        if (table.once(2, slot, [&] { runs.fetch_add(1); return 42; }) != 42) wrong.fetch_add(1);
    });
  for (std::thread& th : threads) th.join();
  EXPECT(runs.load() == 1);
  EXPECT(wrong.load() == 0);
  report(ok, "eight_threads_one_slot");
}

int main() {
  once_per_device_and_slot();
  failure_is_not_recorded();
  out_of_range_is_never_cached();
  eight_threads_one_slot();
  return failures ? 1 : 0;
}
