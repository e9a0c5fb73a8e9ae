// The queue of the calls that wait for a pooled stream (csrc/bpsw_ext_group.h, unchanged) under a sanitizer, without HIP: threads play
// the callers, a vector of busy counts plays the stream pool, a sleep plays the device phase of a group's launch chain.
//   ext_group_host stress <threads> <calls> <streams> <max_group>
//   ext_group_host fifo
// stress: every call completes exactly once (as a leader or led), no group exceeds the maximum, a caller that runs alone never leads or
// joins a group, no slot is held twice, the queue's own counts add up.  fifo: callers are queued one by one behind one busy slot (the
// gauge says when each has arrived), and the order of leaders and the members each takes must be the arrival order.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "bpsw_ext_group.h"

using bpsw::ExtGroupQueue;
using bpsw::ExtGroupWaiter;

namespace {

struct Pool {
  ExtGroupQueue q;
  std::vector<int> busy;  // guarded by the queue's lock (take / put run under it)
  int take() {
    for (size_t i = 0; i < busy.size(); ++i)
      if (!busy[i]) { busy[i] = 1; return (int)i; }
    return ExtGroupQueue::NO_SLOT;
  }
};

struct Call {
  int id = 0;
  bool compatible = false;
  std::atomic<int> completed{0};
  int led_by = -1;
};

std::atomic<long> g_wrong{0};
void wrong(const char* what) {
  fprintf(stderr, "EXTGROUP wrong: %s\n", what);
  g_wrong.fetch_add(1);
}

struct GroupLog {
  std::mutex mu;
  std::vector<std::vector<int>> groups;  // leader id, then member ids
};

// one call: returns when it has completed, as a leader or led
void run_call(Pool& P, Call& me, int max_group, int hold_us, std::vector<std::atomic<int>>& slot_holders, GroupLog* log) {
  ExtGroupWaiter w;
  w.compatible = me.compatible;
  w.item = &me;
  ExtGroupWaiter* members[ExtGroupQueue::MAX_GROUP];
  int n = 0;
  const bool leads = P.q.acquire(w, me.compatible ? max_group : 1, [&] { return P.take(); }, members, &n);
  if (!leads) {
    if (!me.compatible) wrong("a caller that runs alone was led");
    if (w.status != 7) wrong("a led caller did not get the leader's status");
    if (w.group_n < 2 || w.group_n > max_group) wrong("a led caller's group size");
    if (me.completed.load() != 1) wrong("a led caller woke before its completion was booked");
    return;
  }
  if (w.slot < 0) wrong("a leader without a slot");
  if (slot_holders[(size_t)w.slot].fetch_add(1) != 0) wrong("a slot held twice");
  if (1 + n > max_group) wrong("a group above the maximum");
  if (!me.compatible && n != 0) wrong("a caller that runs alone leads a group");
  std::vector<int> entry{me.id};
  for (int i = 0; i < n; ++i) {
    Call* m = (Call*)members[i]->item;
    if (!m->compatible) wrong("a caller that runs alone was taken into a group");
    m->led_by = me.id;
    entry.push_back(m->id);
  }
  if (log) { std::lock_guard<std::mutex> g(log->mu); log->groups.push_back(entry); }
  std::this_thread::sleep_for(std::chrono::microseconds(hold_us));  // the launch chain on the device
  me.completed.fetch_add(1);
  for (int i = 0; i < n; ++i) ((Call*)members[i]->item)->completed.fetch_add(1);
  P.q.complete(members, n, 7, 0.25f);
  slot_holders[(size_t)w.slot].fetch_sub(1);
  const int slot = w.slot;
  P.q.release([&] { P.busy[(size_t)slot] = 0; }, [&] { return P.take(); });
}

int stress(int threads, int calls, int streams, int max_group) {
  Pool P;
  P.busy.assign((size_t)streams, 0);
  std::vector<std::atomic<int>> holders((size_t)streams);
  for (auto& h : holders) h.store(0);
  std::vector<std::vector<Call>> all((size_t)threads);
  for (int t = 0; t < threads; ++t) {
    all[(size_t)t] = std::vector<Call>((size_t)calls);
    for (int k = 0; k < calls; ++k) {
      all[(size_t)t][(size_t)k].id = t * calls + k;
      all[(size_t)t][(size_t)k].compatible = (t * 7 + k * 3) % 5 != 0;  // a fifth run alone
    }
  }
  std::vector<std::thread> th;
  for (int t = 0; t < threads; ++t)
    th.emplace_back([&, t] {
      for (int k = 0; k < calls; ++k) {
        run_call(P, all[(size_t)t][(size_t)k], max_group, 30 + (t * 13 + k * 7) % 90, holders, nullptr);
        if (k % 3 == 0) std::this_thread::sleep_for(std::chrono::microseconds(20 + (t + k) % 40));  // host work between two calls
      }
    });
  for (auto& x : th) x.join();
  long compat = 0;
  for (auto& v : all)
    for (auto& c : v) {
      if (c.completed.load() != 1) wrong("a call completed not exactly once");
      if (c.compatible) ++compat;
    }
  unsigned long long cnt[3];
  P.q.counts(cnt);
  if ((long)cnt[1] != compat) wrong("the queue's member count is not the number of grouped-plan calls");
  if ((int)cnt[2] > max_group || cnt[0] > cnt[1]) wrong("the queue's counts");
  if (P.q.waiting() != 0) wrong("waiters left in the queue");
  printf("EXTGROUP calls %d groups %llu members %llu largest %llu wrong %ld\n", threads * calls, cnt[0], cnt[1], cnt[2], g_wrong.load());
  return g_wrong.load() == 0 ? 0 : 1;
}

int fifo() {
  Pool P;
  P.busy.assign(1, 0);
  std::vector<std::atomic<int>> holders(1);
  holders[0].store(0);
  GroupLog log;
  const bool compat[10] = {true, false, true, true, false, true, true, true, true, true};
  std::vector<Call> calls(10);
  // the main thread holds the one slot
  ExtGroupWaiter hold;
  ExtGroupWaiter* none[1];
  int n0 = 0;
  if (!P.q.acquire(hold, 1, [&] { return P.take(); }, none, &n0) || hold.slot != 0) wrong("the free slot was not taken at once");
  std::vector<std::thread> th;
  for (int i = 0; i < 10; ++i) {
    calls[(size_t)i].id = i;
    calls[(size_t)i].compatible = compat[i];
    th.emplace_back([&, i] { run_call(P, calls[(size_t)i], 4, 200, holders, &log); });
    while (P.q.waiting() != i + 1) std::this_thread::yield();  // arrival order = i
  }
  P.q.release([&] { P.busy[0] = 0; }, [&] { return P.take(); });
  for (auto& x : th) x.join();
  const std::vector<std::vector<int>> want = {{0, 2, 3, 5}, {1}, {4}, {6, 7, 8, 9}};
  if (log.groups != want) {
    wrong("leaders and members are not in arrival order");
    for (auto& g : log.groups) { for (int v : g) fprintf(stderr, " %d", v); fprintf(stderr, " |"); }
    fprintf(stderr, "\n");
  }
  for (auto& c : calls)
    if (c.completed.load() != 1) wrong("a call completed not exactly once");
  unsigned long long cnt[3];
  P.q.counts(cnt);
  if (cnt[0] != 2 || cnt[1] != 8 || cnt[2] != 4) wrong("the queue's counts (two groups of four; the callers that ran alone are not counted)");
  printf("EXTGROUP fifo groups %zu wrong %ld\n", log.groups.size(), g_wrong.load());
  return g_wrong.load() == 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "fifo")) return fifo();
  if (argc >= 6 && !strcmp(argv[1], "stress")) return stress(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
  fprintf(stderr, "usage: ext_group_host stress <threads> <calls> <streams> <max_group> | fifo\n");
  return 2;
}
