// bpsw_ext_group.h -- the queue of the calls that wait for a pooled stream, and the groups the extension calls among them form.
//
// Why: a process has as many busy streams as hardware queues (GPU_MAX_HW_QUEUES, 4 where nobody set it), and an extension call holds
// its stream for the kernels AND the hand-over to the next caller (its wake-up, two enqueues, an event poll).  With more callers than
// streams the step runs at the rate of that lease, the device half empty.  The callers queued behind a stream therefore ride ONE
// launch chain: when a stream frees, the oldest waiter becomes its leader and takes with it, in arrival order, the waiters whose
// batches the same launch can serve (`compatible`); the leader enqueues and waits for the device, the others sleep until it hands
// them their status.  A waiter that is neither led nor promoted never polls.
//
// No HIP in here: what a "slot" is (a pooled stream) and how one is taken is the caller's, through the `take` callable -- called with
// the queue's lock held, returns the index of a slot it has taken, NO_SLOT when all are busy, or OWN_SLOT when there is no pool at
// all (the caller then uses a stream of its own and nothing is released).  tests/ext_group_host plays it with threads and sleeps.
#pragma once

#include <condition_variable>
#include <deque>
#include <mutex>

namespace bpsw {

struct ExtGroupWaiter {
  enum State { WAITING, LEADER, TAKEN, DONE };
  std::condition_variable cv;
  State state = WAITING;
  bool compatible = false;  // may share a launch chain with other compatible waiters (else: runs alone)
  void* item = nullptr;     // what the leader needs of this member (the caller's)
  int slot = -1;            // LEADER: the slot it holds
  // DONE: what the leader hands over
  int status = 0;
  float span_ms = 0.f;
  int group_n = 1;
};

class ExtGroupQueue {
 public:
  static constexpr int NO_SLOT = -1, OWN_SLOT = -2;
  static constexpr int MAX_GROUP = 8;

  // Blocks until the caller leads (returns true: w.slot is its slot, members[0..*n_members) are the waiters it leads besides itself,
  // already off the queue) or has been led by another (returns false: w.status / span_ms / group_n are set).  max_group: the
  // largest group, the leader included; 1 or an incompatible waiter: no members.
  template <class Take>
  bool acquire(ExtGroupWaiter& w, int max_group, Take&& take, ExtGroupWaiter** members, int* n_members) {
    *n_members = 0;
    std::unique_lock<std::mutex> lk(mu_);
    if (waiters_.empty()) {  // (a waiter is only ever queued while every slot is busy: nobody overtakes one)
      const int s = take();
      if (s != NO_SLOT) {
        w.slot = s;
        w.state = ExtGroupWaiter::LEADER;
        if (w.compatible) count_group(1);
        return true;
      }
    }
    w.state = ExtGroupWaiter::WAITING;
    waiters_.push_back(&w);
    w.cv.wait(lk, [&] { return w.state == ExtGroupWaiter::LEADER || w.state == ExtGroupWaiter::DONE; });
    if (w.state == ExtGroupWaiter::DONE) return false;
    if (w.compatible) {
      if (max_group > MAX_GROUP) max_group = MAX_GROUP;
      for (auto it = waiters_.begin(); it != waiters_.end() && *n_members + 1 < max_group;) {
        if ((*it)->compatible) {
          (*it)->state = ExtGroupWaiter::TAKEN;
          members[(*n_members)++] = *it;
          it = waiters_.erase(it);
        } else {
          ++it;
        }
      }
      count_group(1 + *n_members);
    }
    return true;
  }

  // The leader's, after the device phase of its group: every member gets its status and is woken.
  void complete(ExtGroupWaiter** members, int n_members, int status, float span_ms) {
    std::lock_guard<std::mutex> lk(mu_);
    for (int i = 0; i < n_members; ++i) {
      ExtGroupWaiter* m = members[i];
      m->status = status;
      m->span_ms = span_ms;
      m->group_n = 1 + n_members;
      m->state = ExtGroupWaiter::DONE;
      m->cv.notify_one();  // (under the lock: the waiter lives on its thread's stack and is gone once that thread has seen DONE)
    }
  }

  // A slot comes back (`put` gives it back, under the lock): the oldest waiters lead while slots can be taken.
  template <class Put, class Take>
  void release(Put&& put, Take&& take) {
    std::lock_guard<std::mutex> lk(mu_);
    put();
    while (!waiters_.empty()) {
      const int s = take();
      if (s < 0) break;
      ExtGroupWaiter* w = waiters_.front();
      waiters_.pop_front();
      w->slot = s;
      w->state = ExtGroupWaiter::LEADER;
      w->cv.notify_one();
    }
  }

  int waiting() {
    std::lock_guard<std::mutex> lk(mu_);
    return (int)waiters_.size();
  }
  int waiting_compatible() {  // ... of them, the ones that may be grouped
    std::lock_guard<std::mutex> lk(mu_);
    int n = 0;
    for (const ExtGroupWaiter* w : waiters_) n += w->compatible ? 1 : 0;
    return n;
  }
  // groups launched, members summed, largest group
  void counts(unsigned long long out[3]) {
    std::lock_guard<std::mutex> lk(mu_);
    out[0] = groups_; out[1] = members_; out[2] = largest_;
  }

 private:
  void count_group(int n) {
    ++groups_;
    members_ += (unsigned long long)n;
    if ((unsigned long long)n > largest_) largest_ = (unsigned long long)n;
  }
  std::mutex mu_;
  std::deque<ExtGroupWaiter*> waiters_;
  unsigned long long groups_ = 0, members_ = 0, largest_ = 0;
};

}  // namespace bpsw
