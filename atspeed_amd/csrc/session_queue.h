// Host-only bookkeeping of a session (include/atspeed_hip.h "sessions"): the lane table, the ticket table and the submission queue.
// No HIP call and no device type in here: the engine (engine.hip) keeps what a user needs on the device in `Job`, and
// tests/test_session_queue_cpu.py compiles this header into a stand-alone program under the address and undefined-behaviour sanitizers.
//
//   submit(job)          -> ticket (1, 2, ... in submission order); only queues
//   admit(on_admit)      -> every free lane, in ascending lane order, takes the next queued user in submission order
//   begin_round()        -> counts one round for the session and for every occupied lane (call it only when a lane is occupied)
//   retire(lane, status) -> frees the lane; the user's record waits in `done` until take_done() hands it out, exactly once
// A ticket is in exactly one place at a time: the queue, a lane, or the list of finished users that have not been reported yet.
#pragma once
#include <stdint.h>

#include <deque>
#include <utility>
#include <vector>

namespace ats_session {

struct Done {                      // what a finished user leaves behind (atspeed_session_done)
  int64_t ticket;
  int32_t lane, status;
  int64_t rounds_queued, rounds_in_lane;
};

template <typename Job>
class Queue {
 public:
  explicit Queue(int n_lanes) : lanes_(n_lanes > 0 ? (size_t)n_lanes : 0) {}

  int n_lanes() const { return (int)lanes_.size(); }
  int occupied() const { return occupied_; }
  int64_t queued() const { return (int64_t)waiting_.size(); }
  int64_t pending() const { return queued() + occupied_; }           // users a drain still has to finish
  bool idle() const { return waiting_.empty() && occupied_ == 0; }
  int64_t rounds() const { return rounds_; }
  int64_t lane_rounds() const { return lane_rounds_; }
  int64_t admitted() const { return admitted_; }
  int64_t retired() const { return retired_; }

  int64_t submit(Job job) {
    waiting_.push_back(Waiting{next_ticket_, rounds_, std::move(job)});
    return next_ticket_++;
  }

  bool lane_busy(int lane) const { return lanes_[(size_t)lane].busy; }
  Job& lane_job(int lane) { return lanes_[(size_t)lane].job; }

  // on_admit(lane, ticket, job) -> 0, or an error: that user then stays at the head of the queue, its lane stays free, and admission stops
  template <typename F>
  int admit(F&& on_admit) {
    int rc = 0;
    for (size_t l = 0; l < lanes_.size() && !waiting_.empty(); ++l) {
      Lane& ln = lanes_[l];
      if (ln.busy) continue;
      Waiting& w = waiting_.front();
      if ((rc = on_admit((int)l, w.ticket, w.job)) != 0) break;
      ln.busy = true; ln.ticket = w.ticket; ln.rounds_queued = rounds_ - w.submit_round; ln.rounds_in_lane = 0;
      ln.job = std::move(w.job);
      waiting_.pop_front();
      ++occupied_; ++admitted_;
    }
    return rc;
  }

  void begin_round() {
    ++rounds_;
    for (Lane& ln : lanes_) if (ln.busy) { ++ln.rounds_in_lane; ++lane_rounds_; }
  }

  void retire(int lane, int32_t status) {
    Lane& ln = lanes_[(size_t)lane];
    if (!ln.busy) return;
    done_.push_back(Done{ln.ticket, lane, status, ln.rounds_queued, ln.rounds_in_lane});
    ln.busy = false; ln.ticket = 0; ln.job = Job();
    --occupied_; ++retired_;
  }

  int64_t done_waiting() const { return (int64_t)done_.size(); }
  // up to `cap` finished users, oldest first; each record leaves the table here
  int take_done(Done* out, int cap) {
    int n = 0;
    while (n < cap && !done_.empty()) { out[n++] = done_.front(); done_.pop_front(); }
    return n;
  }

 private:
  struct Waiting { int64_t ticket, submit_round; Job job; };
  struct Lane { bool busy = false; int64_t ticket = 0, rounds_queued = 0, rounds_in_lane = 0; Job job{}; };
  std::vector<Lane> lanes_;
  std::deque<Waiting> waiting_;
  std::deque<Done> done_;
  int occupied_ = 0;
  int64_t next_ticket_ = 1, rounds_ = 0, lane_rounds_ = 0, admitted_ = 0, retired_ = 0;
};

}  // namespace ats_session
