// Stand-alone check of atspeed_amd/csrc/session_queue.h (the host-only tables of a session): tests/test_session_queue_cpu.py compiles this
// with -fsanitize=address,undefined and runs it.  Every CHECK that fails prints its line and the program exits 1; "session_queue ok" ends a
// clean run.  The "user" here is a number of rounds it needs: a lane counts it down once per round and retires at zero.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <set>
#include <vector>

#include "session_queue.h"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

struct Job {
  int rounds_left = 0;
  std::shared_ptr<int> payload;          // heap state that moves with the job: the sanitizers see a leak or a use after free
};
using Q = ats_session::Queue<Job>;
using ats_session::Done;

static Job job(int rounds) { return Job{rounds, std::make_shared<int>(rounds)}; }

// admission, one round over the occupied lanes, retirement: what atspeed_session_round does with the tables; returns false for an empty round
static bool round_of(Q& q, std::vector<Done>* out, std::vector<std::pair<int, int64_t>>* admitted = nullptr) {
  const int rc = q.admit([&](int lane, int64_t ticket, Job& j) {
    CHECK(j.payload && *j.payload == j.rounds_left);
    if (admitted) admitted->push_back({lane, ticket});
    return 0;
  });
  CHECK(rc == 0);
  if (q.occupied() == 0) return false;
  q.begin_round();
  for (int l = 0; l < q.n_lanes(); ++l)
    if (q.lane_busy(l) && --q.lane_job(l).rounds_left == 0) q.retire(l, 0);
  Done buf[8];
  for (int n; (n = q.take_done(buf, 8)) > 0;) out->insert(out->end(), buf, buf + n);
  return true;
}

static void test_submission_order_and_lane_reuse() {
  Q q(2);
  CHECK(q.idle() && q.n_lanes() == 2);
  for (int u = 0; u < 5; ++u) CHECK(q.submit(job(u == 0 ? 3 : 1)) == u + 1);       // tickets 1 .. 5 in submission order
  CHECK(q.queued() == 5 && q.occupied() == 0 && q.pending() == 5);
  std::vector<Done> done;
  std::vector<std::pair<int, int64_t>> adm;
  CHECK(round_of(q, &done, &adm));                                                  // round 1: tickets 1, 2 in lanes 0, 1; 2 retires
  CHECK(adm.size() == 2 && adm[0] == std::make_pair(0, (int64_t)1) && adm[1] == std::make_pair(1, (int64_t)2));
  CHECK(done.size() == 1 && done[0].ticket == 2 && done[0].lane == 1 && done[0].rounds_in_lane == 1 && done[0].rounds_queued == 0);
  CHECK(q.lane_busy(0) && !q.lane_busy(1));
  adm.clear();
  CHECK(round_of(q, &done, &adm));                                                  // round 2: lane 1 is reused by ticket 3 (retirement and admission
  CHECK(adm.size() == 1 && adm[0] == std::make_pair(1, (int64_t)3));                //          at the same boundary), which retires at once
  CHECK(done.size() == 2 && done[1].ticket == 3 && done[1].lane == 1 && done[1].rounds_queued == 1);
  adm.clear();
  CHECK(round_of(q, &done, &adm));                                                  // round 3: ticket 4 in lane 1; tickets 1 and 4 retire together
  CHECK(adm.size() == 1 && adm[0] == std::make_pair(1, (int64_t)4));
  CHECK(done.size() == 4 && done[2].ticket == 1 && done[2].rounds_in_lane == 3 && done[3].ticket == 4 && done[3].rounds_queued == 2);
  adm.clear();
  CHECK(round_of(q, &done, &adm));                                                  // round 4: the lowest free lane takes the last user
  CHECK(adm.size() == 1 && adm[0] == std::make_pair(0, (int64_t)5));
  CHECK(done.size() == 5 && done[4].ticket == 5 && done[4].lane == 0);
  CHECK(q.idle() && q.rounds() == 4 && q.lane_rounds() == 3 + 1 + 1 + 1 + 1 && q.admitted() == 5 && q.retired() == 5);
}

static void test_empty_round_and_once_only() {
  Q q(3);
  std::vector<Done> done;
  CHECK(!round_of(q, &done) && done.empty() && q.rounds() == 0);                    // nothing queued, no lane occupied: nothing happens
  q.submit(job(2));
  CHECK(round_of(q, &done) && done.empty());
  CHECK(round_of(q, &done) && done.size() == 1);
  Done extra[4];
  CHECK(q.take_done(extra, 4) == 0);                                                // a ticket is reported exactly once
  CHECK(!round_of(q, &done) && done.size() == 1 && q.rounds() == 2);
  q.retire(0, 0);                                                                   // retiring a free lane changes nothing
  CHECK(q.retired() == 1 && q.done_waiting() == 0);
}

static void test_done_list_is_handed_out_in_pieces() {
  Q q(4);
  for (int u = 0; u < 4; ++u) q.submit(job(1));
  CHECK(q.admit([](int, int64_t, Job&) { return 0; }) == 0);
  q.begin_round();
  for (int l = 0; l < 4; ++l) q.retire(l, l == 2 ? -6 : 0);
  CHECK(q.done_waiting() == 4);
  Done a[3], b[3];
  CHECK(q.take_done(a, 3) == 3 && q.take_done(b, 3) == 1 && q.take_done(b + 1, 2) == 0);
  CHECK(a[0].ticket == 1 && a[1].ticket == 2 && a[2].ticket == 3 && a[2].status == -6 && b[0].ticket == 4 && b[0].status == 0);
}

static void test_admission_error_and_failed_round() {
  Q q(2);
  for (int u = 0; u < 3; ++u) q.submit(job(2));
  CHECK(q.admit([](int, int64_t ticket, Job&) { return ticket == 2 ? -3 : 0; }) == -3);       // ticket 2 is refused: it keeps its place
  CHECK(q.admitted() == 1 && q.occupied() == 1 && q.queued() == 2 && q.lane_busy(0) && !q.lane_busy(1));
  int64_t into_lane_1 = 0;
  CHECK(q.admit([&](int lane, int64_t ticket, Job&) { if (lane == 1) into_lane_1 = ticket; return 0; }) == 0);
  CHECK(q.admitted() == 2 && into_lane_1 == 2);
  q.retire(0, -2); q.retire(1, -2);                                                 // a failed round: its users retire with the round's status
  Done d[2];
  CHECK(q.occupied() == 0 && q.queued() == 1 && q.take_done(d, 2) == 2 && d[0].ticket == 1 && d[1].ticket == 2 && d[1].status == -2);
}

static void test_queue_grows() {
  Q q(3);
  const int n_users = 5000;
  for (int u = 0; u < n_users; ++u) q.submit(job(1 + u % 3));
  CHECK(q.queued() == n_users);
  std::vector<Done> done;
  std::set<int64_t> seen;
  int arrivals = 0;
  while (round_of(q, &done))
    if (arrivals < 100) { q.submit(job(2)); ++arrivals; }                           // users keep arriving while the queue is served
  for (const Done& d : done) CHECK(seen.insert(d.ticket).second);
  CHECK((int)seen.size() == n_users + arrivals && *seen.begin() == 1 && *seen.rbegin() == n_users + arrivals);
  CHECK(q.idle() && q.admitted() == n_users + arrivals && q.retired() == q.admitted());
}

// rounds of `need` users through `lanes` lanes, each free lane refilled at the round boundary
static int64_t rounds_refilled(const std::vector<int>& need, int lanes) {
  Q q(lanes);
  for (int r : need) q.submit(job(r));
  std::vector<Done> done;
  while (round_of(q, &done)) {}
  CHECK(done.size() == need.size());
  int64_t lane_rounds = 0;
  for (size_t i = 0; i < done.size(); ++i) {
    CHECK(done[i].rounds_in_lane == need[(size_t)done[i].ticket - 1]);
    lane_rounds += done[i].rounds_in_lane;
  }
  CHECK(lane_rounds == q.lane_rounds());
  return q.rounds();
}

static void test_replay_of_the_measured_round_counts() {
  // loop iterations per user of golden case k6_dk12_new7_gamma3_s9 over the prompts synth.synthetic_prompt(18 + 5 * (u % 7), 900 + u), u < 24
  const std::vector<int> need = {7, 6, 4, 5, 5, 5, 3, 4, 6, 7, 6, 4, 4, 4, 5, 3, 5, 5, 5, 5, 5, 6, 7, 5};
  int total = 0, chunked = 0;
  for (size_t i = 0; i < need.size(); ++i) total += need[i];
  for (size_t i = 0; i < need.size(); i += 4) {
    int slowest = 0;
    for (size_t j = i; j < i + 4; ++j) slowest = need[j] > slowest ? need[j] : slowest;
    chunked += slowest;
  }
  CHECK(total == 121 && chunked == 36);
  CHECK(rounds_refilled(need, 4) == 31);
  CHECK(rounds_refilled(need, 1) == 121);                                          // one lane: one user after the other
  CHECK(rounds_refilled(need, 24) == 7 && rounds_refilled(need, 64) == 7);          // a lane for everyone: the slowest user's rounds
}

int main() {
  test_submission_order_and_lane_reuse();
  test_empty_round_and_once_only();
  test_done_list_is_handed_out_in_pieces();
  test_admission_error_and_failed_round();
  test_queue_grows();
  test_replay_of_the_measured_round_counts();
  puts("session_queue ok");
  return 0;
}
