// Stand-alone check of atspeed_amd/csrc/round_plan.h (the host-only arithmetic of a beam-SD round): tests/test_round_plan_cpu.py compiles
// this with -fsanitize=address,undefined and runs it.  Every CHECK that fails prints its line and the program exits 1.
//   round_plan_check                                   the placed cases (literals of the formulas the header replaced, partition, capacity);
//                                                      "round_plan ok" ends a clean run
//   round_plan_check GAMMA NEW K DK  P:a,b,..  P:a,..  a lock-step call of users with prompt length P and accepted steps a, b, .. per round,
//                                                      replayed as bssd_round does it: prints the target's forwards (packed, staged), the
//                                                      draft's, and every user's (rounds run, tokens generated) after each of its rounds
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "round_plan.h"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

using namespace ats_round;
static const int MAXB = 64;                      // ATSPEED_MAX_BEAMS

static bool same(const Span& s, int row0, int n_tok, int n_slots, int n_logit) {
  return s.row0 == row0 && s.n_tok == n_tok && s.n_slots == n_slots && s.n_logit == n_logit;
}

// the placed user of a first round and of a later one, dl = 0 .. 3
static void placed(User u) {
  const int n0 = u.n0, nb = u.nb, base = u.base, dk = u.dk;
  for (int dl = 0; dl <= 3; ++dl) {
    const Span all = span(u, 0, dl);
    CHECK(same(all, 0, n0 + dk * dl, base + n0 + dk * dl, nb + dk * dl));
    CHECK(same(span(u, 0, 0), 0, n0, base + n0, nb));
    // partition: the one-block spans tile the packed span's token rows and logit rows; their slot counts grow up to the packed count
    int tok = 0, rows = 0, slots = 0;
    for (int p = 0; p <= dl; ++p) {
      const Span s = span(u, p, p);
      if (p >= 1) CHECK(same(s, n0 + dk * (p - 1), dk, base + n0 + dk * p, dk));
      CHECK(s.row0 == tok && logit_row(u, 0, p) == rows && logit_row(u, p, p) == 0 && s.n_slots > slots);
      CHECK(s.n_slots == u.base + s.row0 + s.n_tok);             // a segment sees the kept past and its own rows
      tok += s.n_tok; rows += s.n_logit; slots = s.n_slots;
      CHECK(beam_row0(u, p) == s.row0 + s.n_tok - s.n_logit);    // the beams are a block's last rows
      const Blocks st = phase_blocks(true, p, dl), pk = phase_blocks(false, p, dl);
      CHECK(st.b0 == p && st.b1 == p && pk.b0 == 0 && pk.b1 == dl);
    }
    CHECK(tok == all.n_tok && rows == all.n_logit && slots == all.n_slots);
  }
}

static void placed_cases() {
  User u{23, 1, 5, 6, 12, 0, false};
  placed(u);
  CHECK(same(span(u, 0, 3), 0, 59, 64, 37) && same(span(u, 2, 2), 35, 12, 52, 12) && logit_row(u, 0, 3) == 25 && beam_row0(u, 0) == 22);
  CHECK(same(reingest_span(u), 0, 18, 28, 1));
  advance(u, 2, 3);                                              // two of three blocks accepted
  CHECK(u.base == 5 + 23 + 24 && u.n0 == 6 && u.nb == 6 && u.gen == 3 && !u.reingest && u.k == 6 && u.dk == 12);
  placed(u);
  CHECK(same(span(u, 0, 3), 0, 42, 94, 42) && same(span(u, 1, 1), 6, 12, 70, 12) && logit_row(u, 0, 2) == 18 && beam_row0(u, 0) == 0);
  advance(u, 3, 3);
  CHECK(u.base == 52 + 6 + 36 && u.gen == 7 && u.reingest);
  // what a user does in a round (gamma 3, 7 new tokens)
  const int gens[] = {0, 3, 4, 5, 6, 7, 8}, dls[] = {3, 3, 2, 1, 0, 0, 0};
  const Kind kinds[] = {VERIFY, VERIFY, VERIFY, VERIFY, FINAL_STEP, EXPORT_ONLY, EXPORT_ONLY};
  for (int i = 0; i < 7; ++i) { const Start s = classify(gens[i], 7, 3); CHECK(s.kind == kinds[i] && s.dl == dls[i]); }
  CHECK(classify(0, 1, 3).kind == FINAL_STEP && classify(0, 9, 1).dl == 1);
  // capacity: 4 users of 23 prompt tokens, gamma 3, k 6, dk 12; short prompts count as k; a target-only call has no draft blocks
  const int n0[4] = {23, 23, 23, 23}, tiny[2] = {2, 30};
  const Capacity c = worst_round(n0, 4, 3, 6, 12, MAXB);
  CHECK(c.t_tok == 236 && c.t_rows == 400 && c.d_tok == 92 && c.d_rows == 256);
  const Capacity s = worst_round(tiny, 2, 3, 6, 12, MAXB), t = worst_round(tiny, 2, 0, 6, 6, MAXB);
  CHECK(s.t_tok == 6 + 30 + 72 && s.d_tok == 18 + 30 && t.t_tok == 36 && t.t_rows == 128);
  CHECK(call_slots(23, 7, 12) == 95 && call_slots(23, 1, 12) == 23);
}

// ---- the replay
struct Sim {
  User u;
  std::vector<int> acc;          // accepted steps per round
  int P = 0, n_run = 0, dl = 0;
  bool done = false;
  std::string seq;
};
struct Log {
  std::string s;
  void add(int tok, int rows) { s += " " + std::to_string(tok) + "," + std::to_string(rows); }
};

static void replay(int gamma, int max_new, int dk, std::vector<Sim> us, bool staged, const Capacity& cap, Log& tlog, Log& dlog) {
  for (;;) {
    std::vector<Sim*> ver, fin;
    for (Sim& s : us) {
      if (s.done) continue;
      const Start st = classify(s.u.gen, max_new, gamma);
      if (st.kind == EXPORT_ONLY) { s.done = true; continue; }
      s.dl = st.dl;
      (st.kind == VERIFY ? ver : fin).push_back(&s);
    }
    if (ver.empty() && fin.empty()) break;
    // draft: step i of every user that drafts more than i blocks
    for (int i = 0;; ++i) {
      int tok = 0, rows = 0;
      for (Sim* s : ver) if (s->dl > i) {
        const Span sp = span(s->u, i, i);
        const Span in = (i == 0 && s->u.reingest) ? reingest_span(s->u) : sp;
        CHECK(in.n_slots == sp.n_slots && in.n_logit == sp.n_logit);
        tok += in.n_tok; rows += in.n_logit;
      }
      if (tok == 0) break;
      CHECK(tok <= cap.d_tok && rows <= cap.d_rows);
      dlog.add(tok, rows);
    }
    // target: phases over the users whose walk is pending
    std::vector<Sim*> pend = ver;
    int row_off = 0;
    for (int p = 0;; ++p) {
      int tok = 0, rows = 0;
      bool more = false;
      for (Sim* s : pend) {
        const Blocks ph = phase_blocks(staged, p, s->dl);
        const Span sp = span(s->u, ph.b0, ph.b1);
        CHECK(sp.n_slots <= call_slots(s->P, max_new, dk));          // the bound a session checks at submission holds in every round
        tok += sp.n_tok; rows += sp.n_logit;
        more = more || ph.b1 < s->dl;
      }
      if (p == 0) for (Sim* s : fin) { const Span sp = span(s->u, 0, 0); tok += sp.n_tok; rows += sp.n_logit; }
      CHECK(tok <= cap.t_tok && row_off + rows <= cap.t_rows);
      tlog.add(tok, rows);
      if (!more) break;
      std::vector<Sim*> next;
      for (Sim* s : pend) if (s->acc.at((size_t)s->n_run) >= p + 1) next.push_back(s);   // its walk accepted steps 0 .. p and needs block p + 1
      row_off += rows;
      pend.swap(next);
      if (pend.empty()) break;
    }
    for (Sim* s : fin) {
      s->u.gen += 1; s->done = true;
      s->seq += " " + std::to_string(s->n_run) + "," + std::to_string(s->u.gen);
    }
    for (Sim* s : ver) {
      const int nm = s->acc.at((size_t)s->n_run);
      CHECK(nm >= 0 && nm <= s->dl);
      advance(s->u, nm, s->dl);
      s->n_run++;
      s->seq += " " + std::to_string(s->n_run) + "," + std::to_string(s->u.gen);
    }
  }
  if (!staged) for (size_t i = 0; i < us.size(); ++i) printf("user%zu%s\n", i, us[i].seq.c_str());
}

int main(int argc, char** argv) {
  if (argc == 1) {
    placed_cases();
    printf("round_plan ok\n");
    return 0;
  }
  CHECK(argc >= 6);
  const int gamma = atoi(argv[1]), max_new = atoi(argv[2]), k = atoi(argv[3]), dk = atoi(argv[4]);
  std::vector<Sim> us;
  std::vector<int> n0;
  for (int a = 5; a < argc; ++a) {
    Sim s{};
    char* p = nullptr;
    const int P = (int)strtol(argv[a], &p, 10);
    CHECK(P >= 1 && *p == ':');
    while (*p == ':' || *p == ',') s.acc.push_back((int)strtol(p + 1, &p, 10));
    s.u = User{P, 1, 0, k, dk, 0, false};
    s.P = P;
    us.push_back(s);
    n0.push_back(P);
  }
  const Capacity cap = worst_round(n0.data(), (int)n0.size(), gamma, k, dk, MAXB);
  Log packed, staged, draft, draft_again;
  replay(gamma, max_new, dk, us, false, cap, packed, draft);
  replay(gamma, max_new, dk, us, true, cap, staged, draft_again);
  CHECK(draft.s == draft_again.s);                   // a staged round drafts exactly as a packed one
  printf("packed%s\nstaged%s\ndraft%s\n", packed.s.c_str(), staged.s.c_str(), draft.s.c_str());
  return 0;
}
