// Host-only arithmetic of a beam-SD round (beamSD.py:458-542): what a user does in a round, which rows of its token buffer a forward takes,
// where a walk finds a block's logit rows, what a round leaves behind, and how large the worst round is.  No HIP call and no device type in
// here, plain ints in and out: the engine (engine.hip, bssd_round and the entry points around it) is the only includer, and
// tests/test_round_plan_cpu.py compiles this header into a stand-alone program under the address and undefined-behaviour sanitizers.
//
// A user's token buffer holds, per round, its ROUND INPUTS (block 0: n0 token rows, the last nb of them the round's beams, one logit row per
// beam) and behind them the draft's blocks 1 .. dl (dk token rows and dk logit rows each); its KV slots below `base` are the kept past.
#pragma once
#include <algorithm>

namespace ats_round {

// ---- what a user does in the round that starts now (beamSD.py:504-509): its last verification produced the last token (nothing but the
// export is left), one closing beam step of the target alone, or a verification of dl draft blocks
enum Kind { EXPORT_ONLY, FINAL_STEP, VERIFY };
struct Start { Kind kind; int dl; };
inline Start classify(int gen, int max_new, int gamma) {
  if (gen >= max_new) return Start{EXPORT_ONLY, 0};
  const int dl = std::min(gamma, max_new - gen - 1);
  return Start{dl == 0 ? FINAL_STEP : VERIFY, dl};
}

// ---- a user between two rounds
struct User {
  int n0, nb, base, k, dk;     // round inputs: token rows / beams among them; KV slots kept below them; target / draft beam size
  int gen; bool reingest;      // tokens generated so far; the last round accepted every block (the draft's step 0 takes reingest_span)
};

// token rows / logit rows in front of block b
inline int tok_before(const User& u, int b) { return b == 0 ? 0 : u.n0 + (b - 1) * u.dk; }
inline int rows_before(const User& u, int b) { return b == 0 ? 0 : u.nb + (b - 1) * u.dk; }

// blocks b0 .. b1 as one segment of a forward: the first token row, the token count, the KV slots the segment sees and its logit rows.
// A draft step, a final step and a staged phase are span(b, b); a packed verification is span(0, dl).
struct Span { int row0, n_tok, n_slots, n_logit; };
inline Span span(const User& u, int b0, int b1) {
  return Span{tok_before(u, b0), tok_before(u, b1 + 1) - tok_before(u, b0), u.base + tok_before(u, b1 + 1), rows_before(u, b1 + 1) - rows_before(u, b0)};
}
// block b's first logit row, counted from the first logit row of a span that starts at block b0 <= b
inline int logit_row(const User& u, int b0, int b) { return rows_before(u, b) - rows_before(u, b0); }
// the first token row of the beams that block b's logit rows belong to: the last nb round inputs, every row of a draft block
inline int beam_row0(const User& u, int b) { return b == 0 ? u.n0 - u.nb : tok_before(u, b); }
// the draft's step 0 after a round that accepted everything: where span(0, 0) stands otherwise, its own last block and the new beams
// (dk + k rows of a buffer of their own, beamSD.py:402-416)
inline Span reingest_span(const User& u) { return Span{0, u.dk + u.k, u.base + u.n0, u.nb}; }

// the blocks phase p of a verification forwards for a user that drafted dl blocks: packed, one phase holds them all; staged, phase p holds block p
struct Blocks { int b0, b1; };
inline Blocks phase_blocks(bool staged, int p, int dl) { return staged ? Blocks{p, p} : Blocks{0, dl}; }

// ---- the round's end: the walk accepted nm of dl blocks (beamSD.py:522).  Everything up to the end of block nm is kept, the k new beams
// are the next round's inputs
inline void advance(User& u, int nm, int dl) {
  u.base += u.n0 + nm * u.dk;
  u.n0 = u.nb = u.k;
  u.gen += nm + 1;
  u.reingest = nm == dl;
}

// ---- capacity.  The largest forwards a round of these users can ask of the two models: tokens and logit rows, target and draft (a
// target-only call: gamma = 0).  n0[u]: the longest round inputs user u can have, i.e. its prompt; max_beams: ATSPEED_MAX_BEAMS
struct Capacity { int t_tok, t_rows, d_tok, d_rows; };
inline Capacity worst_round(const int* n0, int n, int gamma, int k, int dk, int max_beams) {
  Capacity c{0, 0, 0, n * max_beams};
  for (int u = 0; u < n; ++u) {
    c.t_tok += std::max(n0[u], k) + gamma * dk;
    c.t_rows += max_beams + gamma * dk;
    c.d_tok += std::max(n0[u], dk + k);
  }
  return c;
}
// KV slots: a round's verification of dl blocks reaches span(0, dl).n_slots; a whole call can reach (every draft block of every round kept)
inline int call_slots(int prompt_len, int max_new, int dk) { return prompt_len + (max_new - 1) * dk; }

}  // namespace ats_round
