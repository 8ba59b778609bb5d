"""The forwards of a lock-step beam-SD call, restated from the round rule alone (beamSD.py:504-522): no torch, no library.  Two tests read it:
tests/test_staged_verify_gpu.py compares it with the forward logs of the engine, tests/test_round_plan_cpu.py with the replay that
tests/round_plan_check.cpp makes through atspeed_amd/csrc/round_plan.h."""


def expected_log(prompt_lens, accept_steps, gamma, new, k, dk, staged, t_star=None):
    """The target forwards of a lock-step call over users with these accepted steps per round, from the round rule alone (beamSD.py:504-522):
    -> ([(tokens, logit rows)], segments per forward, passes per user, draft-block counts gamma' per user and round).  With t_star a round
    is staged only when its packed forward would exceed that many tokens (the switch at 1)."""
    n = len(prompt_lens)
    st = [dict(gen=0, n0=prompt_lens[u], nb=1, r=0, done=False) for u in range(n)]
    log, segs, passes, dls = [], [], [0] * n, [[] for _ in range(n)]
    while not all(s["done"] for s in st):
        ver, fin = [], []
        for u, s in enumerate(st):
            if s["done"]:
                continue
            if s["gen"] >= new:
                s["done"] = True                      # its last verification produced the last token: export only
                continue
            dl = min(gamma, new - s["gen"] - 1)
            dls[u].append(dl)
            (ver if dl > 0 else fin).append((u, dl))
        if not ver and not fin:
            continue
        packed_tokens = sum(st[u]["n0"] + dl * dk for u, dl in ver) + sum(st[u]["n0"] for u, _ in fin)
        if not staged or not ver or (t_star is not None and packed_tokens <= t_star):
            log.append((packed_tokens, sum(st[u]["nb"] + dl * dk for u, dl in ver) + sum(st[u]["nb"] for u, _ in fin)))
            segs.append(len(ver) + len(fin))
            for u, _ in ver + fin:
                passes[u] += 1
        else:
            log.append((sum(st[u]["n0"] for u, _ in ver + fin), sum(st[u]["nb"] for u, _ in ver + fin)))
            segs.append(len(ver) + len(fin))
            for u, _ in ver + fin:
                passes[u] += 1
            for p in range(1, gamma + 1):             # block p: the users whose walk accepted steps 0 .. p - 1 and that drafted a block p
                alive = [u for u, dl in ver if dl >= p and accept_steps[u][st[u]["r"]] >= p]
                if not alive:
                    break
                log.append((len(alive) * dk, len(alive) * dk))
                segs.append(len(alive))
                for u in alive:
                    passes[u] += 1
        for u, _ in fin:
            st[u]["done"] = True
        for u, _ in ver:
            s = st[u]
            s["gen"] += accept_steps[u][s["r"]] + 1
            s["r"] += 1
            s["n0"] = s["nb"] = k
    return log, segs, passes, dls


def expected_draft_log(prompt_lens, accept_steps, gamma, new, k, dk):
    """The draft's forwards of the same call (one_step_beam_search, beamSD.py:108-179; a staged round drafts exactly as a packed one):
    -> ([(tokens, logit rows)], per user its (rounds run, tokens generated) after every round it took part in).  A round's step 0 takes, of
    every verifying user, its round inputs -- or, after a round that accepted every block, that block and the new beams (dk + k tokens,
    :402-416) -- and gives one logit row per beam; step i >= 1 takes dk tokens and gives dk rows per user that drafts more than i blocks."""
    n = len(prompt_lens)
    st = [dict(gen=0, n0=prompt_lens[u], nb=1, r=0, reingest=False) for u in range(n)]
    log, seq = [], [[] for _ in range(n)]
    live = list(range(n))
    while live:
        ver = [(u, min(gamma, new - st[u]["gen"] - 1)) for u in live if st[u]["gen"] < new]
        live = [u for u, dl in ver if dl > 0]         # dl == 0: the target's closing step, the user's last round
        for u, dl in ver:
            if dl == 0:
                st[u]["gen"] += 1
                seq[u].append((st[u]["r"], st[u]["gen"]))
        ver = [(u, dl) for u, dl in ver if dl > 0]
        for i in range(max([dl for _, dl in ver], default=0)):
            us = [u for u, dl in ver if dl > i]
            if i == 0:
                log.append((sum(dk + k if st[u]["reingest"] else st[u]["n0"] for u in us), sum(st[u]["nb"] for u in us)))
            else:
                log.append((len(us) * dk, len(us) * dk))
        for u, dl in ver:
            s = st[u]
            nm = accept_steps[u][s["r"]]
            s["gen"] += nm + 1
            s["r"] += 1
            s["n0"] = s["nb"] = k
            s["reingest"] = nm == dl
            seq[u].append((s["r"], s["gen"]))
    return log, seq
