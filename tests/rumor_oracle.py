"""The rumor-trace rule (include/gossip/gossip.h "Rumor trace") in numpy, over the CPU oracle's
messages(), joinreps(), start_tick() and fail_tick() only -- never over engine output.

know[x] is a 32-bit mask; at tick t a receiver alive at t ORs in know_{t-1}[s] of the senders it
merges: per receiver the messages sorted by sender, a delivered JOINREP as sender -1 (it sorts
first and stands for node 0), the first K of them (all when K = 0).  Bits newly set give
heard[b][r] = t and count into known[b][t].

advance() is the rule for one tick on plain arrays; Trace carries a run (seeds, snapshots of what
gsp_*_rumor_get must return) and records what the workload exercised: the longest segment, the
(node, tick) pairs where the inbox cut withheld a new bit, and the JOINREPs that carried a rumor.
"""
import numpy as np

ALIVE = 1


def alive_at(start, fail, t):
    return (start <= t) & (t <= fail)


def states(start, fail, t):
    return np.where(t < start, 0, np.where(t <= fail, 1, 2)).astype(np.uint8)


def schedule(orc, n):
    """(start, fail) tick arrays of an oracle."""
    return (np.array([orc.start_tick(r) for r in range(n)], np.int64),
            np.array([orc.fail_tick(r) for r in range(n)], np.int64))


def advance(know_prev, t, src, dst, joiners, start, fail, K):
    """know of tick t and the tick's record.  src/dst: the GOSSIP pairs sent at t - 1 that
    survived; joiners: the destinations of the delivered JOINREPs of t - 1; K: inbox (0: all)."""
    know_prev = np.asarray(know_prev, np.uint32)
    n = know_prev.size
    s = np.concatenate([np.asarray(src, np.int64), np.full(len(joiners), -1, np.int64)])
    d = np.concatenate([np.asarray(dst, np.int64), np.asarray(joiners, np.int64)])
    order = np.lexsort((s, d))                       # by receiver, then sender
    s, d = s[order], d[order]
    first = np.searchsorted(d, d, side="left")       # index of the receiver's first message
    rank = np.arange(d.size) - first
    live = alive_at(start, fail, t)
    ok = live[d] if d.size else np.zeros(0, bool)
    keep = ok & ((rank < K) if K else np.ones(d.size, bool))
    word = know_prev[np.maximum(s, 0)] if d.size else np.zeros(0, np.uint32)
    got = np.zeros(n, np.uint32)
    np.bitwise_or.at(got, d[keep], word[keep])
    every = np.zeros(n, np.uint32)                   # what no cut would have let through
    np.bitwise_or.at(every, d[ok], word[ok])
    know = know_prev | got
    rec = {
        "longest": int(np.bincount(d, minlength=1).max()) if d.size else 0,
        "cut_withheld": int(((every & ~know) != 0).sum()),
        "joinrep_carried": int((keep & (s < 0) & (word != 0)).sum()),
    }
    return know, rec


class Trace:
    """A traced run: seed() between ticks, tick() per tick, snapshot() = what get returns."""

    def __init__(self, n, rumors, start, fail, K, opened_at=0):
        self.n, self.rumors, self.K = n, rumors, K
        self.start, self.fail = np.asarray(start, np.int64), np.asarray(fail, np.int64)
        self.t = opened_at
        self.opened_at = opened_at
        self.know = np.zeros(n, np.uint32)
        self.heard = np.full((rumors, n), -1, np.int32)
        self.known = [np.zeros(rumors, np.int64) for _ in range(opened_at + 1)]
        self.seed_tick = [-1] * rumors
        self.seeded = [set() for _ in range(rumors)]
        self.longest, self.cut_withheld, self.joinrep_carried = 0, 0, 0

    def _mark(self, before):
        new = self.know & ~before
        for b in range(self.rumors):
            rows = np.nonzero((new >> np.uint32(b)) & np.uint32(1))[0]
            self.heard[b, rows] = self.t
            self.known[self.t][b] += rows.size

    def seed(self, rumor, sources):
        live = alive_at(self.start, self.fail, self.t)
        src = [int(x) for x in np.atleast_1d(sources) if live[int(x)]]
        before = self.know.copy()
        if src:
            self.know[np.array(src)] |= np.uint32(1 << rumor)
            self.seeded[rumor].update(src)
            if self.seed_tick[rumor] < 0:
                self.seed_tick[rumor] = self.t
        self._mark(before)

    def tick(self, src, dst, joiners):
        self.t += 1
        self.known.append(np.zeros(self.rumors, np.int64))
        before = self.know
        self.know, rec = advance(before, self.t, src, dst, joiners, self.start, self.fail, self.K)
        self._mark(before)
        self.longest = max(self.longest, rec["longest"])
        self.cut_withheld += rec["cut_withheld"]
        self.joinrep_carried += rec["joinrep_carried"]

    def snapshot(self, rumor):
        """(heard, state, known[0..t], info) of one rumor at the current tick."""
        heard = self.heard[rumor].copy()
        state = states(self.start, self.fail, self.t)
        got = heard >= 0
        info = {"tick": self.t, "n": self.n, "rumor": rumor, "seed_tick": self.seed_tick[rumor],
                "sources": len(self.seeded[rumor]), "alive": int((state == ALIVE).sum()),
                "known": int(got.sum()), "known_alive": int((got & (state == ALIVE)).sum()),
                "last_heard": int(heard.max()) if got.any() else -1,
                "ticks_traced": self.t - self.opened_at}
        known = np.array([k[rumor] for k in self.known], np.int32)
        return heard, state, known, info


def run(orc, n, ticks, K, rumors, seeds, at):
    """Step `orc` from tick 0 to `ticks` with a trace opened at tick 0.  seeds: {tick: [(rumor,
    sources), ...]}, applied once the run stands at that tick; at: the ticks whose snapshots of
    every rumor are kept.  Returns the digests, the snapshots and the Trace."""
    start, fail = schedule(orc, n)
    tr = Trace(n, rumors, start, fail, K)
    ref = {"digest": [None], "at": {}, "trace": tr, "start": start, "fail": fail}
    for t in range(0, ticks + 1):
        if t:
            src, dst = orc.messages()                # sent at t - 1, merged at t
            joiners = orc.joinreps()
            ref["digest"].append(orc.step())
            tr.tick(src, dst, joiners)
        for rumor, sources in seeds.get(t, ()):
            tr.seed(rumor, sources)
        if t in at:
            ref["at"][t] = [tr.snapshot(b) for b in range(rumors)]
    return ref
