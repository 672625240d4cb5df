"""The traffic-ledger rule (include/gossip/gossip.h "Traffic ledger") in numpy, over the CPU
oracle's messages(), joinreps(), start_tick(), fail_tick(), row() and step() digests only -- never
over engine output.

A message sent at t - 1 arrives at t.  Per receiver the arrivals are sorted by sender, a delivered
JOINREP as sender -1 (it sorts first and stands for node 0).  A receiver alive at t counts them
all as recv and merges the first K of them (all when K = 0); a receiver that is not alive counts
them as lost.  A merged GOSSIP from s costs 1 + size[s] entries, size[s] = s's gossipable members at
t - 1 (with TFAIL: listed and (t - 1) - ts < tfail); a merged JOINREP costs 1 + min(intro_list,
size[0]).  The sends of t are the oracle's messages() after its step to t, plus one per delivered
JOINREP for node 0.

arrivals() / account() are the rule for one tick on plain arrays; Ledger carries a run (snapshots
of what gsp_*_traffic_get must return) and records what the workload exercised.
"""
import numpy as np

BUCKETS = 18
ALIVE = 1
INFO = ("tick", "n", "open_tick", "ticks_counted", "n_watch", "sent", "recv", "merged", "lost", "entries",
        "overflow", "max_fanin", "max_fanin_node")


def alive_at(start, fail, t):
    return (start <= t) & (t <= fail)


def states(start, fail, t):
    return np.where(t < start, 0, np.where(t <= fail, 1, 2)).astype(np.uint8)


def schedule(orc, n):
    return (np.array([orc.start_tick(r) for r in range(n)], np.int64),
            np.array([orc.fail_tick(r) for r in range(n)], np.int64))


def bucket_of(k):
    """0 for k = 0, else b with 2^(b-1) <= k < 2^b, the last bucket open-ended (exact integers)."""
    k = np.asarray(k, np.int64)
    b = np.zeros(k.shape, np.int64)
    for i in range(1, 40):
        b[k >= (1 << (i - 1))] = i
    return np.minimum(b, BUCKETS - 1)


def arrivals(t, src, dst, joiners, start, fail, K):
    """(sender, receiver, alive-receiver flag, merged flag) of the messages that arrive at t."""
    s = np.concatenate([np.asarray(src, np.int64), np.full(len(joiners), -1, np.int64)])
    d = np.concatenate([np.asarray(dst, np.int64), np.asarray(joiners, np.int64)])
    order = np.lexsort((s, d))                       # by receiver, then sender
    s, d = s[order], d[order]
    rank = np.arange(d.size) - np.searchsorted(d, d, side="left")
    ok = alive_at(start, fail, t)[d] if d.size else np.zeros(0, bool)
    keep = ok & ((rank < K) if K else np.ones(d.size, bool))
    return s, d, ok, keep


def account(n, t, arr, size, intro_list, start, fail):
    """The tick's per-node (recv, merged, lost, entries) from arrivals(); size[s]: payload entries
    of a GOSSIP from s (read for merged senders only; node 0's for a JOINREP)."""
    s, d, ok, keep = arr
    recv = np.bincount(d[ok], minlength=n).astype(np.int64)
    lost = np.bincount(d[~ok], minlength=n).astype(np.int64)
    merged = np.bincount(d[keep], minlength=n).astype(np.int64)
    ks, kd = s[keep], d[keep]
    pay = np.array([min(intro_list, size[0]) if x < 0 else size[int(x)] for x in ks], np.int64)
    entries = np.zeros(n, np.int64)
    np.add.at(entries, kd, 1 + pay)
    return recv, merged, lost, entries


class Ledger:
    """A run's ledger opened at `opened_at`: tick() per tick, snapshot() = what get returns."""

    def __init__(self, n, start, fail, K, intro_list, span, opened_at=0, watch=()):
        self.n, self.K, self.intro_list, self.span = n, K, intro_list, span
        self.start, self.fail = np.asarray(start, np.int64), np.asarray(fail, np.int64)
        self.t = self.opened_at = opened_at
        z = lambda: np.zeros(n, np.int64)
        self.sent, self.recv, self.merged, self.lost, self.entries = z(), z(), z(), z(), z()
        self.peak, self.peak_tick = z(), np.full(n, -1, np.int64)
        self.by_tick = np.zeros((span, 6), np.int64)
        self.fanin = np.zeros((span, BUCKETS), np.int64)
        self.watch_ids = np.asarray(watch, np.int64)
        self.watch = np.zeros((len(self.watch_ids), span, 2), np.int64)
        # what the workload exercised
        self.longest = self.joinreps_merged = self.cut_payloads = 0

    def tick(self, arr, size, sent_src, sent_joinreps, listed=None):
        """arr: arrivals() of the new tick; size: payload sizes at the send tick; sent_src /
        sent_joinreps: the GOSSIP senders and the delivered JOINREPs of the new tick's sends;
        listed[s]: the entries s listed (recorded against size: what TFAIL left out)."""
        self.t += 1
        t, n = self.t, self.n
        recv, merged, lost, entries = account(n, t, arr, size, self.intro_list, self.start, self.fail)
        sent = np.bincount(np.asarray(sent_src, np.int64), minlength=n).astype(np.int64)
        sent[0] += sent_joinreps
        self.sent += sent
        self.recv += recv
        self.merged += merged
        self.lost += lost
        self.entries += entries
        up = recv > self.peak
        self.peak[up], self.peak_tick[up] = recv[up], t
        self.by_tick[t] = [sent.sum(), recv.sum(), merged.sum(), lost.sum(), entries.sum(), recv.max()]
        live = alive_at(self.start, self.fail, t)
        self.fanin[t] = np.bincount(bucket_of(recv[live]), minlength=BUCKETS)
        if len(self.watch_ids):
            self.watch[:, t, 0], self.watch[:, t, 1] = sent[self.watch_ids], recv[self.watch_ids]
        s, d, ok, keep = arr
        self.longest = max(self.longest, int(np.bincount(d, minlength=1).max()) if d.size else 0)
        self.joinreps_merged += int((keep & (s < 0)).sum())
        if listed is not None:
            self.cut_payloads += sum(1 for x in set(s[keep & (s >= 0)].tolist()) if size[x] < listed[x])

    def snapshot(self):
        t = self.t
        top = int(self.peak.max())
        node = -1
        if top > 0:
            cand = np.nonzero(self.peak == top)[0]
            node = int(cand[np.lexsort((cand, self.peak_tick[cand]))[0]])
        info = {"tick": t, "n": self.n, "open_tick": self.opened_at, "ticks_counted": t - self.opened_at,
                "n_watch": len(self.watch_ids), "sent": int(self.sent.sum()), "recv": int(self.recv.sum()),
                "merged": int(self.merged.sum()), "lost": int(self.lost.sum()),
                "entries": int(self.entries.sum()), "overflow": int((self.recv - self.merged).sum()),
                "max_fanin": top, "max_fanin_node": node}
        return {"sent": self.sent.copy(), "recv": self.recv.copy(), "merged": self.merged.copy(),
                "lost": self.lost.copy(), "entries_in": self.entries.copy(), "peak_recv": self.peak.copy(),
                "peak_tick": self.peak_tick.copy(), "state": states(self.start, self.fail, t),
                "by_tick": self.by_tick[:t + 1].copy(), "fanin": self.fanin[:t + 1].copy(),
                "watch": self.watch[:, :t + 1].copy(), "info": info}


def payload_sizes(orc, kind, senders, t_sent, tfail):
    """({s: gossipable entries}, {s: listed entries}) of `senders` from the oracle's rows, which
    must stand at tick t_sent."""
    size, listed = {}, {}
    for s in senders:
        row = orc.row(int(s))
        if kind == "pview":
            ts = row[2].astype(np.int64)
            have = np.ones(ts.size, bool)
        else:
            ts = row[2].astype(np.int64)
            have = row[0].astype(bool)
        listed[int(s)] = int(have.sum())
        size[int(s)] = int((have & ((t_sent - ts) < tfail)).sum()) if tfail else listed[int(s)]
    return size, listed


def run(orc, kind, n, ticks, K, tfail, intro_list, at, opened_at=0, watch=()):
    """Step `orc` from tick 0 to `ticks` with a ledger opened at `opened_at`; at: the ticks whose
    snapshots are kept.  Returns the digests, the snapshots, the Ledger and the schedule."""
    start, fail = schedule(orc, n)
    led = Ledger(n, start, fail, K, intro_list, ticks + 1, opened_at, watch)
    ref = {"digest": [None], "at": {}, "ledger": led, "start": start, "fail": fail}
    if opened_at in at:
        ref["at"][opened_at] = led.snapshot()
    for t in range(1, ticks + 1):
        src, dst = orc.messages()                    # sent at t - 1, taken at t
        joiners = orc.joinreps()
        arr = arrivals(t, src, dst, joiners, start, fail, K)
        size = listed = None
        if t > opened_at:                            # the senders' rows while they stand at t - 1
            s, keep = arr[0], arr[3]
            need = set(s[keep & (s >= 0)].tolist()) | ({0} if (keep & (s < 0)).any() else set())
            size, listed = payload_sizes(orc, kind, sorted(need), t - 1, tfail)
        ref["digest"].append(orc.step())
        if t <= opened_at:
            continue
        led.tick(arr, size, orc.messages()[0], len(orc.joinreps()), listed)
        if t in at:
            ref["at"][t] = led.snapshot()
    return ref


# ---- the oracle workloads the CPU and GPU tests share (the shapes of tests/test_rumor_gpu.py) ----
FAIL_RANDOM = 1
_A = dict(view=32, fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=50000, seed=4128)
WORKLOADS = {
    # n = 3000 in 2,048-column tiles: a ragged second tile of 952 nodes; crashes at tick 2
    ("full", "main"): dict(n=3000, ticks=40, at=(0, 1, 12, 25, 40), pol=None,
                           kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000,
                                   seed=3003)),
    # node i starts at int(0.05 i): 599 starts at tick 29
    ("full", "join"): dict(n=600, ticks=35, at=(0, 5, 20, 35), pol=dict(step_rate=0.05, intro_list=8),
                           kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000,
                                   seed=600)),
    # node i starts at int(0.01 i): 100 nodes per tick, whose JOINREQ answers land on node 0
    ("full", "burst"): dict(n=600, ticks=20, at=(1, 3, 8, 20), pol=dict(step_rate=0.01, intro_list=8),
                            kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000,
                                    seed=600)),
    ("full", "variants"): dict(n=1024, ticks=13, at=(6, 13), pol=None,
                               kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                                       fail_ppm=20000, seed=3003, tfail=4, swim=2)),
    ("pview", "A7"): dict(n=4096, ticks=40, at=(0, 1, 12, 25, 40), pol=None, kw=dict(inbox=7, **_A)),
    ("pview", "A2"): dict(n=4096, ticks=40, at=(12, 40), pol=None, kw=dict(inbox=2, **_A)),
    ("pview", "A0"): dict(n=4096, ticks=40, at=(12, 40), pol=None, kw=dict(inbox=0, **_A)),
    ("pview", "B"): dict(n=1000, ticks=40, at=(12, 40), pol=None,
                         kw=dict(view=64, fanout=3, inbox=0, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                                 fail_ppm=50000, seed=1064)),
    # node i starts at int(0.02 i): 250 at tick 5, the last joiner 1199 at tick 23
    ("pview", "join"): dict(n=1200, ticks=40, at=(6, 20, 30, 40), pol=dict(step_rate=0.02, intro_list=8),
                            kw=dict(view=32, fanout=3, inbox=3, tremove=9, fail_mode=FAIL_RANDOM,
                                    fail_tick=10, fail_ppm=30000, seed=77)),
    # TFAIL: the payload sizes come from the sizing pass, not from the row lengths
    ("pview", "tfail"): dict(n=1024, ticks=24, at=(1, 8, 16, 24), pol=None,
                             kw=dict(view=32, fanout=3, inbox=3, tremove=9, tfail=4, fail_mode=FAIL_RANDOM,
                                     fail_tick=2, fail_ppm=50000, seed=1024)),
}


def watch_of(w):
    """The watched nodes of a workload: node 0, the ends, a few in between -- more than 67 of
    them, so that write_msgcount reaches the node-67 layout."""
    n = w["n"]
    return sorted({0, 1, n // 2, n - 2, n - 1} | set(range(3, n, max(1, n // 70))))


def make_oracle(kind, name):
    from tests.oracle_binding import PviewOracle, ScaleOracle, make_policy
    w = WORKLOADS[kind, name]
    pol = make_policy(**w["pol"]) if w["pol"] else None
    return (PviewOracle if kind == "pview" else ScaleOracle)(w["n"], policy=pol, **w["kw"])


_REFS = {}


def reference(kind, name):
    """The workload's oracle run with a ledger opened at tick 0, computed once per process."""
    if (kind, name) not in _REFS:
        w = WORKLOADS[kind, name]
        orc = make_oracle(kind, name)
        _REFS[kind, name] = run(orc, kind, w["n"], w["ticks"], w["kw"].get("inbox", 0), w["kw"].get("tfail", 0),
                                (w["pol"] or {}).get("intro_list", 0), set(w["at"]), 0, watch_of(w))
        orc.close()
    return _REFS[kind, name]
