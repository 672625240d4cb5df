"""The detection-ledger rule (include/gossip/gossip.h "Detection ledger") in numpy, over the CPU
oracle's per-tick events() with its fail_tick() / start_tick() only -- never over engine output.

A record is (kind, t, r, x): kind 1 join, 2 remove, 3 evict; r changed its list, x is the member.
With crash[x] the member's crash tick (INT32_MAX: never):
  remove, t >  crash[x]   true:   first_remove = min t, last_remove = max t, removers += 1
  remove, t <= crash[x]   false:  false_removes += 1, first_false = min t
  join,   t >  crash[x]   revivals += 1
  evict                   evicts += 1
and by_tick[t] counts the four classes by the record's tick.
"""
import numpy as np

JOIN, REMOVE, EVICT = 1, 2, 3
ARRAYS = ("first_remove", "last_remove", "removers", "false_removes", "first_false", "revivals",
          "evicts")
INFO = ("tick", "n", "open_tick", "kinds", "ticks_folded", "records", "lost", "true_removes",
        "false_removes", "joins", "revivals", "evicts")


def states(start, fail, t):
    return np.where(t < start, 0, np.where(t <= fail, 1, 2)).astype(np.uint8)


def schedule(orc, n):
    """(start, crash) tick arrays of an oracle."""
    return (np.array([orc.start_tick(r) for r in range(n)], np.int64),
            np.array([orc.fail_tick(r) for r in range(n)], np.int64))


class Ledger:
    """fold() takes record arrays; snapshot(T) is what gsp_*_detect_get must return at tick T."""

    def __init__(self, n, start, crash, span, opened_at=0, kinds=14):
        self.n, self.span, self.opened_at, self.kinds = n, span, opened_at, kinds
        self.start, self.crash = np.asarray(start, np.int64), np.asarray(crash, np.int64)
        self.first_remove = np.full(n, -1, np.int32)
        self.last_remove = np.full(n, -1, np.int32)
        self.first_false = np.full(n, -1, np.int32)
        self.removers, self.false_removes, self.revivals, self.evicts = (np.zeros(n, np.uint32) for _ in range(4))
        self.by_tick = np.zeros((span, 4), np.uint64)
        self.records = self.joins = 0

    @staticmethod
    def _min_into(dst, x, t):
        cur = np.where(dst < 0, np.iinfo(np.int32).max, dst).astype(np.int64)
        np.minimum.at(cur, x, t)
        dst[:] = np.where(cur == np.iinfo(np.int32).max, -1, cur).astype(np.int32)

    def fold(self, kind, t, x):
        kind, x = np.asarray(kind, np.int64), np.asarray(x, np.int64)
        t = np.broadcast_to(np.asarray(t, np.int64), kind.shape)
        keep = (self.kinds >> kind) & 1 == 1          # the kinds the engine records
        kind, t, x = kind[keep], t[keep], x[keep]
        after = t > self.crash[x]
        true, false = (kind == REMOVE) & after, (kind == REMOVE) & ~after
        revive, evict = (kind == JOIN) & after, kind == EVICT
        self._min_into(self.first_remove, x[true], t[true])
        np.maximum.at(self.last_remove, x[true], t[true].astype(np.int32))
        self._min_into(self.first_false, x[false], t[false])
        for dst, m in ((self.removers, true), (self.false_removes, false), (self.revivals, revive),
                       (self.evicts, evict)):
            np.add.at(dst, x[m], np.uint32(1))
        for c, m in enumerate((true, false, revive, evict)):
            np.add.at(self.by_tick[:, c], t[m], np.uint64(1))
        self.records += int(kind.size)
        self.joins += int((kind == JOIN).sum())

    def snapshot(self, T):
        out = {a: getattr(self, a).copy() for a in ARRAYS}
        out["state"] = states(self.start, self.crash, T)
        out["by_tick"] = self.by_tick[:T + 1].copy()
        out["info"] = {"tick": T, "n": self.n, "open_tick": self.opened_at, "kinds": self.kinds,
                       "ticks_folded": T - self.opened_at, "records": self.records, "lost": 0,
                       "true_removes": int(self.removers.astype(np.int64).sum()),
                       "false_removes": int(self.false_removes.astype(np.int64).sum()),
                       "joins": self.joins,
                       "revivals": int(self.revivals.astype(np.int64).sum()),
                       "evicts": int(self.evicts.astype(np.int64).sum())}
        return out


def run(orc, n, ticks, at=(), keep_r=True):
    """Step `orc` from tick 0 to `ticks` with a ledger opened at tick 0.  Keeps every tick's
    digest and records (kind, r, x; r = None unless keep_r), and the snapshots at the ticks `at`."""
    start, crash = schedule(orc, n)
    led = Ledger(n, start, crash, ticks + 1)
    ref = {"digest": [None], "events": [None], "at": {}, "start": start, "crash": crash, "ledger": led}
    for t in range(0, ticks + 1):
        if t:
            ref["digest"].append(orc.step())
            k, r, x = orc.events()
            ref["events"].append((k.astype(np.int8), r.copy() if keep_r else None, x.copy()))
            led.fold(k, t, x)
        if t in at:
            ref["at"][t] = led.snapshot(t)
    return ref


def ledger_over(ref, n, ticks, lo, hi, kinds=14):
    """A ledger of the recorded ticks lo..hi (inclusive), opened at tick `lo - 1` or earlier."""
    led = Ledger(n, ref["start"], ref["crash"], ticks + 1, kinds=kinds)
    for t in range(lo, hi + 1):
        k, _, x = ref["events"][t]
        led.fold(k, t, x)
    return led


def pack(kind, t, r, x):
    """The 64-bit records of the event ring."""
    return ((np.asarray(kind, np.uint64) << np.uint64(62)) | (np.asarray(t, np.uint64) << np.uint64(42))
            | (np.asarray(r, np.uint64) << np.uint64(21)) | np.asarray(x, np.uint64))
