"""The probe methods both scale engines have (gsp_scale_* / gsp_pview_* in
include/gossip/gossip.h), eight probes: census, view audit, overlay reach (single-source-set and
64-tree form), overlay clustering, overlay components, rumor trace, detection ledger and traffic
ledger.  The entry points differ only in their prefix, the class attribute `_abi`.
"""
from . import audit as _audit
from . import census as _census
from . import cluster as _cluster
from . import components as _components
from . import detect as _detect
from . import reach as _reach
from . import reach_multi as _reach_multi
from . import rumor as _rumor
from . import traffic as _traffic
from ._lib import check, lib


class ProbeMethods:
    """Mixin of ScaleEngine and PviewEngine; reads their _h, n and params."""

    _abi = None                # "gsp_scale" / "gsp_pview"
    _traffic_watch = ()        # the ids of the open traffic ledger's watch rows

    def _probe(self, name):
        """(entry point, its name for error messages)."""
        what = "%s_%s" % (self._abi, name)
        return getattr(lib(), what), what

    def _age_limit(self, age_limit):
        return _census.default_age_limit(self.params) if age_limit is None else age_limit

    def census(self, age_limit=None):
        """The membership census of the current tick (census.Census); age_limit (1..32) bounds
        `fresh`, default tfail if set, else tremove.  Collective across the ranks of a job."""
        fn, what = self._probe("census")
        return _census.run(fn, self._h, self.n, self._age_limit(age_limit), what)

    def audit(self, age_limit=None):
        """The view audit of the current tick (audit.Audit): per alive observer what its view
        holds and its fingerprint; age_limit (1..32) bounds `suspect`, default as for census().
        Collective across the ranks of a job."""
        fn, what = self._probe("audit")
        return _audit.run(fn, self._h, self.n, self._age_limit(age_limit), what)

    def reach(self, sources=0, direction="from", age_limit=None):
        """BFS hop counts over the membership graph of the current tick (reach.Reach), from
        (direction "from") or towards ("to") `sources`, an id or a sequence of ids; an edge is
        an entry younger than age_limit (1..32), default as for census().  Collective across
        the ranks of a job."""
        fn, what = self._probe("reach")
        return _reach.run(fn, self._h, self.n, sources, direction, self._age_limit(age_limit), what)

    def reach_multi(self, sources, direction="from", age_limit=None, hops=True, level_cap=256):
        """Up to 64 single-source BFS trees over the graph of reach() in one call
        (reach_multi.ReachMulti): row b of every array is reach(sources[b]).  hops=False leaves
        the [n_sources, n] matrix out; level_cap bounds level_sizes.  age_limit defaults as for
        reach().  Collective across the ranks of a job."""
        fn, what = self._probe("reach_multi")
        return _reach_multi.run(fn, self._h, self.n, sources, direction, self._age_limit(age_limit),
                                hops, level_cap, what)

    def cluster(self, observers, age_limit=None):
        """Overlay clustering of up to 64 observers over the graph of reach() (cluster.Cluster):
        per observer its out-degree, the links among its neighbours and the neighbours that list
        it back.  age_limit defaults as for census().  Collective across the ranks of a job."""
        fn, what = self._probe("cluster")
        return _cluster.run(fn, self._h, self.n, observers, self._age_limit(age_limit), what)

    def components(self, kind="strong", age_limit=None, max_sweeps=0):
        """The exact components of the graph of reach() (components.Components): kind "weak"
        (either endpoint lists the other) or "strong" (mutually reachable); every alive node is
        labelled with the smallest id of its component.  age_limit defaults as for reach();
        max_sweeps caps the table sweeps (0: the library's default), and a capped call comes back
        with converged False.  Collective across the ranks of a job."""
        fn, what = self._probe("components")
        return _components.run(fn, self._h, self.n, kind, self._age_limit(age_limit), max_sweeps, what)

    def rumor_open(self, rumors=32):
        """Open a rumor trace of `rumors` (1..32) independent rumors (rumor.py): from now on
        every tick also moves them one hop over the messages delivered (the partial view: over
        the messages merged -- a bounded inbox: its `inbox` smallest senders).  Collective."""
        fn, what = self._probe("rumor_open")
        _rumor.open_trace(fn, self._h, rumors, what)

    def rumor_seed(self, rumor, sources):
        """Give rumor `rumor` to `sources` (an id or a sequence) at the current tick; sources
        that are not alive are ignored.  Collective."""
        fn, what = self._probe("rumor_seed")
        _rumor.seed(fn, self._h, rumor, sources, what)

    def rumor(self, rumor=0):
        """rumor.Rumor of one rumor at the current tick.  Collective."""
        fn, what = self._probe("rumor_get")
        return _rumor.get(fn, self._h, self.n, self.params.max_ticks, rumor, what)

    def rumor_close(self):
        """Free the trace; step is back to the launches it makes without one.  Collective."""
        fn, what = self._probe("rumor_close")
        check(fn(self._h), what)

    def detect_open(self):
        """Open the detection ledger (detect.py; needs events with removes recorded): what the
        ring holds is folded now, and from now on every tick ends with one fold of its event
        records per member on the device, which empties the ring."""
        fn, what = self._probe("detect_open")
        check(fn(self._h), what)

    def detect(self):
        """detect.Detect of the open ledger at the current tick.  Collective."""
        fn, what = self._probe("detect_get")
        return _detect.get(fn, self._h, self.params, what)

    def detect_close(self):
        """Free the ledger; the ring is left empty and fills and drains as before.  Collective."""
        fn, what = self._probe("detect_close")
        check(fn(self._h), what)

    def traffic_open(self, watch=None):
        """Open the traffic ledger (traffic.py): from now on every tick counts, on the device,
        what each node sends, is sent, merges and loses to dead receivers.  watch: up to 1,024
        distinct node ids whose (sent, recv) are kept for every tick."""
        fn, what = self._probe("traffic_open")
        self._traffic_watch = _traffic.open_(fn, self._h, watch, what)

    def traffic(self):
        """traffic.Traffic of the open ledger at the current tick.  Collective."""
        fn, what = self._probe("traffic_get")
        return _traffic.get(fn, self._h, self.params, self._traffic_watch, what)

    def traffic_close(self):
        """Free the ledger; step is back to the launches it makes without one.  Collective."""
        fn, what = self._probe("traffic_close")
        check(fn(self._h), what)
