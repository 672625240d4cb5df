"""The parameter-edge workloads (tests/param_edges.py) reach the edges they are named for.

Everything here is read from the CPU oracle's record alone, so it runs without a GPU: if a
workload stopped reaching its edge (another seed, a changed rule), the GPU comparison in
tests/test_param_edges_gpu.py would still pass and prove nothing -- these fail instead.
"""
import numpy as np
import pytest

from tests import param_edges as pe

ALIVE = pe.ALIVE


def _ref(name):
    return pe.reference(name)


@pytest.mark.parametrize("name", sorted(pe.WORKLOADS))
def test_oracle_run_stays_short(name):
    """The GPU module re-runs every oracle workload: each stays under 5 s of oracle steps."""
    ref = _ref(name)
    print("%s: %.2f s in %d oracle steps" % (name, ref["seconds"], ref["w"]["ticks"]))
    assert len(ref["digest"]) == ref["w"]["ticks"] + 1
    assert ref["seconds"] < 5.0, "%s: %.2f s" % (name, ref["seconds"])


def test_every_parameter_end_is_visited():
    """The ends of validate_common's box, over the whole table."""
    kws = [w["kw"] for w in pe.WORKLOADS.values()]
    seen = lambda k, default: {kw.get(k, default) for kw in kws}
    assert {1, 2, 31} <= seen("tremove", 20)
    assert any(kw.get("tfail") == kw["tremove"] - 1 for kw in kws if "tremove" in kw)
    assert any(kw.get("tfail") == 1 for kw in kws)
    assert {1, 16} <= seen("fanout", 3) and {0, 100} <= seen("drop_pct", 0) and 8 in seen("swim", 0)
    assert {1, 2, 256} <= seen("view", None) and {0, 1, 7} <= seen("inbox", 7)
    assert {2, 9} <= {w["n"] for w in pe.WORKLOADS.values()}
    assert 2046 in seen("h0", 1)
    for w in pe.WORKLOADS.values():                     # h0 + max_ticks <= 2047 is admitted
        assert w["kw"].get("h0", 1) + w["ticks"] <= 2047
    assert {1, 2, 16, 30, 31, 32} <= set(pe.EDGE_LIMITS)


def test_hb_2047_fills_the_heartbeat_field():
    ref = _ref("hb_2047")
    hb, _ = pe.final_entries(ref)
    assert hb.size == 1100 * 1099 and (hb >= 1024).all()
    assert int((hb == 2047).sum()) == 8800 and hb.max() == 2047
    c = ref["census"][1]
    senders = {s for s, _ in ref["messages"][0]}
    assert len(senders) > 0 and int((c["max_hb"] == 2047).sum()) == len(senders)


@pytest.mark.parametrize("name", ["hb_top", "hb_top_swim", "pv_hb_top", "pv_hb_top_drain",
                                  "pv_hb_2046"])
def test_hb_top_workloads_reach_the_top_with_churn(name):
    ref = _ref(name)
    hb, _ = pe.final_entries(ref)
    assert 2040 <= hb.max() <= 2047
    assert pe.total(ref, "joins") > 0
    if name != "pv_hb_2046":                            # one tick: nothing is old enough yet
        assert pe.total(ref, "removes") > 0
    if ref["pview"]:
        assert pe.total(ref, "evicts") > 0
    if "census" in ref["w"]:
        assert int(ref["census"][ref["w"]["ticks"]]["max_hb"].max()) >= 2040


def test_hb_cross_has_both_sides_of_bit_15():
    hb, _ = pe.final_entries(_ref("hb_cross"))
    assert (hb < 1024).any() and (hb >= 1024).any()
    ref = _ref("hb_cross")
    assert pe.total(ref, "joins") > 0 and pe.total(ref, "removes") > 0


def test_tr31_ages_reach_30_past_the_wrap():
    ref = _ref("tr31")
    for t in (33, 36):
        c = ref["census"][t]
        f = c["fresh"]
        assert not np.array_equal(f[30], f[31]), "no live row holds an entry of age 30 at %d" % t
        assert not np.array_equal(f[16], f[30]), "ages 16..29 are empty at %d" % t
        assert (f[1] != f[2]).any()
        assert np.array_equal(f[31], f[32]) and np.array_equal(f[32], c["listed"])
    c20 = ref["census"][20]["fresh"]                    # before the wrap nothing is older than 20
    assert np.array_equal(c20[30], c20[32]) and not np.array_equal(c20[16], c20[30])
    assert pe.total(ref, "joins") > 0 and pe.total(ref, "removes") > 0
    assert ref["w"]["ticks"] > 64                       # two wraps of ts mod 32
    assert sum(len(e) for e in ref["events"][1:]) == pe.total(ref, "joins") + pe.total(ref, "removes")
    # reach: the age limit changes the graph somewhere
    r = ref["reach"][33]
    assert any(not np.array_equal(r[(1, d)][0], r[(32, d)][0]) for _, d in pe.DIRS)


def test_tr31_tf30_suspects_at_the_last_age():
    ref, plain = _ref("tr31_tf30"), _ref("tr31")
    assert ref["w"]["kw"]["tfail"] == ref["w"]["kw"]["tremove"] - 1
    assert ref["digest"] != plain["digest"]
    assert pe.total(ref, "removes") > 0 and pe.total(ref, "joins") > 0


def test_pv_tr31_census_and_reach_inputs():
    ref = _ref("pv_tr31_sw8")
    assert pe.total(ref, "evicts") > 0 and pe.total(ref, "overflow") > 0
    for t in (20, 33, 36):
        f = ref["census"][t]["fresh"]
        assert (f[1] != f[2]).any() and (f[2] != f[16]).any()
        assert np.array_equal(f[32], ref["census"][t]["listed"])
        r = ref["reach"][t]
        assert any(not np.array_equal(r[(1, d)][0], r[(32, d)][0]) for _, d in pe.DIRS)
    assert pe.total(_ref("pv_tr31_drain"), "evicts") > 0


@pytest.mark.parametrize("name", ["tr1", "pv_tr1"])
def test_tremove_1_empties_live_rows(name):
    ref = _ref(name)
    assert any((v[ref["fail"] >= t] == 0).any() for t, v in ref["lens"].items() if t > 0)
    assert pe.total(ref, "removes") > 0 and pe.total(ref, "joins") > 0
    live_rows = [r for r in range(ref["w"]["n"]) if ref["fail"][r] >= ref["w"]["ticks"]]
    t = ref["w"]["ticks"]
    snap = ref["snap"][t]
    for r in live_rows[::17]:                           # a live row keeps only this tick's entries
        row = snap.row(r)
        ts = row[2] if ref["pview"] else row[2][row[0].astype(bool)]
        assert (ts == t).all()


def test_tr2_tf1_sw8_holds_ages_0_and_1_only():
    ref = _ref("tr2_tf1_sw8")
    t = ref["w"]["ticks"]
    ages = set()
    for r, row in ref["snap"][t].rows.items():
        if ref["fail"][r] >= t:
            ages |= set((t - row[2][row[0].astype(bool)]).tolist())
    assert ages == {0, 1}
    assert pe.total(ref, "removes") > 0


def test_pv_tr2_row_lengths_span_the_view():
    ref = _ref("pv_tr2")
    lens = np.concatenate([v[ref["fail"] >= t] for t, v in ref["lens"].items() if t > 0])
    assert lens.min() == 0 and lens.max() == ref["w"]["kw"]["view"]
    assert pe.total(ref, "removes") > 0


def test_f16_and_tiny_deliver():
    assert _ref("f16")["digest"][-1]["delivered"] > 1100 * 8
    for name in ("tiny_n2", "tiny_n9", "pv_n2"):
        ref = _ref(name)
        assert ref["w"]["kw"]["fanout"] >= ref["w"]["n"] - 1
        assert all(d["delivered"] > 0 for d in ref["digest"][1:])


@pytest.mark.parametrize("name", ["drop100", "pv_drop100"])
def test_drop_100_delivers_nothing_and_empties_every_row(name):
    ref = _ref(name)
    n = ref["w"]["n"]
    assert all(d["delivered"] == 0 for d in ref["digest"][1:])
    assert all(d["sent"] == d["dropped"] for d in ref["digest"][1:])
    assert pe.total(ref, "removes") == (n * ref["w"]["kw"]["view"] if ref["pview"] else n * (n - 1))
    hb, _ = pe.final_entries(ref)
    assert hb.size == 0
    assert (ref["fail"] >= ref["w"]["ticks"]).all()     # with every node alive
    if name == "drop100":
        c = ref["census"][12]
        assert (c["state"] == ALIVE).all()
        assert not c["listed"].any() and not c["max_hb"].any()
        assert all(not f.any() for f in c["fresh"].values())


def test_small_views_evict_and_overflow():
    v1, v2 = _ref("pv_v1"), _ref("pv_v2_f16_k1")
    assert pe.total(v1, "evicts") == pe.total(v1, "joins") > 0
    assert pe.total(v2, "overflow") > 0 and pe.total(v2, "evicts") > 0
    big = _ref("pv_v256_f16_drain")
    assert big["w"]["kw"]["view"] == 256 and big["w"]["kw"]["inbox"] == 0
    assert pe.total(big, "evicts") > 0
    assert max(d["delivered"] for d in big["digest"][1:]) > 7 * big["w"]["n"]   # hub-size inboxes


def test_census_big_lists_ids_past_the_lds_cut():
    ref = _ref("pv_census_big")
    n, view = ref["w"]["n"], ref["w"]["kw"]["view"]
    assert n > 4096 and n * view > 2 * 256 * 1024       # two grid-stride passes at 256 CUs
    for t, c in ref["census"].items():
        assert c["listed"][4096:].any(), "no id >= 4096 is listed at tick %d" % t
        assert c["listed"][:4096].any()
    c = ref["census"][6]
    assert (c["fresh"][3] != c["listed"]).any() and c["max_hb"][4096:].max() > 1
