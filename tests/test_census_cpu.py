"""The membership census without a GPU: the struct mirror, the argument checks that run before
any device call, and Census.summary() on hand-made arrays."""
import ctypes

import numpy as np

from gossip_protocol_amd import _lib
from gossip_protocol_amd.census import ALIVE, CRASHED, NOT_STARTED, Census, default_age_limit


def test_census_info_layout():
    assert _lib.lib().gsp_struct_size(b"gsp_census_info") == ctypes.sizeof(_lib.GspCensusInfo)
    assert ctypes.sizeof(_lib.GspCensusInfo) == 32


def test_null_handle_is_invalid_and_named():
    L = _lib.lib()
    for name in ("gsp_scale_census", "gsp_pview_census"):
        rc = getattr(L, name)(None, 9, None, None, None, None, None)
        assert rc == -1, name
        assert name.encode() in L.gsp_last_error(), name


def test_summary_covers_every_field():
    # member:            0      1      2        3        4            5
    state = np.array([ALIVE, ALIVE, ALIVE, CRASHED, CRASHED, NOT_STARTED], np.uint8)
    # 0 and 1 are listed by both other alive nodes; 2 is an orphan; 3 is still listed by two
    # nodes (undetected); 4 has been removed by everyone; 5 has not started
    listed = np.array([2, 2, 0, 2, 0, 0], np.uint32)
    fresh = np.array([2, 1, 0, 0, 0, 0], np.uint32)
    max_hb = np.array([7, 6, 0, 3, 0, 0], np.uint32)
    c = Census(11, state, listed, fresh, max_hb, {"tick": 11, "alive": 3})
    assert c.tick == 11 and c.info["alive"] == 3
    assert c.summary() == {"tick": 11, "alive": 3, "crashed": 2, "undetected": 1, "stale_pairs": 2,
                           "orphans": 1, "missing_pairs": (2 - 2) + (2 - 2) + (2 - 0),
                           "max_listed": 2}
    full = Census(0, np.full(4, ALIVE, np.uint8), np.full(4, 3), np.full(4, 3), np.ones(4))
    assert full.summary() == {"tick": 0, "alive": 4, "crashed": 0, "undetected": 0, "stale_pairs": 0,
                              "orphans": 0, "missing_pairs": 0, "max_listed": 3}
    assert full.listed.dtype == np.uint32 and full.state.dtype == np.uint8


def test_default_age_limit_is_tfail_else_tremove():
    assert default_age_limit(_lib.GspScaleParams(tremove=9)) == 9
    assert default_age_limit(_lib.GspScaleParams(tremove=9, tfail=4)) == 4
    assert default_age_limit(_lib.GspPviewParams(tremove=20, tfail=0)) == 20
