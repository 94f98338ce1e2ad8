"""The option keys of quber_set_option / quber_get_option: the key -> field table of csrc/runtime.hip against include/quber_hip.h."""
import os

import pytest

from quber_amd import _lib, arch, engine

pytestmark = pytest.mark.gpu

# key -> default, written out from include/quber_hip.h (never derived from the library under test)
DEFAULTS = {3: 0, 4: 0, 5: 1, 6: 0, 7: 32, 8: 67, 9: 0, 10: 32, 13: 1, 14: 32, 15: 256, 16: 0, 17: 0, 18: 1, 19: 1, 20: 0, 21: 2, 24: 1,
            25: 1, 27: 160, 29: 1, 30: 1, 31: 1, 32: 224, 35: 1, 36: 2, 37: 8, 38: 1, 39: 1, 41: 1, 42: 1, 43: 1}
# the keys that shape the plan: refused once quber_finalize_weights has built it (31 and 38 are read at launch too and stay settable)
PLAN_TIME = (6, 7, 8, 9, 10, 18, 25, 27, 29, 39, 41)


def options(eng):
    return {k: eng.get_option(k) for k in DEFAULTS}


def test_option_defaults_and_round_trip():
    assert len(DEFAULTS) == 32
    eng = engine.Engine(engine.make_config(height=32, width=32, with_network=False), "cuda:0")       # nothing is planned
    try:
        env_keys = ({6, 9} if "QUBER_WINOGRAD" in os.environ else set()) | ({13} if "QUBER_PERSIST" in os.environ else set())      # _lib.load() writes these process defaults
        got = options(eng)
        for k, v in DEFAULTS.items():
            if k not in env_keys:
                assert got[k] == v, f"default of key {k}"
        for k in DEFAULTS:
            before = options(eng)
            eng.set_option(k, 1000 + k)
            after = options(eng)
            assert after.pop(k) == 1000 + k and before.pop(k) != 1000 + k
            assert after == before, f"set_option({k}) moved another key"
            eng.set_option(k, got[k])
        assert options(eng) == got
        for k in [k for k in range(51) if k not in DEFAULTS] + [99]:         # the process-only 2, 11, 12, 26 and the retired 33, 34 among them
            with pytest.raises(_lib.QuberError, match="unknown option key"):
                eng.set_option(k, 1)
            with pytest.raises(_lib.QuberError, match="unknown option key"):
                eng.get_option(k)
    finally:
        eng.close()


def test_plan_time_options_refused_after_finalize():
    h, w = 53, 75                           # the smallest frame of test_gpu_network.py::test_network_vs_oracle_small
    eng = engine.Engine(engine.make_config(h, w, max_batch=1), "cuda:0")
    try:
        eng.load_state_dict(arch.init_state_dict(seed=1))
        start = options(eng)
        for k in DEFAULTS:
            if k in PLAN_TIME:
                with pytest.raises(_lib.QuberError, match="shapes the plan"):
                    eng.set_option(k, start[k] + 1)
                assert eng.get_option(k) == start[k]
            else:
                eng.set_option(k, start[k] + 1)
                assert eng.get_option(k) == start[k] + 1
                eng.set_option(k, start[k])
        assert options(eng) == start
    finally:
        eng.close()
