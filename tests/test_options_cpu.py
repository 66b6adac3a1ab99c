"""CPU: the contract of sw_set_option / sw_get_option (include/algoGPU.h "Tuning knobs"): every key's
default, the values it accepts and the ones it rejects, and that the keys the header documents are
exactly the keys the library knows.  The library loads without a GPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# key -> (default, accepted values, rejected values)
RANGES = {
    "W": (0, (0, 1, 2, 4, 8), (-1, 3, 16)),
    "C": (0, (0, 16, 32, 64), (8, 48)),
    "timeout": (30, (1, 3600), (0, 3601)),
    "blocks": (0, (0, 1, 1 << 40), (-1,)),
    "stall_item": (-1, (-1, 0, 1 << 40), (-2,)),
    "trace_mb": (1024, (1, 3072), (0, 3073)),
    "orient": (0, (0, 2), (-1, 3)),
    "mode": (-1, (-1, 5), (-2, 6)),
    "f2_wgs": (0, (0, 4), (-1, 5)),
    "f2w": (0, (0, 4), (-1, 5)),
    "f2pwg": (-1, (-1, 0, 1), (-2, 2)),
    "ring": (-1, (-1, 0, 1), (-2, 2)),
    "f3split": (-1, (-1, 0, 1), (-2, 2)),
    "linear": (-1, (-1, 0), (-2, 1)),
    "duo_tab": (1, (0, 1, 2), (-1, 3)),
    "duo_prio": (-1, (-1, 0, 6, 20), (-2, 1, 5, 21)),
    "ring_rows": (4096, (512, 1024, 1 << 20), (256, 768, 1 << 21)),
}
RANGES.update({k: (1, (0, 1), (-1, 2)) for k in ("f3", "f3a", "f3hl", "f3slab", "duo_lds", "duo_roles", "duo_raw", "hep")})
RANGES.update({k: (0, (0, 1), (-1, 2)) for k in ("f3rhl", "f3pool", "slab_plain")})
# any value, stored as v != 0
FLAGS = {"bytes": 0, "duo16": 1, "f2stream": 0, "f3pwg": 1}
# any value, stored as given
RAW = {"trace": 0}
DEFAULTS = {**{k: v[0] for k, v in RANGES.items()}, **FLAGS, **RAW}


@pytest.fixture
def sw():
    import concurrentproject_amd as eng
    eng.lib()
    before = {k: eng.get_option(k) for k in DEFAULTS}
    yield eng
    for k, v in before.items():
        eng.set_option(k, v)


def test_defaults_in_a_fresh_process():
    code = ("import json, concurrentproject_amd as sw\n"
            "print(json.dumps({k: sw.get_option(k) for k in %r}))" % sorted(DEFAULTS))
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, capture_output=True, text=True).stdout
    import json
    assert json.loads(out.strip().splitlines()[-1]) == DEFAULTS


@pytest.mark.parametrize("key", sorted(RANGES))
def test_accepts_and_rejects(sw, key):
    _, good, bad = RANGES[key]
    for v in good:
        sw.set_option(key, v)
        assert sw.get_option(key) == v, (key, v)
        for r in bad:
            with pytest.raises(sw.SwError):
                sw.set_option(key, r)
            assert sw.lib().sw_set_option(key.encode(), r) == -1
            assert sw.get_option(key) == v, (key, v, r)


@pytest.mark.parametrize("key", sorted(FLAGS))
def test_flags_store_nonzero(sw, key):
    for v, stored in ((5, 1), (0, 0), (-1, 1), (1, 1), (0, 0)):
        sw.set_option(key, v)
        assert sw.get_option(key) == stored, (key, v)


def test_trace_stores_any_value(sw):
    for v in (0, -1, 5, 1 << 47, -(1 << 40)):
        sw.set_option("trace", v)
        assert sw.get_option("trace") == v


def test_unknown_key(sw):
    L = sw.lib()
    assert L.sw_set_option(b"W", 3) == -1   # a rejected value: -1, and the error text stays as it was
    before = L.sw_last_error()
    assert L.sw_set_option(b"W", 3) == -1 and L.sw_last_error() == before
    assert L.sw_set_option(b"no_such_key", 1) == -1
    assert b"unknown option 'no_such_key'" in L.sw_last_error()
    with pytest.raises(sw.SwError):
        sw.set_option("no_such_key", 1)
    assert sw.get_option("no_such_key") == -1
    assert L.sw_set_option(None, 1) == -1 and L.sw_get_option(None) == -1


def test_header_documents_exactly_the_known_keys(sw):
    """The quoted keys of the "Tuning knobs" comment against the library's own list (sw_option_name)."""
    L = sw.lib()
    import ctypes
    L.sw_option_name.argtypes = [ctypes.c_int]
    L.sw_option_name.restype = ctypes.c_char_p
    names, i = [], 0
    while L.sw_option_name(i) is not None:
        names.append(L.sw_option_name(i).decode())
        i += 1
    assert L.sw_option_name(-1) is None
    assert len(names) == len(set(names)) and set(names) == set(DEFAULTS)
    with open(os.path.join(ROOT, "include", "algoGPU.h")) as f:
        text = f.read()
    comment = text[text.index("Tuning knobs"):text.index("int sw_set_option")]
    documented = set(re.findall(r'"(\w+)"', comment))
    assert documented == set(names)
