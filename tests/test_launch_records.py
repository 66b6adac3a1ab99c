"""GPU: the same launch for the same call.  tests/golden/launch_records.json holds, for about fifty
calls that between them reach every grid organisation, every variant bit and each flow3 kernel, what
the engine decided (the planning fields of sw_last_stats) and the score, recorded by
tests/golden/gen_launch_records.py and checked against the oracle there.  Each case is replayed here:
every recorded field and the score must be equal.  The decisions depend on the CU count, so the file
states the one it was recorded on."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_launch_records", os.path.join(HERE, "golden", "gen_launch_records.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.PATH) as _f:
    DOC = json.load(_f)
RECORDS = DOC["records"]


@pytest.fixture(scope="module", autouse=True)
def _options(engine):
    """Every case sets all options (timeout 5: a wrongly sized ring launch errors, it does not wait);
    afterwards the defaults, with the session's timeout."""
    yield
    gen.reset(engine)
    engine.set_option("timeout", 5)


def test_records_cover_every_kernel():
    assert gen.coverage_missing(RECORDS) == []
    assert len(gen.FLOW3_KERNELS) == 29 and len(RECORDS) <= 60
    assert [r["case"] for r in RECORDS] == json.loads(json.dumps(gen.cases()))


@pytest.mark.parametrize("idx", range(len(RECORDS)), ids=[r["case"]["name"] for r in RECORDS])
def test_same_launch(engine, idx):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != DOC["cus"]:
        pytest.skip("recorded on %d CUs, this device has %d" % (DOC["cus"], cus))
    rec = RECORDS[idx]
    stats, scores = gen.run_case(engine, idx, rec["case"])
    assert stats == rec["stats"], (rec["case"], gen.flow3_kernel(stats["variant"], stats["C"]))
    assert scores == rec["scores"]
