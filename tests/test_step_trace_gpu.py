"""The launches of a train step are fixed: for every routing configuration (helpers.TRACE_CONFIGS) the
second train step's kernel launches -- entry point, stream, every integer / float argument, every
pointer as null or not -- equal tests/golden/step_traces.json, recorded by tools/record_step_trace.py
at the commit the file names.  A routing refactor must leave every entry as it is; a change that
moves a route on purpose re-records the file and says so."""
import json
import os

import pytest

from helpers import TRACE_CONFIGS, step_trace

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_traces.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["traces"]


@pytest.mark.parametrize("cid", list(TRACE_CONFIGS))
def test_step_trace(golden, cid):
    got = json.loads(json.dumps(step_trace(cid)))  # (tuples -> lists, as the file holds them)
    want = golden[cid]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{cid}: launch {i} differs"
    assert len(got) == len(want), f"{cid}: {len(got)} launches, the file has {len(want)}"
