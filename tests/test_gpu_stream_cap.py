"""Every grid-capped streaming kernel past its cap (tests/stream_helpers.py holds the cap table, the cases, the references and the checker;
tests/test_stream_cap_cpu.py proves them without a GPU).  Each case asserts the trip count it was written for -- exactly one full trip,
a second trip, three or more -- launches the entry through the C-ABI and compares whole allocations, sentinels included, with a plain
reference: bit for bit wherever the contract is one rounded operation per step, else within the project's existing bounds against float64.
Each test prints the worst |got - ref| / bound it saw."""
import os

import pytest

import stream_helpers as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip, oracle):
    return S.Backend(hip, oracle.lib())


def test_the_gathers_caps_are_the_defaults():
    """the release library reads no environment variable; a lab build would take the gathers' caps from these two"""
    assert "FFH_EMB_FWD_CAP" not in os.environ and "FFH_EMB_BAGS_CAP" not in os.environ


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_stream_case(dev, c):
    assert dev.device and dev.lib.backend != "oracle-cpu"
    worst = S.run_case(dev, c)
    assert worst <= 1.0
