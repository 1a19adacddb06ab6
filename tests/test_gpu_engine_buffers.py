"""Nothing an engine allocates was renamed, added or dropped: every key of ``bufs.d``, ``derived.d``, ``ws.d`` and the tape
bank's tables with its shape and dtype (planes: rows, K and operand format too), and the tape pool's buffers by shape, after
the runs of tests/engine_buffer_cases.py, equal tests/golden/engine_buffers.json -- names and shapes recorded on the MI355X
before the engines shared a base class (srhip/engine.py).  One process, one net after the other; the runs are shared by the
cases below."""
import json
import os

import pytest
import torch

import engine_buffer_cases as E

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_buffers.json")


@pytest.fixture(scope="module")
def described():
    from srhip import ops
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    mode = ops.lib.srhip_get_matmul_mode()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        # (through JSON: tuples and lists compare as the file holds them)
        return json.loads(json.dumps({case: E.run(case) for case in E.CASES}))
    finally:
        ops.set_matmul_mode(mode)
        torch.use_deterministic_algorithms(was, warn_only=warn)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_lists_these_cases(golden):
    assert sorted(golden) == sorted(E.CASES)


@pytest.mark.parametrize("case", E.CASES)
def test_engine_allocates_what_it_did(case, described, golden):
    got, want = described[case], golden[case]
    assert sorted(got) == sorted(want)
    for table in want:
        if table == "pool":
            assert got[table] == want[table], f"{case}: tape pool buffers by shape"
            continue
        have, had = {e[0]: e[1:] for e in got[table]}, {e[0]: e[1:] for e in want[table]}
        assert sorted(have) == sorted(had), (f"{case} {table}: added {sorted(set(have) - set(had))}, "
                                            f"dropped {sorted(set(had) - set(have))}")
        for k in had:
            assert have[k] == had[k], f"{case} {table}[{k!r}]: {have[k]} was {had[k]}"
