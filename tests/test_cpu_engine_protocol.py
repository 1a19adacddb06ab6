"""The protocol of the seventeen engines (srhip/engine.py: Engine, srhip/tape.py: TapeEngine) on CPU nets -- no launch is
made: base classes, gradient buckets, the hipGraph default, which engines carry the attributes whose PRESENCE is the signal
(forward_h16, backward_h16, amp_train_ok, intermediate_outs, taps, last_eval_path), invalidate(), the texts that open every
backward(), all against tests/golden/engine_protocol.json (recorded with protocol_of() before the engines shared a base
class); and the rule of the cached job table (Engine.prep_table) with a stub in place of ops.PrepTable."""
import json
import os

import pytest
import torch

import net_protocol_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_protocol.json")
SIGNALS = ("forward_h16", "backward_h16", "amp_train_ok", "_amp_train_refusal", "intermediate_outs", "taps",
           "layer0_bucket_groups", "last_eval_path")
TAPE_BACKED = ("DBPN", "SRFBN", "ProSR", "ENLCN", "NLSN", "DFCAN", "ACT", "OmniSR", "GRL", "SwinIRTape")
CASES = list(C.NETS) + ["SwinIRTape"]


def make_engine(name):
    if name != "SwinIRTape":
        return C.build(name).engine
    # a window the fused engine does not take: network_swinir.py routes it to the tape graph
    from dlib.models.network_swinir import SwinIR
    torch.manual_seed(0)
    return SwinIR(**dict(C.NETS["SwinIR"][2], window_size=4)).engine


def _raised(fn):
    try:
        fn()
    except Exception as e:      # noqa: BLE001  (the type is what is recorded)
        return [type(e).__name__, str(e)]
    return None


def protocol_of(name):
    eng = make_engine(name)
    out = {"class": type(eng).__name__, "bucket_prefixes": eng.bucket_prefixes(),
           "train_graph_default": bool(getattr(eng, "train_graph_default", False)),   # as ModelPlain reads it
           "has": [a for a in SIGNALS if hasattr(eng, a)]}
    eng.saved = None
    out["backward_unsaved"] = _raised(lambda: eng.backward(None, {}))
    if name not in C.INPUT_GRAD:            # (SwinIR and EDSR return the input gradient)
        eng.saved = object()
        out["backward_need_dx"] = _raised(lambda: eng.backward(None, {}, need_dx=True))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_lists_these_engines(golden):
    assert sorted(golden) == sorted(CASES)
    assert golden["SwinIR"]["class"] == "SwinIREngine" and golden["SwinIRTape"]["class"] == "SwinIRTapeEngine"
    for name in CASES:
        assert golden[name]["backward_unsaved"] == ["AssertionError", "backward() without a saved forward"], name


@pytest.mark.parametrize("name", CASES)
def test_engine_keeps_its_protocol(name, golden):
    from srhip.engine import Engine
    from srhip.tape import TapeEngine
    got = protocol_of(name)
    assert got == golden[name]
    eng = make_engine(name)
    assert isinstance(eng, Engine)
    assert isinstance(eng, TapeEngine) == (name in TAPE_BACKED)
    assert not hasattr(eng, "last_eval_path")
    assert eng.saved is None and eng.prepared is False
    eng.prepared = True
    eng.invalidate()
    assert eng.prepared is False


def test_base_classes_define_no_signal_attribute():
    from srhip.engine import Engine
    from srhip.tape import TapeEngine
    for cls in (Engine, TapeEngine):
        assert [a for a in SIGNALS if hasattr(cls, a)] == []
        assert [a for a in SIGNALS if hasattr(cls(torch.nn.Linear(1, 1)), a)] == []


class _StubTable:
    log = []

    def __init__(self):
        self.jobs = []

    def build(self, device):
        self.log.append(("build", tuple(self.jobs), str(device)))
        return self

    def run(self):
        self.log.append(("run", tuple(self.jobs)))


def test_prep_table_builds_reruns_and_rebuilds(monkeypatch):
    from srhip import ops
    from srhip.engine import Engine
    monkeypatch.setattr(ops, "PrepTable", _StubTable)
    log = _StubTable.log = []
    net = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
    eng = Engine(net)
    fills = []

    def fill(tb):
        fills.append(1)
        tb.jobs.append(len(fills))

    eng.prep_table(fill)
    assert log == [("build", (1,), "cpu"), ("run", (1,))]
    # values changed in place, invalidate(): the same storage, so the table is only run again
    with torch.no_grad():
        net[0].weight.mul_(2.0)
    eng.invalidate()
    del log[:]
    eng.prep_table(fill, before_run=lambda: log.append("before_run"))
    assert log == ["before_run", ("run", (1,))] and len(fills) == 1
    # one parameter's storage replaced: a new table
    net[1].bias.data = net[1].bias.data.clone()
    del log[:]
    eng.prep_table(fill, before_run=lambda: log.append("before_run"))
    assert log == [("build", (2,), "cpu"), "before_run", ("run", (2,))] and len(fills) == 2
    del log[:]
    eng.prep_table(fill)
    assert log == [("run", (2,))] and len(fills) == 2
