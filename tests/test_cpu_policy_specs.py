"""CPU: the test policies of tests/policy_specs.py are what they were when
tests/golden/policy_specs.json was written (by tests/golden/make_policy_specs.py, on the three
per-feature modules that policy_specs replaced): ONNX bytes, weights, expected view, device
weights, observations and, for the integer probes, inputs, int64 answers with and without a
zeroed unit, and the exactness bound. One case per model; a failure names what moved.
"""
import importlib.util
import json
import os

import pytest

import policy_specs as ps
from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_policy_specs", os.path.join(GOLDEN, "make_policy_specs.py"))
make = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make)

with open(make.OUT) as _fh:
    PINNED = json.load(_fh)


def test_every_model_is_pinned_once():
    names = [n for _, n, _ in make.names()]
    assert len(names) == len(set(names)) == 22
    assert list(PINNED) == names
    assert {n: r["family"] for n, r in PINNED.items()} == {n: f for f, n, _ in make.names()}
    assert all(ps.FAMILIES[f] is ps.family(n) for f, n, _ in make.names())


@pytest.mark.parametrize("family,name,probe", make.names(), ids=[n for _, n, _ in make.names()])
def test_model_did_not_move(family, name, probe):
    got, want = make.record(family, name, probe), PINNED[name]
    assert sorted(got) == sorted(want)
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, (name, moved)


def test_model_bytes_are_deterministic():
    for name in ("ea_front", "res_skip"):
        assert ps.model_bytes(name) == ps.model_bytes(name)
