"""Which kernel a configuration runs on is pinned: tests/golden/kernel_names.json holds ptm_sweep_kernel_name and ptm_step_kernel_name
of the configurations listed in tests/golden/make_kernel_names.py, recorded before the choice moved into ptm_sweep_plan.hpp.  The same
engines are created again here (configured, never stepped) and must report the same names, string for string."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_kernel_names as MK

pytestmark = pytest.mark.gpu

with open(MK.OUT) as fh:
    RECORDED = json.load(fh)


def test_the_fixture_holds_exactly_the_listed_configurations():
    keys = [MK.key(c) for c in MK.CONFIGS] + ["%s | %s" % (v, MK.key(c)) for v, cs in MK.VARIANTS.items() for c in cs]
    assert len(set(keys)) == len(keys)
    assert set(keys) == set(RECORDED)


@pytest.mark.parametrize("c", MK.CONFIGS, ids=MK.key)
def test_kernel_names_are_the_recorded_ones(c):
    assert MK.names_of(c) == RECORDED[MK.key(c)]


@pytest.mark.parametrize("variant", sorted(MK.VARIANTS))
def test_kernel_names_under_an_environment_switch_are_the_recorded_ones(variant):
    """the engine reads its switches once per process: a child process per variant"""
    got = MK.variant_names(variant)
    assert got == {k: v for k, v in RECORDED.items() if k.startswith(variant + " | ")}
