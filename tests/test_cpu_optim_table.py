"""The optimizer table (fullbatchtraining_amd/optimizers.py) answers every combination of optimizer selection and scope-relevant option the
way ``training.py`` did before the table existed: accepted, or the same exception class with the same complete message, the same refusal
first where several apply.  The answers of that commit are tests/golden/optim_scope_parent.json (tests/golden/make_optim_scope.py, which also
defines the cells and how an answer is taken)."""
import json
import os

import pytest

from fullbatchtraining_amd import optimizers
from fullbatchtraining_amd.training import _check_scope, optim_interface
from tests.golden import make_optim_scope as gen

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_scope_parent.json")) as _handle:
    PARENT = json.load(_handle)
CELLS = list(gen.cells())


def test_the_fixture_has_every_cell_of_the_cross_product():
    assert set(optimizers.TABLE) == {("Gradient Descent", "none"), ("Gradient Descent", "wolfe"), ("Adam", "none"), ("GD-AGC", "none"), ("FISTA", "none")}
    assert len(CELLS) == 8 * 3 * 2 * 2 * 2 * 2 and {key for key, *_ in CELLS} == set(PARENT)
    assert {"non-monotone", "restarting", "unknown"} < set(gen.SELECTIONS) and gen.MODIFICATIONS == ("none", "SAM", "LARS")
    refused = {json.dumps(v) for v in PARENT.values() if v != "accepted"}
    assert any(v == "accepted" for v in PARENT.values()) and len(refused) > 20


@pytest.mark.parametrize("selection", list(gen.SELECTIONS))
def test_every_cell_is_answered_like_before_the_table(selection, monkeypatch):
    cells = [c for c in CELLS if c[0].startswith(selection + "|")]
    assert len(cells) == 48
    for key, overrides, multi, world in cells:
        with monkeypatch.context() as m:
            got = gen.answer(_check_scope, optim_interface, lambda cfg: optimizers.select(cfg.hyp).check(cfg.hyp, multi=True), overrides, multi,
                             world, m.setattr)
        assert got == PARENT[key], key
