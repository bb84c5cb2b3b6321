"""CPU: the producer route fused_mlp gives a call is the one the parent of the route-table refactor gave it.

tests/golden/producer_routes_parent.json was recorded by tests/producer_route_grid.py from a checkout of the commit it names: per
case the booleans of eligible / trainable / wide_ok / bf16_eligible / stackable and the name of the first true one in the order
PSFNet tried them, over a grid that crosses every limit of the predicates from both sides. This test replays the grid on the
tree: every boolean equal, and ``fused_mlp.route`` naming the recorded route. No device is touched: nothing is launched."""
import json
import os
import re

import pytest

import producer_route_grid as grid

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "producer_routes_parent.json")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_fixture_names_its_parent_and_reaches_every_route_and_both_answers_of_every_predicate(recorded):
    assert re.fullmatch(r"[0-9a-f]{40}", recorded["parent"])
    assert recorded["predicates"] == list(grid.PREDICATES)
    assert os.path.getsize(FIXTURE) < 100 * 1024
    bits, names = zip(*(a.split(":") for a in recorded["answers"].values()))
    assert set(names) == set(grid.NAMES) | {"None"}
    for i, p in enumerate(grid.PREDICATES):
        assert {b[i] for b in bits} == {"0", "1"}, f"{p} is not recorded both true and false"
    assert list(recorded["answers"]) == [grid.label(c) for c in grid.cases()]  # the grid of this tree is the recorded one


def test_every_predicate_and_the_route_are_the_parents(recorded):
    from sparsefactorization_amd import fused_mlp
    want = recorded["answers"]
    wrong = []
    for lab, answer, named in grid.answers(fused_mlp, also=fused_mlp.route):
        if answer != want.get(lab, "<not recorded>") or str(named) != answer.split(":")[1]:
            wrong.append((lab, answer, named, want.get(lab, "<not recorded>")))
    for lab, answer, named, w in wrong[:40]:
        print(f"{lab}:\n    tree:   {answer}, route() = {named}\n    parent: {w}")
    assert not wrong, f"{len(wrong)} of {len(want)} cases differ from the parent's (the first are printed above)"
