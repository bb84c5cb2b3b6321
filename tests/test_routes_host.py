"""CPU: the routes the host dispatcher (csrc/psf_chord.hip) names are the ones the parent of the dispatcher refactor named.

tests/golden/routes_parent.json was recorded by tests/route_grid.py from a library built from the commit it names: per case the
return code and string of psf_describe_fwd / psf_describe_bwd / psf_describe_chain_fwd_dtype and the return values of
psf_chord_chain_bwd_supported, psf_mixer_fwd_plan and psf_mixer_fwd_workspace, over a grid that reaches every branch of the
planning code (route_grid.FAMILIES), under the default knobs and with one knob off its default at a time. This test replays
the grid on the tree's library and wants every answer equal. No device is touched: none of these entries launches."""
import os
import re

import pytest

import route_grid

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "routes_parent.json")


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


@pytest.fixture(scope="module")
def recorded():
    return route_grid.load(FIXTURE)


def test_fixture_names_its_parent_and_reaches_every_kernel_family(recorded):
    parent, strings, groups = recorded
    assert re.fullmatch(r"[0-9a-f]{40}", parent)
    assert route_grid.missing_families(strings) == []
    names = {g.split("/", 1)[0] for g in groups}
    assert names == {name for name, _knob, _value in route_grid.settings()}  # the defaults and every knob at every other legal value
    assert os.path.getsize(FIXTURE) < 400 * 1024


def test_every_route_is_the_parents(lib, recorded):
    _parent, strings, groups = recorded
    saved = {k: lib.psf_get_tuning(k.encode()) for k in route_grid.KNOBS}
    position, wrong, seen = {}, [], 0
    try:
        for group, label, answer in route_grid.replay(lib):
            i = position.get(group, 0)
            position[group] = i + 1
            seen += 1
            want = strings[groups[group][i]] if group in groups and i < len(groups[group]) else "<not recorded>"
            if answer != want:
                wrong.append((group, label, answer, want))
    finally:  # (replay restores each knob as it goes; this holds whatever it raised)
        for k, v in saved.items():
            lib.psf_set_tuning(k.encode(), v)
    for group, label, answer, want in wrong[:40]:
        print(f"{group} {label}:\n    tree:   {answer}\n    parent: {want}")
    assert not wrong, f"{len(wrong)} of {seen} cases differ from the parent's (the first are printed above)"
    assert position == {g: len(ix) for g, ix in groups.items()}  # every recorded case was replayed
    assert {k: lib.psf_get_tuning(k.encode()) for k in route_grid.KNOBS} == saved
