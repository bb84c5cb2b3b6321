"""CPU: the host side of the mixer entries answers what the parent of the mixer-plan refactor answered.

tests/golden/mixer_host_parent.json was recorded by tests/mixer_host_grid.py from a checkout of the commit it names: under
``mixer_lds`` = 1 and 0, psf_mixer_fwd_plan / _workspace and their bf16 twins over shapes that cross every limit from both sides,
and the return code and full psf_last_error() text of psf_mixer_fwd_f32 / psf_mixer_fwd_in_f32 / psf_mixer_fwd_bf16 for calls
with fake pointers that are answered before the first HIP call — single faults, and pairs that pin the order of the checks. This
test replays the grid on the tree. Nothing is launched: a call that slipped past validation would show as a HIP error code."""
import json
import os
import re
import threading

import pytest

import mixer_host_grid as grid

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixer_host_parent.json")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _set_knob(value):
    from sparsefactorization_amd import _lib
    _lib.set_tuning("mixer_lds", value)


def test_fixture_names_its_parent_and_holds_every_plan_every_code_and_both_knob_values(recorded):
    assert re.fullmatch(r"[0-9a-f]{40}", recorded["parent"])
    assert os.path.getsize(FIXTURE) < 512 * 1024
    answers = recorded["answers"]
    assert list(answers) == [grid.shape_label(s) for s in grid.shape_cases()] + [lab for lab, _e, _a in grid.call_cases()]
    assert 1000 <= len(answers) <= 3000
    per_knob = [a.split(" ", 1)[1] for v in answers.values() for a in v.split(" || ")]
    plans = {tuple(a.split(",")[0::2]) for a in per_knob if re.fullmatch(r"[-0-9,]+", a)}
    assert {p[0] for p in plans} == {"0", "1", "2"} and {p[1] for p in plans} == {"0", "2"}
    assert {a.split(":")[0] for a in per_knob if ":" in a} == {"0", "-1", "-2", "-3", "-4", "-7"}  # (PSF_E_TUNING comes after the pack launch)
    assert any(v.startswith("lds=1 ") and " || lds=0 " in v for v in answers.values())  # the knob changes some answers
    for entry in grid.ENTRIES:
        assert sum(lab.startswith(entry + " ") for lab in answers) >= 100


def test_every_plan_workspace_code_and_error_text_is_the_parents(lib, recorded):
    want = recorded["answers"]
    got = grid.answers(lib, _set_knob)
    wrong = [(lab, a, want.get(lab, "<not recorded>")) for lab, a in got.items() if a != want.get(lab, "<not recorded>")]
    for lab, a, w in wrong[:40]:
        print(f"{lab}:\n    tree:   {a}\n    parent: {w}")
    assert not wrong and len(got) == len(want), f"{len(wrong)} of {len(want)} cases differ from the parent's (the first are printed above)"


def test_entries_stay_honest_while_another_thread_flips_mixer_lds(lib, recorded):
    """One thread flips ``mixer_lds`` 3000 times; the other repeats a recipe call on a per-step-only shape (N = 16384), a recipe call
    with a misaligned V0 on an LDS shape (rejected under either value, with another code) and the two plan queries. Every answer
    must be one the single-threaded library gives for that call — the recorded ones — and every error text that code's text.
    (This cannot catch a knob read twice inside one call; it keeps the entries honest under concurrent writes. That each entry
    takes one snapshot() is seen in psf_chord.hip: no other read of the knob exists.)"""
    answers = recorded["answers"]
    cases = {lab: (entry, c) for lab, entry, c in grid.call_cases()}

    def allowed(*labels):
        return {a.split(" ", 1)[1] for lab in labels for a in answers[lab].split(" || ")}

    step = "psf_mixer_fwd_in_f32 tokens step: a recipe on a per-step shape"
    on, off = "psf_mixer_fwd_in_f32 tokens lds: V0 misaligned", "psf_mixer_fwd_in_f32 tokens lds: a recipe with mixer_lds=0 + V0 misaligned"
    assert cases[on][1] == dict(cases[off][1], lds=(1,)) and len(allowed(step)) == 1 and len(allowed(on, off)) == 2
    calls = [(cases[step], allowed(step)), (cases[on], allowed(on, off))]
    N, E, M, C, L = grid.SHAPES["both"]
    h = grid.h_table(M, 32)
    errors = []

    def worker():
        for _ in range(3000):
            for (entry, c), ok in calls:
                rc = grid.ask_call(lib, entry, c)
                if f"{rc}:{lib.psf_last_error().decode()}" not in ok:
                    errors.append(f"{entry}: {rc}:{lib.psf_last_error().decode()}")
            if lib.psf_mixer_fwd_plan(N, E, M, h, C, L) not in (1, 2) or lib.psf_mixer_fwd_bf16_plan(N, E, M, h, C, L) not in (0, 2):
                errors.append("plan")

    def knob_worker():
        for i in range(3000):
            if lib.psf_set_tuning(b"mixer_lds", i & 1) != 0:
                errors.append("set_tuning")

    threads = [threading.Thread(target=f) for f in (worker, knob_worker)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        _set_knob(1)
    assert not errors, sorted(set(errors))[:10]
    both = answers[grid.shape_label((N, E, M, 32, C, L))]  # (the plans asked above: 2 / 2 with the knob on, 1 / 0 with it off)
    assert re.fullmatch(r"lds=1 2,\d+,2,\d+ \|\| lds=0 1,\d+,0,\d+", both), both
