"""The Python binding hands the C ABI what it handed it at the commit tests/golden/binding_calls.json was recorded from: for every
call of tests/binding_calls_cfg.py the same entry, the same scalars, the same struct contents, the same bytes behind every host
pointer, and the same shape and dtype back -- or the same refusal, code and message.  No GPU: the recorder stands in for the
library's launching entries and forwards the rest."""
import json

import pytest

import binding_calls_cfg as B
import lanczos_hls_amd as L

with open(B.GOLDEN) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def real():
    return L._lib()


def test_the_cases_are_the_fixtures():
    assert sorted(GOLDEN["cases"]) == sorted(B.NAMES)
    assert len(GOLDEN["commit"]) == 40


def test_the_cases_reach_every_launching_entry_the_module_binds(real):
    """... MultiContext's excepted; and the module binds them: each has its argument types."""
    bound = B.launching(L)
    assert GOLDEN["launching"] == bound
    reached = {c["entry"] for r in GOLDEN["cases"].values() for c in r["calls"]}
    assert reached == set(bound), (set(bound) - reached, reached - set(bound))
    for name in bound:
        assert getattr(real, name).argtypes, name
    assert any("error" in r for r in GOLDEN["cases"].values()) and any("returned" in r for r in GOLDEN["cases"].values())


@pytest.mark.parametrize("name,call", B.CASES, ids=B.NAMES)
def test_call_is_the_recorded_one(real, name, call):
    want = GOLDEN["cases"][name]
    got = json.loads(json.dumps(B.run_case(L, real, call)))   # tuples and ints as the fixture holds them
    assert sorted(got) == sorted(want), (got.get("error"), want.get("error"))
    assert got.get("error") == want.get("error")
    assert got.get("returned") == want.get("returned")
    assert [c["entry"] for c in got["calls"]] == [c["entry"] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert len(g["args"]) == len(w["args"]), g["entry"]
        for i, (ga, wa) in enumerate(zip(g["args"], w["args"])):
            if isinstance(wa, dict) and isinstance(ga, dict):
                assert sorted(ga) == sorted(wa), (g["entry"], i)
                for field in wa:
                    assert ga[field] == wa[field], (g["entry"], i, field)
            else:
                assert ga == wa, (g["entry"], i)
