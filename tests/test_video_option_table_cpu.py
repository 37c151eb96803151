"""Which options of the streamed-video path go together (ssm_amd.video.OPTION_RULES) without a GPU: every single, pair and triple of the
options (tests/video_option_cases.py) gives, through VideoInterpolator and through scripts/interpolate_video.py, byte for byte what the
commit recorded in tests/golden/video_refusals.json gave - the same combinations accepted, the same exception types, the same texts,
and where several rows refuse a triple the same winner - and the table says what the two front ends do, row for row."""
import itertools
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_option_cases as C  # noqa: E402
from ssm_amd import video as V  # noqa: E402

FRONTS = (("api", 0, C.API_VALUES), ("flags", 1, C.FLAG_VALUES))


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_refusals.json")) as f:
        d = json.load(f)
    assert len(d["commit"]) == 40
    return {front: {case: None if i is None else d["messages"][i] for case, i in d[front].items()} for front in ("api", "flags")}


@pytest.fixture(scope="module")
def now():
    import interpolate_video
    return dict(zip(("api", "flags"), C.outcomes(V, interpolate_video)))


@pytest.mark.parametrize("front", ["api", "flags"])
def test_every_combination_is_taken_or_refused_as_recorded(recorded, now, front):
    assert sorted(now[front]) == sorted(recorded[front]), "the cases are the recorded ones"
    assert len(now[front]) == 17 + 136 + 680
    different = {case: (recorded[front][case], got) for case, got in now[front].items() if got != recorded[front][case]}
    assert not different, "%d of %d differ, the first: %s" % (len(different), len(now[front]), sorted(different.items())[:3])


def test_the_cases_cover_the_table():
    """Every option of OPTIONS has a value in the front ends that spell it (detelecine is no argument of the constructor: probe_fields
    gets it as a TelecineSource, tests/test_hip_video_field_order.py), every option of a row is in OPTIONS, FLAG_ORDER is made of the rows
    with a message for the command line, each once."""
    for name, index, values in FRONTS:
        spelt = {k for k, o in V.OPTIONS.items() if o[index] is not None} - ({"detelecine", "flow_beta"} if name == "api" else set())
        assert spelt == set(values)
    for options, others, needs, api, flag in V.OPTION_RULES.values():
        assert set(options + others) <= set(V.OPTIONS) and needs in (True, False) and (api or flag)
    assert sorted(V.FLAG_ORDER) == sorted(k for k, row in V.OPTION_RULES.items() if row[4] is not None)


def _refused_by_the_table(outcome):
    return outcome is not None and (isinstance(outcome, str) or outcome[0] == "ValueError")


@pytest.mark.parametrize("name, index, values", FRONTS)
def test_what_a_row_refuses_the_front_end_refuses(now, name, index, values):
    """For every row with a message for this front end: each of its options with each of the others it refuses, alone, is refused (by
    this row or an earlier one); an option that needs another is refused alone."""
    for row, (options, others, needs, *texts) in V.OPTION_RULES.items():
        if texts[index] is None:
            continue
        for x in options:
            if x not in values:
                continue
            if needs:
                assert _refused_by_the_table(now[name][C.case_id((x,))]), (row, x)
                continue
            for y in others:
                if y in values:
                    case = C.case_id(tuple(k for k in values if k in (x, y)))
                    assert _refused_by_the_table(now[name][case]), (row, case)


@pytest.mark.parametrize("name, index, values", FRONTS)
def test_what_a_front_end_refuses_a_row_names(now, name, index, values):
    """Every single and pair that the front end refuses with the table's exception (the NotImplementedErrors of tile, flow_scale and a
    recurrent model are not the table's) is named by a row with a message for it: a row that refuses has one of the pair among its options
    and the other among its others; a row that needs has one among its options and none of its others in the case."""
    rows = [r for r in V.OPTION_RULES.values() if r[3 + index] is not None]
    for case in (c for c in C.cases(values) if len(c) <= 2):
        if not _refused_by_the_table(now[name][C.case_id(case)]):
            continue
        named = any((x in options and not set(case) & set(others)) if needs else (x in options and y in others)
                    for options, others, needs, *_ in rows for x, y in itertools.permutations(case + (None,) * (2 - len(case))))
        assert named, case


def test_one_sided_rows_are_one_sided_in_the_table():
    """static names active, active does not name static: the message of the pair is static's, in both front ends, whichever is asked first."""
    assert "active" in V.OPTION_RULES["static"][1] and "static" not in V.OPTION_RULES["active"][1]
    assert V.api_refusal({"active": "auto", "static": 0}).startswith("static together with active is not available")
    assert V.flag_refusal({"active": "auto", "static": 0}).startswith("--static does not go together with --active")
    assert V.api_refusal({"static": 0, "upsample_rate": 3, "dedup": None, "flow_scale": 1, "recurrent": False}) is None


def test_the_probe_and_the_tool_share_one_reason():
    """field_probe on a TelecineSource (probe_fields) and --field_probe --detelecine (the tool) give the row's one reason."""
    api = V.api_refusal({"field_probe": 48, "detelecine": True})
    flag = V.flag_refusal({"field_probe": 48, "detelecine": True})
    reason = ": a telecined clip is a mixture of progressive and combed frames by construction, and pulldown removal finds its field order itself"
    assert api == "field_probe together with detelecine is not available" + reason
    assert flag == "--field_probe does not go together with --detelecine" + reason
