"""The error codes AND the whole messages of the camera renders that take views, call by call: the list of
tests/render_call_error_cases.py replayed against the recording beside it (tests/render_call_errors.json).  The kinds'
test_errors_come_in_order pin the order of the errors by keywords; this pins every byte of what ort_last_error() says, so that
the code that assembles the messages can move without changing one.  No GPU: every call ends before any device work."""
import json
import os

import render_call_error_cases as cases
from conftest import HERE


def test_codes_and_messages_are_the_recorded_ones(api):
    want = json.load(open(os.path.join(HERE, "render_call_errors.json")))
    got = cases.replay(api)
    assert set(got) == set(want) == {e[0] for e in cases.entry_points()} and len(got) == 18
    for name in sorted(want):
        for state in ("committed", "uncommitted"):
            assert [r[0] for r in got[name][state]] == [r[0] for r in want[name][state]], (name, state)   # the list itself
            for (label, rc, msg), (_, want_rc, want_msg) in zip(got[name][state], want[name][state]):
                assert rc == want_rc, (name, state, label, rc, msg)
                assert (None if msg is None else msg.encode()) == (None if want_msg is None else want_msg.encode()), (name, state, label)
    # the recording is not vacuous: every code the contract names, and the state errors on the scene they belong to
    codes = {r[1] for e in want.values() for rows in e.values() for r in rows}
    assert codes == {api.OK, api.ERR_INVALID, api.ERR_UNSUPPORTED, api.ERR_STATE, api.ERR_NO_DEVICE}
    for name, e in want.items():
        assert api.ERR_NO_DEVICE in {r[1] for r in e["committed"]} and api.ERR_STATE not in {r[1] for r in e["committed"]}, name
        assert api.ERR_STATE in {r[1] for r in e["uncommitted"]} and api.ERR_NO_DEVICE not in {r[1] for r in e["uncommitted"]}, name
