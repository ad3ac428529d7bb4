"""What every entry point answers to a request for a start, a trace or both — every execution mode, the q counts at which the rule
turns, the C entries and the Python layers over them — against the record taken before the rule was stated in one place
(tests/golden/start_trace_requests.json, written by tools/record_start_trace_requests.py; this test only reads it).  The questions
are asked by that tool's answers(): the library stubbed for the Python entries, "passes" for a C entry that gets as far as the
device, so the record holds with and without one."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_request_is_answered_as_recorded():
    spec = importlib.util.spec_from_file_location("record_start_trace_requests", os.path.join(ROOT, "tools", "record_start_trace_requests.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "start_trace_requests.json")) as f:
        record = json.load(f)
    want = {tuple(row[:4]): record["answers"][row[4]] for row in record["rows"]}
    assert len(want) == len(record["rows"]) == len(list(tool.questions()))
    got = {(e, r, m, n): a for e, r, m, n, a in tool.answers()}
    assert set(got) == set(want)
    wrong = [(k, got[k], want[k]) for k in want if got[k] != want[k]]
    for k, g, w in wrong[:10]:
        print("%s\n  now:      %s\n  recorded: %s" % (k, g, w))
    assert not wrong, "%d of %d answers changed" % (len(wrong), len(want))
