"""What the device-resident entry points of the host layer refuse, and in which order: every row of
tests/device_refusal_table.py -- each fault alone and every pair of faults, on a CPU-path factor -- gives the return value,
the Common->status and the message that tests/golden/device_refusals.json records (tools/record_device_refusals.py writes
it: a refusal changes on purpose only, by recording again).  No GPU is needed, and none is touched."""
import json
import os

import device_refusal_table as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_refusals.json")


def test_every_refusal_is_the_recorded_one():
    with open(GOLDEN) as f:
        want = T.unpack(json.load(f))
    got = T.rows()
    assert sorted(got) == sorted(want) == sorted(T.ENTRIES)
    nrows = 0
    for entry in T.ENTRIES:
        assert list(got[entry]) == list(want[entry]), entry            # the same faults, in the same order
        wrong = {label: (row, want[entry][label]) for label, row in got[entry].items() if row != want[entry][label]}
        assert not wrong, (entry, len(wrong), dict(list(wrong.items())[:5]))
        nrows += len(got[entry])
    print(f"{nrows} rows, {len(T.ENTRIES)} entry points")
    # the table is not trivially the same answer everywhere: the pairs tell the checks apart
    for entry in T.ENTRIES:
        assert len({tuple(r) for r in got[entry].values()}) >= 4, entry
