#!/usr/bin/env python3
"""Record tests/golden/device_refusals.json: what every device-resident entry point of the host layer answers to each fault
and each pair of faults of tests/device_refusal_table.py, from the library that is built in the tree.  No GPU is needed.

Run it on the commit whose answers are to be kept (tests/test_device_refusals.py then holds every later commit to them):

    python tools/record_device_refusals.py            # writes the file
    python tools/record_device_refusals.py --check    # compares instead, exit status 1 on a difference
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import device_refusal_table as T  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "device_refusals.json")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the recorded file instead of writing it")
    args = ap.parse_args()
    table = T.rows()
    nrows = sum(len(t) for t in table.values())
    if args.check:
        with open(GOLDEN) as f:
            want = T.unpack(json.load(f))
        bad = [(e, label) for e, t in table.items() for label, r in t.items() if want.get(e, {}).get(label) != r]
        print(f"{nrows} rows, {len(bad)} differ from {GOLDEN}")
        for e, label in bad[:20]:
            print(f"  {e} [{label}]: {table[e][label]} (recorded: {want.get(e, {}).get(label)})")
        return 1 if bad or {e: list(t) for e, t in table.items()} != {e: list(t) for e, t in want.items()} else 0
    with open(GOLDEN, "w") as f:
        json.dump(T.pack(table), f, separators=(",", ":"))
        f.write("\n")
    print(f"{nrows} rows of {len(table)} entry points -> {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
