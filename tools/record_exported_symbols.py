#!/usr/bin/env python3
"""Record tests/golden/exported_symbols.json: the cholmod_hip_* entry points that the product library and the test-hooks
library export (`nm -D --defined-only`), from the libraries that are built in the tree.  No GPU is needed.

Run it on the commit whose exported surface is to be kept (tests/test_exported_symbols.py then holds every later commit to
it):

    python tools/record_exported_symbols.py            # writes the file
    python tools/record_exported_symbols.py --check    # compares instead, exit status 1 on a difference
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import exported_symbols as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the recorded file instead of writing it")
    args = ap.parse_args()
    got = {lib: E.exported(lib) for lib in E.LIBS}
    if args.check:
        with open(E.GOLDEN) as f:
            want = json.load(f)
        bad = 0
        for lib in E.LIBS:
            diff = sorted(set(got[lib]) ^ set(want.get(lib, [])))
            print(f"{lib}: {len(got[lib])} entry points, {len(diff)} differ from {E.GOLDEN}")
            for s in diff:
                print(f"  {s}: {'not recorded' if s in got[lib] else 'missing'}")
            bad += len(diff)
        return 1 if bad or sorted(want) != sorted(E.LIBS) else 0
    with open(E.GOLDEN, "w") as f:
        json.dump(got, f, indent=0)
        f.write("\n")
    print(", ".join(f"{lib}: {len(s)}" for lib, s in got.items()) + f" entry points -> {E.GOLDEN} ({os.path.getsize(E.GOLDEN)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
